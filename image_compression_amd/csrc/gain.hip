// Gain units (Cui et al. 2021): per-channel gain vectors interpolated between S learnt levels, and the scaling of a
// latent by them (ic_gain_vector*, ic_channel_scale*).
//   * The gain-vector rule (codec.py states it for the container): for a table t (S, C) and a quality q held as
//     fp32, s = min((int)floorf(q), S - 2), f = q - s, a = fma(f, t[s+1][c], fl((1 - f) t[s][c])): the two
//     subtractions and the lower level's product rounded once each (fp_rn.h), the upper level's product fused with the
//     sum and rounded once; g[c] = 1.0f where a == 0 and expf(a) elsewhere.  Both sides of the codec run this kernel on
//     the fp32 quality the stream stores, so they hold the same gain bits; a model with zero tables has gains of
//     exactly 1.0.  The fused step is written out (fmaf): the rule is the format's, not the compiler's choice.
//   * out = x * g is one fp32 multiplication per element (__fmul_rn), the gain broadcast over the positions.
//   * No floating-point atomics: every gradient sum runs in a fixed order (dtable: one thread per (s, c) over the
//     qualities in ascending order; dg: per block over its positions, then one thread per (row, c) over the
//     blocks' partial sums in a workspace), so it is bitwise the same from run to run.
// x is dense channels-last storage (N, P, C): P positions per image, channel fastest.  The scaling kernels are
// grid-stride and HBM-bound: 16-byte accesses when every pointer is 16-byte aligned and C % 4 == 0 (a group of
// four never straddles a position), scalar otherwise.
#include <algorithm>

#include "common.h"
#include "fp_rn.h"
#include "../../include/imgcomp.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_MAXBLOCKS = 1024;
constexpr int GN_MAXQ = 64;        // qualities per launch: they travel as kernel arguments
constexpr int GN_POS = 64;         // positions per block of the gradient's first stage, at least
constexpr int GN_MAXPART = 2048;   // blocks of the first stage over all images, about
constexpr int GN_BATCH = 16;       // partial sums the second stage loads before it adds them

struct GainQ {
  float q[GN_MAXQ];
};

// (s, f) of the rule: the lower level and the weight of the upper one
__device__ __forceinline__ void level_of(float q, int S, int& s, float& f) {
  s = min((int)floorf(q), S - 2);
  f = __fsub_rn(q, (float)s);
}

// out[k0 + k][c] for the nq qualities of one launch
__global__ void __launch_bounds__(GN_THREADS) gain_vector_k(const float* __restrict__ table, int S, int C, GainQ qs,
                                                            int nq, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)nq * C) return;
  const int k = (int)(i / C), c = (int)(i % C);
  int s;
  float f;
  level_of(qs.q[k], S, s, f);
  const float a = fmaf(f, table[(long long)(s + 1) * C + c], mul_rn(__fsub_rn(1.0f, f), table[(long long)s * C + c]));
  out[i] = a == 0.0f ? 1.0f : expf(a);
}

// dtable[s][c] (+)= sum over the launch's qualities, ascending, of dout g w(k, s): dg/da = g (1 = e^0 where a == 0)
__global__ void __launch_bounds__(GN_THREADS) gain_vector_bwd_k(const float* __restrict__ g, const float* __restrict__ dout,
                                                                int S, int C, GainQ qs, int nq, int first,
                                                                float* __restrict__ dtable) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)S * C) return;
  const int s = (int)(i / C), c = (int)(i % C);
  float acc = first ? 0.0f : dtable[i];
  for (int k = 0; k < nq; ++k) {
    int sk;
    float f;
    level_of(qs.q[k], S, sk, f);
    if (s != sk && s != sk + 1) continue;
    const float w = s == sk ? __fsub_rn(1.0f, f) : f;
    acc += dout[(long long)k * C + c] * g[(long long)k * C + c] * w;
  }
  dtable[i] = acc;
}

// out = x * g[row of image blockIdx.y]; `len` = P * C elements per image
template <bool VEC>
__global__ void __launch_bounds__(GN_THREADS) channel_scale_k(const float* __restrict__ x, const float* __restrict__ g,
                                                              long long len, int C, int per_image,
                                                              float* __restrict__ out) {
  const long long base = (long long)blockIdx.y * len;
  const float* xs = x + base;
  float* os = out + base;
  const float* gs = g + (per_image ? (long long)blockIdx.y * C : 0);
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  constexpr int W = VEC ? 4 : 1;
  // the channel of a thread's element advances by (stride * W) % C per iteration: no division in the loop
  const int step = (int)((stride * W) % C);
  int c = (int)((tid * W) % C);
  const long long n = len / W;   // VEC: C % 4 == 0, so len % 4 == 0
  for (long long i = tid; i < n; i += stride) {
    if (VEC) {
      const floatx4v a = reinterpret_cast<const floatx4v*>(xs)[i];
      const floatx4v b = *reinterpret_cast<const floatx4v*>(gs + c);
      floatx4v o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fmul_rn(a[j], b[j]);
      reinterpret_cast<floatx4v*>(os)[i] = o;
    } else {
      os[i] = __fmul_rn(xs[i], gs[c]);
    }
    c += step;
    if (c >= C) c -= C;
  }
}

// First stage of the gradient.  Block (b, n) takes the positions [b * ppb, min(P, (b + 1) * ppb)) of image n:
// dx = dy * g there, and part[(n * gridDim.x + b)][c] = sum of dy x over them.  Thread (tx, ty) owns the channel
// groups tx, tx + TX, ... (a group: W channels) and the positions ty, ty + TY, ... of the slab; the TY sums of a
// group are added in ascending ty.
template <bool VEC>
__global__ void __launch_bounds__(GN_THREADS) channel_scale_bwd_k(const float* __restrict__ x, const float* __restrict__ g,
                                                                  const float* __restrict__ dy, long long P, int C,
                                                                  int per_image, long long ppb, float* __restrict__ dx,
                                                                  float* __restrict__ part) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ float red[GN_THREADS * W];
  const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
  const int G = C / W;
  const long long base = (long long)blockIdx.y * P * C;
  const float* gs = g + (per_image ? (long long)blockIdx.y * C : 0);
  float* ps = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * C;
  const long long p0 = (long long)blockIdx.x * ppb, p1 = p0 + ppb < P ? p0 + ppb : P;
  for (int cg0 = 0; cg0 < G; cg0 += TX) {   // the same trip count for every thread of the block
    const int cg = cg0 + tx;
    const bool on = cg < G;
    float acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = 0.0f;
    if (on) {
      float gv[W];
#pragma unroll
      for (int j = 0; j < W; ++j) gv[j] = gs[cg * W + j];
      for (long long p = p0 + ty; p < p1; p += TY) {
        const long long at = base + p * C + (long long)cg * W;
        if (VEC) {
          const floatx4v a = *reinterpret_cast<const floatx4v*>(x + at);
          const floatx4v d = *reinterpret_cast<const floatx4v*>(dy + at);
          floatx4v o;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = __fmul_rn(d[j], gv[j]);
            acc[j] += d[j] * a[j];
          }
          *reinterpret_cast<floatx4v*>(dx + at) = o;
        } else {
          const float d = dy[at];
          dx[at] = __fmul_rn(d, gv[0]);
          acc[0] += d * x[at];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) red[(ty * TX + tx) * W + j] = acc[j];
    __syncthreads();
    if (on && ty == 0) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        float s = 0.0f;
        for (int r = 0; r < TY; ++r) s += red[(r * TX + tx) * W + j];
        ps[cg * W + j] = s;
      }
    }
    __syncthreads();
  }
}

// Second stage: dg[row][c] = the partial sums of the row's images (all of them when the row is shared), image by
// image and block by block in ascending order
__global__ void __launch_bounds__(GN_THREADS) channel_scale_dg_k(const float* __restrict__ part, int N, int nb, int C,
                                                                 int per_image, float* __restrict__ dg) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int rows = per_image ? N : 1;
  if (i >= (long long)rows * C) return;
  const int row = (int)(i / C), c = (int)(i % C);
  const long long first = per_image ? (long long)row * nb : 0, count = per_image ? nb : (long long)N * nb;
  // GN_BATCH loads in flight, then their additions in order: the loop is bound by the latency of a load, not by
  // the sum (one load at a time: 50 us for 192 partial sums per thread, measured)
  float s = 0.0f;
  for (long long b0 = 0; b0 < count; b0 += GN_BATCH) {
    float v[GN_BATCH];
#pragma unroll
    for (int u = 0; u < GN_BATCH; ++u) v[u] = b0 + u < count ? part[(first + b0 + u) * C + c] : 0.0f;
#pragma unroll
    for (int u = 0; u < GN_BATCH; ++u) s += v[u];
  }
  dg[i] = s;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- the host checks, before any launch
bool quality_ok(const float* q, int nq, int S) {
  if (!q || nq < 1 || S < 2) return false;
  for (int k = 0; k < nq; ++k)
    if (!(q[k] >= 0.0f && q[k] <= (float)(S - 1))) return false;   // NaN fails both comparisons
  return true;
}

bool table_ok(int S, int C, int nq) {
  return S >= 2 && C >= 1 && nq >= 1 && (long long)S * C <= 0x7fffffffll && (long long)nq * C <= 0x7fffffffll;
}

bool scale_shape_ok(long long N, long long P, int C, int g_rows) {
  if (N < 1 || N > 65535 || P < 1 || C < 1 || (g_rows != 1 && g_rows != N)) return false;
  return P <= 0x7fffffffffffffffll / C / N;
}

// blocks per image of the gradient's first stage: a function of the shape alone (the workspace query and the
// launch agree on it)
long long bwd_blocks(long long N, long long P) {
  return std::max<long long>(1, std::min<long long>((P + GN_POS - 1) / GN_POS, std::max<long long>(1, GN_MAXPART / N)));
}

GainQ launch_qualities(const float* q, int k0, int n) {
  GainQ qs;
  for (int k = 0; k < GN_MAXQ; ++k) qs.q[k] = k < n ? q[k0 + k] : 0.0f;
  return qs;
}

}  // namespace

extern "C" {

int ic_gain_vector(const float* table, int S, int C, const float* q, int nq, float* out, void* stream) {
  if (!table || !out || !table_ok(S, C, nq) || !quality_ok(q, nq, S)) return IC_ERR_ARG;
  for (int k0 = 0; k0 < nq; k0 += GN_MAXQ) {
    const int n = std::min(GN_MAXQ, nq - k0);
    hipLaunchKernelGGL(gain_vector_k, dim3(ic_cdiv((long long)n * C, GN_THREADS)), dim3(GN_THREADS), 0,
                       (hipStream_t)stream, table, S, C, launch_qualities(q, k0, n), n, out + (long long)k0 * C);
    IC_CHECK_LAUNCH();
  }
  return IC_OK;
}

int ic_gain_vector_bwd(const float* g, const float* dout, int S, int C, const float* q, int nq, float* dtable,
                       void* stream) {
  if (!g || !dout || !dtable || !table_ok(S, C, nq) || !quality_ok(q, nq, S)) return IC_ERR_ARG;
  for (int k0 = 0; k0 < nq; k0 += GN_MAXQ) {
    const int n = std::min(GN_MAXQ, nq - k0);
    hipLaunchKernelGGL(gain_vector_bwd_k, dim3(ic_cdiv((long long)S * C, GN_THREADS)), dim3(GN_THREADS), 0,
                       (hipStream_t)stream, g + (long long)k0 * C, dout + (long long)k0 * C, S, C,
                       launch_qualities(q, k0, n), n, k0 == 0 ? 1 : 0, dtable);
    IC_CHECK_LAUNCH();
  }
  return IC_OK;
}

int ic_channel_scale(const float* x, const float* g, long long N, long long P, int C, int g_rows, float* out,
                     void* stream) {
  if (!x || !g || !out || !scale_shape_ok(N, P, C, g_rows)) return IC_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(out);
  const long long work = P * C / (vec ? 4 : 1);
  const dim3 grid((unsigned)std::min<long long>((work + GN_THREADS - 1) / GN_THREADS, GN_MAXBLOCKS), (unsigned)N);
  const int per_image = g_rows != 1 ? 1 : 0;
  if (vec)
    hipLaunchKernelGGL(channel_scale_k<true>, grid, dim3(GN_THREADS), 0, (hipStream_t)stream, x, g, P * C, C, per_image,
                       out);
  else
    hipLaunchKernelGGL(channel_scale_k<false>, grid, dim3(GN_THREADS), 0, (hipStream_t)stream, x, g, P * C, C, per_image,
                       out);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

size_t ic_channel_scale_bwd_ws(long long N, long long P, int C, int g_rows) {
  if (!scale_shape_ok(N, P, C, g_rows)) return 0;
  return (size_t)(N * bwd_blocks(N, P)) * (size_t)C * sizeof(float);
}

int ic_channel_scale_bwd(const float* x, const float* g, const float* dy, long long N, long long P, int C, int g_rows,
                         float* dx, float* dg, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !g || !dy || !dx || !dg || !ws || !scale_shape_ok(N, P, C, g_rows)) return IC_ERR_ARG;
  if (ws_bytes < ic_channel_scale_bwd_ws(N, P, C, g_rows)) return IC_ERR_WORKSPACE;
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(dy) && aligned16(dx);
  const int groups = C / (vec ? 4 : 1);
  int tx = 1;
  while (tx < 64 && tx < groups) tx *= 2;
  const long long nb = bwd_blocks(N, P), ppb = (P + nb - 1) / nb;
  const dim3 grid((unsigned)nb, (unsigned)N), block(tx, GN_THREADS / tx);
  const int per_image = g_rows != 1 ? 1 : 0;
  float* part = (float*)ws;
  if (vec)
    hipLaunchKernelGGL(channel_scale_bwd_k<true>, grid, block, 0, (hipStream_t)stream, x, g, dy, P, C, per_image, ppb, dx,
                       part);
  else
    hipLaunchKernelGGL(channel_scale_bwd_k<false>, grid, block, 0, (hipStream_t)stream, x, g, dy, P, C, per_image, ppb, dx,
                       part);
  IC_CHECK_LAUNCH();
  hipLaunchKernelGGL(channel_scale_dg_k, dim3(ic_cdiv((long long)g_rows * C, GN_THREADS)), dim3(GN_THREADS), 0,
                     (hipStream_t)stream, part, (int)N, (int)nb, C, per_image, dg);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
