// Checkerboard context model, inference: the whole context in one launch (ic_context_fwd), computing only
// what is used and every output by arithmetic that does not depend on the batch size.
//
// Tensors are dense channels-last storage (n, i, j, c) of N x H x W x C fp32; position (i, j) is an anchor when
// i + j is even.  At an anchor mu = mu_h and sigma = sigma_h, copied bit for bit.  At a non-anchor, with t running
// over the 12 taps (ky, kx) of the 5 x 5 window whose offset (ky-2) + (kx-2) is odd (the taps that reach anchors),
// in ascending (ky, kx) order, and a neighbour outside the map contributing 0:
//     a[o] = b_mean[o]  + sum_t sum_c W_mean[o,c,ky,kx]  * y_in[c, nbr]
//     b[o] = b_scale[o] + sum_t sum_c W_scale[o,c,ky,kx] * |y_in[c, nbr] - mu_h[c, nbr]|      (one __fsub_rn)
//     mu = __fadd_rn(mu_h, a),  sigma = __fmul_rn(sigma_h, expf(clamp(b, -L, +L))),  L = IC_CKBD_LOG_SCALE_LIMIT
// which is ic_ckbd_input_fwd, the two context convs and ic_ckbd_params_fwd (ckbd.hip) with the 13 dead taps, the
// non-anchor inputs and the anchor outputs left out: a quarter of the convs' multiply-adds.  The 13 same-parity taps of
// the weights and the non-anchors of y_in are never read.
//
// Arithmetic: exact fp32 products, fp32 accumulation, whatever the model's COMPUTE_DTYPE is
// (v_mfma_f32_32x32x2_f32: each accumulator is a k-ordered chain of fmaf, starting from the bias).
//
// Tile map.  The non-anchors of ONE image are numbered q = 0 .. H W / 2 - 1 in ascending (i, j) order (the order of
// ic_ckbd_gather) and cut into tiles of 32; a block never holds positions of two images.  The work of a tile is
// 2 * ceil(C / 32) units, one per head (mean, scale) and 32 output channels; one wave computes one unit, a
// 32 x 32 accumulator over K = 12 taps x 8 ceil(C / 8) channels (channels past C are zero in the packed weights
// and read as zero from the inputs), four waves share a block and so the tile's inputs in L1.  Grid: x = tiles x
// ceil(units / 4), y = image.  The tile grid of an image and the k order of every accumulator depend on (H, W, C)
// only: there is no split of K, no atomic, and N enters only as the number of grid rows -- so image n's outputs
// are bit for bit the same whatever the batch and wherever in it the image lies.
// The wave that owns (head, channels) of tile m also copies that head's hyperprior parameter at anchors
// 32 m .. 32 m + 31 (anchors are numbered like the non-anchors and are at most one more), so the launch writes
// every element of both outputs exactly once.
//
// Weights: the live taps repacked (pack_k) to [head][tap][channel group of 8][output, padded to 32][8 channels], so
// a wave's B fragment of four k-steps is one 16-byte load per lane and 1 KiB contiguous per wave.  The pack lives in
// a caller-owned workspace of ic_context_ws(C) bytes; with `packed` != 0 the workspace already holds the pack of
// these weights and only the context kernel is launched (the eval weight cache).
#include <algorithm>
#include <cstdint>
#include <initializer_list>

#include "common.h"
#include "../../include/imgcomp.h"

namespace {

constexpr int CX_THREADS = 256;   // four waves: four units of one tile
constexpr int CX_TAPS = 12;
constexpr int CX_U = 2;           // channel groups (of 8) of one stage: 8 MFMAs
constexpr int CX_D = 6;           // stages in flight; divides CX_TAPS, so every unit's stage count is a multiple of it
constexpr float CX_LIM = IC_CKBD_LOG_SCALE_LIMIT;

// live tap t = 0 .. 11 in ascending (ky, kx) order: ky + kx odd means 5 ky + kx odd, so it is element 2 t + 1 of the
// 5 x 5 window (arithmetic, not a table: a table lookup is a memory load the MFMA loop would have to wait for)
__host__ __device__ __forceinline__ int tap_ky(int t) { return (2 * t + 1) / 5; }
__host__ __device__ __forceinline__ int tap_kx(int t) { return (2 * t + 1) % 5; }

struct CxGeo {
  long long H, W, C;
  long long cnt0, cnt1;     // anchors / non-anchors of one map
  int KG, NT, UB;           // channel groups of 8, output tiles of 32, blocks per tile
  int vec;                  // 16-byte input loads: C % 4 == 0 and aligned bases
};

// position i * W + j of entry q of the half of parity `par` of one map (ckbd.hip full_unit's rule)
__device__ __forceinline__ long long half_position(long long q, int par, long long W) {
  const long long first = (W - par + 1) / 2;
  const long long pair = q / W, rem = q - pair * W;
  const bool odd = rem >= first;
  const long long i = 2 * pair + (odd ? 1 : 0);
  const long long j = odd ? (1 - par) + 2 * (rem - first) : par + 2 * rem;
  return i * W + j;
}

__device__ __forceinline__ float clamp_log_scale(float b) { return b < -CX_LIM ? -CX_LIM : (b > CX_LIM ? CX_LIM : b); }

// packed[head][t][kg][o][e] = W_head[o][8 kg + e][ky_t][kx_t], 0 where o >= C or 8 kg + e >= C
__global__ void __launch_bounds__(CX_THREADS) pack_k(const float* __restrict__ w_mean, const float* __restrict__ w_scale,
                                                     long long C, long long KG, long long OP, long long total,
                                                     float* __restrict__ packed) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int e = (int)(idx & 7);
    long long rest = idx >> 3;
    const long long o = rest % OP;
    rest /= OP;
    const long long kg = rest % KG;
    rest /= KG;
    const int t = (int)(rest % CX_TAPS);
    const int head = (int)(rest / CX_TAPS);
    const long long c = 8 * kg + e;
    float v = 0.0f;
    if (o < C && c < C) v = (head ? w_scale : w_mean)[(o * C + c) * 25 + 2 * t + 1];
    packed[idx] = v;
  }
}

struct CxFrag {
  floatx4v y[CX_U], m[CX_U], b[CX_U];
};

// One unit of one image: the 32 x 32 accumulator of (tile, head, 32 output channels) over all of K.
// K is walked in stages of CX_U channel groups of one tap (4 CX_U MFMAs); the loads of CX_D stages are in flight
// while one is consumed, so a stage's inputs have CX_D - 1 stages of MFMAs to arrive in (the packed weights are too
// large to stay in L2 beside the activations: a stage loaded only one ahead waits for the memory side every time).
// Every load is unconditional and in bounds -- a neighbour outside the map, a channel group past the last and the
// stages past the end read a valid address whose value is dropped by a select where it is used -- so the loads
// of a stage are one straight run the wait counters can count.
// Where a stream of stages stands: tap t, stage kb of the tap, and for this lane's row whether the tap's neighbour
// lies inside the map and the element offset to read it at (the row's own position when it does not: a valid address
// whose value is dropped).  The per-lane 64-bit arithmetic runs once per tap; a stage costs a few scalar operations.
struct CxCursor {
  int t, kb;
  bool inb;
  long long at;
};

template <bool VEC, bool SCALE>
__device__ __forceinline__ floatx16 unit_gemm(const float* __restrict__ yn, const float* __restrict__ mn,
                                              const float* __restrict__ wp, const CxGeo& geo, long long pos1, int g,
                                              int steps, int KB, float bias) {
  const long long H = geo.H, W = geo.W;
  const int C = (int)geo.C, KG = geo.KG;
  const int OP8 = 32 * geo.NT * 8;   // floats of one (tap, channel group) of the pack: below 2^31 in all (C <= 4096)
  const long long pi = pos1 >= 0 ? pos1 / W : 0, pj = pos1 >= 0 ? pos1 - pi * W : 0;
  const long long own = pos1 >= 0 ? pos1 * geo.C : 0;
  const float* __restrict__ wg = wp + 4 * g;
  const int cg = 4 * g;

  auto enter = [&](CxCursor& c, int t) {
    c.t = t;
    c.kb = 0;
    const long long ni = pi + tap_ky(t) - 2, nj = pj + tap_kx(t) - 2;
    c.inb = pos1 >= 0 && ni >= 0 && ni < H && nj >= 0 && nj < W;
    c.at = c.inb ? (ni * W + nj) * geo.C : own;
  };
  auto advance = [&](CxCursor& c) {   // past the last stage: stays there
    if (c.kb + 1 < KB)
      ++c.kb;
    else if (c.t + 1 < CX_TAPS)
      enter(c, c.t + 1);
  };
  auto load = [&](const CxCursor& c, CxFrag& f) {
    const float* __restrict__ yp = yn + c.at;
    const float* __restrict__ mp = mn + c.at;
#pragma unroll
    for (int u = 0; u < CX_U; ++u) {
      const int kg = min(c.kb * CX_U + u, KG - 1);
      const int c0 = 8 * kg + cg;
      if constexpr (VEC) {   // C % 4 == 0: four channels exist together; past C the last four, dropped at use
        const int ch = c0 < C ? c0 : C - 4;
        f.y[u] = *reinterpret_cast<const floatx4v*>(yp + ch);
        if constexpr (SCALE) f.m[u] = *reinterpret_cast<const floatx4v*>(mp + ch);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int ch = c0 + k < C ? c0 + k : C - 1;
          f.y[u][k] = yp[ch];
          if constexpr (SCALE) f.m[u][k] = mp[ch];
        }
      }
      f.b[u] = *reinterpret_cast<const floatx4v*>(wg + (c.t * KG + kg) * OP8);
    }
  };

  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = bias;

  auto use = [&](const CxCursor& c, const CxFrag& f) {
#pragma unroll
    for (int u = 0; u < CX_U; ++u) {
      const int kg = c.kb * CX_U + u;
      const bool group = kg < KG;   // a group past the last one (KG not a multiple of CX_U) adds 0 * 0
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bool live = c.inb && group && 8 * kg + cg + s < C;
        float a = f.y[u][s];
        if constexpr (SCALE) a = fabsf(__fsub_rn(a, f.m[u][s]));
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(live ? a : 0.0f, group ? f.b[u][s] : 0.0f, acc, 0, 0, 0);
      }
    }
  };

  CxFrag buf[CX_D];
  CxCursor lc, uc;   // the stage being loaded runs CX_D ahead of the stage being used
  enter(lc, 0);
  enter(uc, 0);
#pragma unroll
  for (int d = 0; d < CX_D; ++d) {   // steps is a multiple of CX_TAPS, and CX_D divides CX_TAPS: at least CX_D stages
    load(lc, buf[d]);
    advance(lc);
  }
  for (int base = 0; base < steps; base += CX_D) {
#pragma unroll
    for (int d = 0; d < CX_D; ++d) {
      use(uc, buf[d]);
      advance(uc);
      load(lc, buf[d]);   // past the end: the last stage again, never used
      advance(lc);
    }
  }
  return acc;
}

template <bool VEC>
__global__ void __launch_bounds__(CX_THREADS) context_k(const float* __restrict__ y_in, const float* __restrict__ mu_h,
                                                        const float* __restrict__ sigma_h,
                                                        const float* __restrict__ packed,
                                                        const float* __restrict__ b_mean,
                                                        const float* __restrict__ b_scale, int N, CxGeo geo,
                                                        float* __restrict__ mu, float* __restrict__ sigma) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, g = lane >> 5;
  const long long tile = blockIdx.x / geo.UB;
  const int unit = (int)(blockIdx.x % geo.UB) * 4 + wave;
  if (unit >= 2 * geo.NT) return;   // no barrier below: a wave without a unit just leaves
  const int head = unit / geo.NT, nt = unit % geo.NT;
  const long long H = geo.H, W = geo.W, C = geo.C;
  const long long o = 32ll * nt + r;   // this lane's output channel: B's column, the accumulators' column

  // row r of the tile: non-anchor q (the GEMM's row) and anchor q (the copy's)
  const long long q = tile * 32 + r;
  const long long pos1 = q < geo.cnt1 ? half_position(q, 1, W) : -1;
  const long long pos0 = q < geo.cnt0 ? half_position(q, 0, W) : -1;

  const float bias = o < C ? (head ? b_scale : b_mean)[o] : 0.0f;
  const int KB = (geo.KG + CX_U - 1) / CX_U;
  const int steps = geo.cnt1 > 32 * tile ? CX_TAPS * KB : 0;   // a tile past the last non-anchor only copies
  // this head's packed taps, at this lane's output channel
  const float* __restrict__ wp = packed + (long long)head * CX_TAPS * geo.KG * (32ll * geo.NT * 8) + o * 8;

  for (long long n = blockIdx.y; n < N; n += gridDim.y) {
    const long long img = n * H * W * C;
    floatx16 acc;
    if (steps == 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[v] = bias;
    } else if (head) {
      acc = unit_gemm<VEC, true>(y_in + img, mu_h + img, wp, geo, pos1, g, steps, KB, bias);
    } else {
      acc = unit_gemm<VEC, false>(y_in + img, mu_h + img, wp, geo, pos1, g, steps, KB, bias);
    }

    const float* __restrict__ hin = (head ? sigma_h : mu_h) + img;
    float* __restrict__ out = (head ? sigma : mu) + img;
    // The hyperprior's values first, all 32 loads in flight (a row past the end or a padded column reads element 0
    // or channel C - 1, which exist, and stores nothing), then the stores.
    // Non-anchors: accumulator v of this lane is row (v & 3) + 8 (v >> 2) + 4 g of the tile, column o.
    // Anchors: rows g, g + 2, ... of the tile, column o.
    const long long oc = o < C ? o : C - 1;
    long long pn[16], pa[16];
    float hn[16], ha[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      pn[v] = __shfl(pos1, (v & 3) + 8 * (v >> 2) + 4 * g);
      pa[v] = __shfl(pos0, g + 2 * v);
      hn[v] = hin[(pn[v] >= 0 ? pn[v] : 0) * C + oc];
      ha[v] = hin[(pa[v] >= 0 ? pa[v] : 0) * C + oc];
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      if (pn[v] >= 0 && o < C)
        out[pn[v] * C + o] = head ? __fmul_rn(hn[v], expf(clamp_log_scale(acc[v]))) : __fadd_rn(hn[v], acc[v]);
      if (pa[v] >= 0 && o < C) out[pa[v] * C + o] = ha[v];
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// N H W C as one element count; 0: a size below 1 or a product past 2^63 - 1 (ckbd.hip's rule)
long long checked_count(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 1) return 0;
  const long long a = (long long)N * H, b = (long long)W * C;
  if (a > 0x7fffffffffffffffll / b) return 0;
  return a * b;
}

long long pack_floats(int C) {
  const long long KG = ((long long)C + 7) / 8, OP = ((long long)C + 31) / 32 * 32;
  return 2ll * CX_TAPS * KG * OP * 8;
}

}  // namespace

extern "C" {

size_t ic_context_ws(int C) {
  if (C < 1 || C > IC_CONTEXT_MAXC) return 0;
  return (size_t)pack_floats(C) * sizeof(float);
}

int ic_context_fwd(const float* y_in, const float* mu_h, const float* sigma_h, const float* w_mean,
                        const float* b_mean, const float* w_scale, const float* b_scale, int N, int H, int W, int C,
                        float* mu, float* sigma, void* ws, size_t ws_bytes, int packed, void* stream) {
  const long long n = checked_count(N, H, W, C);
  if (!y_in || !mu_h || !sigma_h || !w_mean || !b_mean || !w_scale || !b_scale || !mu || !sigma || !ws || n == 0)
    return IC_ERR_ARG;
  if (C > IC_CONTEXT_MAXC || mu == sigma) return IC_ERR_ARG;
  for (const float* in : {y_in, mu_h, sigma_h})
    if (in == mu || in == sigma) return IC_ERR_ARG;   // blocks read their neighbours' inputs while others write
  if (!aligned16(ws)) return IC_ERR_ARG;
  if (ws_bytes < ic_context_ws(C)) return IC_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;

  CxGeo geo;
  geo.H = H;
  geo.W = W;
  geo.C = C;
  const long long hw = (long long)H * W;
  geo.cnt0 = (hw + 1) / 2;
  geo.cnt1 = hw / 2;
  geo.KG = (C + 7) / 8;
  geo.NT = (C + 31) / 32;
  geo.UB = (2 * geo.NT + 3) / 4;
  geo.vec = C % 4 == 0 && aligned16(y_in) && aligned16(mu_h);
  const long long tiles = (geo.cnt0 + 31) / 32;   // >= 1; the anchors are never fewer than the non-anchors
  if (tiles > 0x7fffffffll / geo.UB) return IC_ERR_ARG;

  if (!packed && geo.cnt1 > 0) {   // a 1 x 1 map has no non-anchor: the copy alone
    const long long total = pack_floats(C);
    const int blocks = (int)std::min<long long>((total + CX_THREADS - 1) / CX_THREADS, 4096);
    hipLaunchKernelGGL(pack_k, dim3(blocks), dim3(CX_THREADS), 0, st, w_mean, w_scale, (long long)C, (long long)geo.KG,
                       32ll * geo.NT, total, (float*)ws);
    IC_CHECK_LAUNCH();
  }
  const dim3 grid((unsigned)(tiles * geo.UB), (unsigned)std::min(N, 65535));
  if (geo.vec)
    hipLaunchKernelGGL(context_k<true>, grid, dim3(CX_THREADS), 0, st, y_in, mu_h, sigma_h, (const float*)ws, b_mean,
                       b_scale, N, geo, mu, sigma);
  else
    hipLaunchKernelGGL(context_k<false>, grid, dim3(CX_THREADS), 0, st, y_in, mu_h, sigma_h, (const float*)ws, b_mean,
                       b_scale, N, geo, mu, sigma);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
