// Encode-time latent refinement (Campos et al. 2019; Yang, Bamler and Mandt 2020): the device-side bookkeeping of the
// loop that moves the coded latent v of every image by Adam steps on that image's own R + lambda D and keeps the best
// integers it saw (codec.py states the rule; Compressor2018.compress_each_refined runs it).  Nothing here copies to
// the host or waits for a stream: the loop enqueues whole.
//
//   * ic_refine_update: one pass over the latent.  With a gradient g, the Adam step on v (moments m, u) in exactly
//     this fp32 operation order, every operation rounded once and none contracted with another:
//         m' = 0.9f * m + 0.1f * g                     (two products, one sum)
//         u' = 0.999f * u + 0.001f * (g * g)           (g * g first, then two products, one sum)
//         v' = v - (lr * (m' * c1)) / (sqrtf(u' * c2) + 1e-8f)
//     c1 = 1 / (1 - 0.9^t) and c2 = 1 / (1 - 0.999^t) are formed by the caller in double and passed as fp32.  Then,
//     with or without a step, the Evaluate rule on the (new) v:
//         sym = symbol_of(v' - mu)     (codec_sym.h; one fp32 subtraction: ic_codec_symbolize_mean_seg's symbols)
//         y_hat = (float)sym + mu      (one fp32 addition: ic_add_mean's reconstruction)
//     without mu neither the subtraction nor the addition is performed.  The arithmetic is written with plain
//     operators, sqrtf and / under `fp contract(off)`: in this toolchain's headers __fmul_rn / __fadd_rn / __fsub_rn /
//     __fdiv_rn are those same operators (which the default contraction mode may fuse) and __fsqrt_rn is the
//     hardware's approximate square root; the operators here are IEEE round-to-nearest each (the build has no
//     fast-math flag), so a numpy float32 restatement has the same bits.
//   * ic_refine_dist_grad: the gradient of sum_n w_n D_n at x_hat: gx = (float)(2 w_n) * (x_hat - x).
//   * ic_refine_objective: B_n, D_n and J_n = B_n + w_n D_n in fp64 from the per-block maps of ic_block_bits and
//     ic_block_sse, one thread per image over its blocks in ascending order: one fixed order, bitwise repeatable.
//   * ic_refine_keep: mode 0, grid (blocks, images): every block reads J[n] and best J[n] and copies image n's symbols
//     into the kept ones when J[n] < best[n] (strict; a NaN never wins); mode 1, a second tiny launch: best (B, D, J)
//     and best_step of the winners.  No block reads what another writes in the same launch.
//   * ic_refine_kmax: max |symbol| per image, one integer atomicMax per block.  No floating-point atomics anywhere.
// v, m, u, g, mu, sym and y_hat are dense channels-last storage (N, P, C).  Grid-stride and HBM-bound, as gain.hip and
// budget.hip: 16-byte accesses when every pointer is 16-byte aligned and C % 4 == 0, scalar accesses with the same
// arithmetic otherwise.  Every argument is checked on the host before any launch.
#include <algorithm>
#include <limits.h>

#include "common.h"
#include "codec_sym.h"
#include "../../include/imgcomp.h"

#pragma clang fp contract(off)

namespace {

typedef int intx4v __attribute__((ext_vector_type(4)));

constexpr int RF_THREADS = 256;
constexpr int RF_MAXBLOCKS = 1024;
constexpr int RF_BATCH = 16;   // map values an objective thread loads before it adds them (latency, as gain.hip)

struct Adam {
  float lr, c1, c2;
};

// one element of ic_refine_update; STEP: the Adam step in front of the Evaluate rule
template <bool STEP, bool MEAN>
__device__ __forceinline__ void update_one(float& v, float& m, float& u, float g, float mu, const Adam a, int& sym,
                                           float& y_hat) {
  if (STEP) {
    const float m1 = 0.9f * m;
    const float m2 = 0.1f * g;
    m = m1 + m2;
    const float gg = g * g;
    const float u1 = 0.999f * u;
    const float u2 = 0.001f * gg;
    u = u1 + u2;
    const float mh = m * a.c1;
    const float uh = u * a.c2;
    const float num = a.lr * mh;
    const float den = sqrtf(uh) + 1e-8f;
    const float q = num / den;
    v = v - q;
  }
  if (MEAN) {
    sym = symbol_of(v - mu);
    y_hat = (float)sym + mu;
  } else {
    sym = symbol_of(v);
    y_hat = (float)sym;
  }
}

template <bool VEC, bool STEP, bool MEAN>
__global__ void __launch_bounds__(RF_THREADS) refine_update_k(float* __restrict__ v, float* __restrict__ m,
                                                              float* __restrict__ u, const float* __restrict__ g,
                                                              const float* __restrict__ mu, long long n, Adam a,
                                                              int* __restrict__ sym, float* __restrict__ y_hat) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  if (VEC) {
    const long long n4 = n / 4;   // C % 4 == 0, so n % 4 == 0
    for (long long i = tid; i < n4; i += stride) {
      floatx4v vv = reinterpret_cast<floatx4v*>(v)[i];
      floatx4v mm = {0.f, 0.f, 0.f, 0.f}, uu = mm, gg = mm, cc = mm, yy;
      if (STEP) {
        mm = reinterpret_cast<floatx4v*>(m)[i];
        uu = reinterpret_cast<floatx4v*>(u)[i];
        gg = reinterpret_cast<const floatx4v*>(g)[i];
      }
      if (MEAN) cc = reinterpret_cast<const floatx4v*>(mu)[i];
      intx4v ss;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float vj = vv[j], mj = mm[j], uj = uu[j], yj;
        int sj;
        update_one<STEP, MEAN>(vj, mj, uj, gg[j], cc[j], a, sj, yj);
        vv[j] = vj; mm[j] = mj; uu[j] = uj; ss[j] = sj; yy[j] = yj;
      }
      if (STEP) {
        reinterpret_cast<floatx4v*>(v)[i] = vv;
        reinterpret_cast<floatx4v*>(m)[i] = mm;
        reinterpret_cast<floatx4v*>(u)[i] = uu;
      }
      reinterpret_cast<intx4v*>(sym)[i] = ss;
      reinterpret_cast<floatx4v*>(y_hat)[i] = yy;
    }
  } else {
    for (long long i = tid; i < n; i += stride) {
      float vj = v[i], mj = STEP ? m[i] : 0.f, uj = STEP ? u[i] : 0.f, yj;
      int sj;
      update_one<STEP, MEAN>(vj, mj, uj, STEP ? g[i] : 0.f, MEAN ? mu[i] : 0.f, a, sj, yj);
      if (STEP) {
        v[i] = vj;
        m[i] = mj;
        u[i] = uj;
      }
      sym[i] = sj;
      y_hat[i] = yj;
    }
  }
}

// blockIdx.y = image; gx = (float)(2 w[image]) * (x_hat - x) over the image's `len` elements
template <bool VEC>
__global__ void __launch_bounds__(RF_THREADS) refine_dist_grad_k(const float* __restrict__ x,
                                                                 const float* __restrict__ x_hat,
                                                                 const double* __restrict__ w, long long len,
                                                                 float* __restrict__ gx) {
  const long long base = (long long)blockIdx.y * len;
  const float s = (float)(2.0 * w[blockIdx.y]);
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  if (VEC) {
    const floatx4v* a = reinterpret_cast<const floatx4v*>(x + base);
    const floatx4v* b = reinterpret_cast<const floatx4v*>(x_hat + base);
    floatx4v* o = reinterpret_cast<floatx4v*>(gx + base);
    for (long long i = tid; i < len / 4; i += stride) {
      const floatx4v av = a[i], bv = b[i];
      floatx4v ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = bv[j] - av[j];
        ov[j] = s * d;
      }
      o[i] = ov;
    }
  } else {
    for (long long i = tid; i < len; i += stride) {
      const float d = x_hat[base + i] - x[base + i];
      gx[base + i] = s * d;
    }
  }
}

// one thread per image: out[0][n] = B_n, out[1][n] = D_n, out[2][n] = J_n, the maps' nb blocks in ascending order
__global__ void __launch_bounds__(RF_THREADS) refine_objective_k(const float* __restrict__ bits,
                                                                 const float* __restrict__ sse,
                                                                 const double* __restrict__ w, int N, long long nb,
                                                                 double* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* bp = bits + (long long)n * nb;
  const float* sp = sse + (long long)n * nb;
  double B = 0.0, D = 0.0;
  for (long long b0 = 0; b0 < nb; b0 += RF_BATCH) {
    float vb[RF_BATCH], vs[RF_BATCH];
#pragma unroll
    for (int k = 0; k < RF_BATCH; ++k) {
      vb[k] = b0 + k < nb ? bp[b0 + k] : 0.0f;
      vs[k] = b0 + k < nb ? sp[b0 + k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < RF_BATCH; ++k)
      if (b0 + k < nb) {   // the map's own values alone, in ascending order
        B = B + (double)vb[k];
        D = D + (double)vs[k];
      }
  }
  const double wd = w[n] * D;
  out[n] = B;
  out[(long long)N + n] = D;
  out[2ll * N + n] = B + wd;
}

// blockIdx.y = image: its `len` symbols into the kept ones when J[n] < best J[n]
template <bool VEC>
__global__ void __launch_bounds__(RF_THREADS) refine_keep_copy_k(const int* __restrict__ sym, int* __restrict__ best_sym,
                                                                 const double* __restrict__ obj,
                                                                 const double* __restrict__ best, int N, long long len) {
  const int n = blockIdx.y;
  if (!(obj[2ll * N + n] < best[2ll * N + n])) return;   // the same answer in every thread of the image's blocks
  const long long base = (long long)n * len;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  if (VEC) {
    const intx4v* s = reinterpret_cast<const intx4v*>(sym + base);
    intx4v* d = reinterpret_cast<intx4v*>(best_sym + base);
    for (long long i = tid; i < len / 4; i += stride) d[i] = s[i];
  } else {
    for (long long i = tid; i < len; i += stride) best_sym[base + i] = sym[base + i];
  }
}

// one thread per image: the winner's (B, D, J) and step
__global__ void __launch_bounds__(RF_THREADS) refine_keep_best_k(const double* __restrict__ obj, double* __restrict__ best,
                                                                 int* __restrict__ best_step, int step, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  if (!(obj[2ll * N + n] < best[2ll * N + n])) return;
  best[n] = obj[n];
  best[(long long)N + n] = obj[(long long)N + n];
  best[2ll * N + n] = obj[2ll * N + n];
  best_step[n] = step;
}

// blockIdx.y = image; kmax[image] = max |symbol| (INT_MAX for INT_MIN)
__global__ void __launch_bounds__(RF_THREADS) refine_kmax_k(const int* __restrict__ sym, long long len,
                                                            int* __restrict__ kmax) {
  const int* s = sym + (long long)blockIdx.y * len;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  int m = 0;
  for (long long i = tid; i < len; i += stride) {
    const int k = s[i];
    m = max(m, k == INT_MIN ? INT_MAX : (k < 0 ? -k : k));
  }
  m = block_max(m);
  if (threadIdx.x == 0) atomicMax(kmax + blockIdx.y, m);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool shape_ok(long long N, long long P, int C) {
  if (N < 1 || N > 65535 || P < 1 || C < 1) return false;
  return P <= 0x7fffffffffffffffll / C / N;
}

unsigned blocks_for(long long work) {
  return (unsigned)std::max<long long>(1, std::min<long long>((work + RF_THREADS - 1) / RF_THREADS, RF_MAXBLOCKS));
}

template <bool VEC, bool STEP>
void launch_update(hipStream_t st, unsigned grid, float* v, float* m, float* u, const float* g, const float* mu,
                   long long n, Adam a, int* sym, float* y_hat) {
  if (mu)
    hipLaunchKernelGGL((refine_update_k<VEC, STEP, true>), dim3(grid), dim3(RF_THREADS), 0, st, v, m, u, g, mu, n, a, sym,
                       y_hat);
  else
    hipLaunchKernelGGL((refine_update_k<VEC, STEP, false>), dim3(grid), dim3(RF_THREADS), 0, st, v, m, u, g, mu, n, a, sym,
                       y_hat);
}

}  // namespace

extern "C" {

int ic_refine_update(float* v, float* m, float* u, const float* g, const float* mu, long long N, long long P, int C,
                     float lr, float c1, float c2, int* sym, float* y_hat, void* stream) {
  if (!v || !sym || !y_hat || !shape_ok(N, P, C)) return IC_ERR_ARG;
  if (g && (!m || !u)) return IC_ERR_ARG;
  if (g && !(lr > 0.0f && lr < INFINITY && c1 >= 1.0f && c1 < INFINITY && c2 >= 1.0f && c2 < INFINITY))
    return IC_ERR_ARG;   // NaN fails every comparison
  const long long n = N * P * C;
  bool vec = C % 4 == 0 && aligned16(v) && aligned16(sym) && aligned16(y_hat) && (!mu || aligned16(mu));
  if (g) vec = vec && aligned16(m) && aligned16(u) && aligned16(g);
  const unsigned grid = blocks_for(n / (vec ? 4 : 1));
  const Adam a = {lr, c1, c2};
  hipStream_t st = (hipStream_t)stream;
  if (g) {
    if (vec) launch_update<true, true>(st, grid, v, m, u, g, mu, n, a, sym, y_hat);
    else launch_update<false, true>(st, grid, v, m, u, g, mu, n, a, sym, y_hat);
  } else {
    if (vec) launch_update<true, false>(st, grid, v, m, u, g, mu, n, a, sym, y_hat);
    else launch_update<false, false>(st, grid, v, m, u, g, mu, n, a, sym, y_hat);
  }
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_refine_dist_grad(const float* x, const float* x_hat, const double* w, int N, long long len, float* gx,
                        void* stream) {
  if (!x || !x_hat || !w || !gx || N < 1 || N > 65535 || len < 1 || len > 0x7fffffffffffffffll / N) return IC_ERR_ARG;
  const bool vec = len % 4 == 0 && aligned16(x) && aligned16(x_hat) && aligned16(gx);
  const dim3 grid(blocks_for(len / (vec ? 4 : 1)), (unsigned)N);
  if (vec)
    hipLaunchKernelGGL(refine_dist_grad_k<true>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, x, x_hat, w, len, gx);
  else
    hipLaunchKernelGGL(refine_dist_grad_k<false>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, x, x_hat, w, len, gx);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_refine_objective(const float* bits, const float* sse, const double* w, int N, long long nb, double* out,
                        void* stream) {
  if (!bits || !sse || !w || !out || N < 1 || N > 65535 || nb < 1 || nb > 0x7fffffffffffffffll / N) return IC_ERR_ARG;
  hipLaunchKernelGGL(refine_objective_k, dim3(ic_cdiv(N, RF_THREADS)), dim3(RF_THREADS), 0, (hipStream_t)stream, bits,
                     sse, w, N, nb, out);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_refine_keep(const int* sym, int* best_sym, const double* obj, double* best, int* best_step, int step, int N,
                   long long len, int mode, void* stream) {
  if (!obj || !best || N < 1 || N > 65535 || (mode != 0 && mode != 1)) return IC_ERR_ARG;
  if (mode == 0) {
    if (!sym || !best_sym || sym == best_sym || len < 1 || len > 0x7fffffffffffffffll / N) return IC_ERR_ARG;
    const bool vec = len % 4 == 0 && aligned16(sym) && aligned16(best_sym);
    const dim3 grid(blocks_for(len / (vec ? 4 : 1)), (unsigned)N);
    if (vec)
      hipLaunchKernelGGL(refine_keep_copy_k<true>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, sym, best_sym, obj,
                         best, N, len);
    else
      hipLaunchKernelGGL(refine_keep_copy_k<false>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, sym, best_sym, obj,
                         best, N, len);
  } else {
    if (!best_step || step < 0) return IC_ERR_ARG;
    hipLaunchKernelGGL(refine_keep_best_k, dim3(ic_cdiv(N, RF_THREADS)), dim3(RF_THREADS), 0, (hipStream_t)stream, obj,
                       best, best_step, step, N);
  }
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_refine_kmax(const int* sym, int N, long long len, int* kmax, void* stream) {
  if (!sym || !kmax || N < 1 || N > 65535 || len < 1 || len > 0x7fffffffffffffffll / N) return IC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(kmax, 0, sizeof(int) * N, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(refine_kmax_k, dim3(blocks_for(len), (unsigned)N), dim3(RF_THREADS), 0, st, sym, len, kmax);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
