// Mean-scale hyperprior: the elementwise ops that code y about a mean mu = h_s(z_hat) (ic_codec_symbolize_mean*,
// ic_center_round, ic_add_mean).  The symbols are rint(y - mu), the reconstruction is r + mu:
//   * d = y - mu is one fp32 subtraction and y_hat = r + mu one fp32 addition (__fsub_rn / __fadd_rn: never
//     contracted with anything), so the encoder's eval forward and the decoder, which holds the same r (the
//     integers it decoded, as floats) and the same mu bits, form the same y_hat bits;
//   * the symbol of d is codec.hip's rule (codec_sym.h), the maximum one integer atomicMax per block:
//     order-independent, deterministic.  No floating-point atomics.
// y and mu are dense channels-last storage of the same length in the same order.  All kernels are grid-stride
// and HBM-bound: 16-byte accesses when every pointer is 16-byte aligned (and, with segments, every segment
// start is), then a scalar tail of n % 4 elements; scalar throughout otherwise.
#include <algorithm>

#include "common.h"
#include "codec_sym.h"
#include "../../include/imgcomp.h"

namespace {

typedef int intx4v __attribute__((ext_vector_type(4)));

constexpr int MC_THREADS = 256;
constexpr int MC_MAXBLOCKS = 1024;

// blockIdx.y = segment; kmax[segment] = its max |symbol|
template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) mean_symbolize_k(const float* __restrict__ y, const float* __restrict__ mu,
                                                               long long seg_len, int* __restrict__ sym,
                                                               int* __restrict__ kmax) {
  const long long base = (long long)blockIdx.y * seg_len;
  const float* ys = y + base;
  const float* ms = mu + base;
  int* ss = sym + base;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  int m = 0;
  long long done = 0;
  if (VEC) {
    const long long n4 = seg_len >> 2;
    for (long long i = tid; i < n4; i += stride) {
      const floatx4v a = reinterpret_cast<const floatx4v*>(ys)[i];
      const floatx4v b = reinterpret_cast<const floatx4v*>(ms)[i];
      intx4v k;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        k[j] = symbol_of(__fsub_rn(a[j], b[j]));
        m = max(m, k[j] < 0 ? -k[j] : k[j]);
      }
      reinterpret_cast<intx4v*>(ss)[i] = k;
    }
    done = n4 << 2;
  }
  for (long long i = done + tid; i < seg_len; i += stride) {
    const int k = symbol_of(__fsub_rn(ys[i], ms[i]));
    ss[i] = k;
    m = max(m, k < 0 ? -k : k);
  }
  m = block_max(m);
  if (threadIdx.x == 0) atomicMax(kmax + blockIdx.y, m);
}

// rint(y - mu) as the float the decoder will hold: (float)(int) is never -0.0, so a residual that rounds to -0.0
// becomes +0.0 here (x + 0.0f is x but for that), and r + mu has the same bits on both sides even where mu is -0.0
__device__ __forceinline__ float residual_of(float y, float mu) { return __fadd_rn(rintf(__fsub_rn(y, mu)), 0.0f); }

// r = rint(y - mu) as float, y_hat = r + mu
template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) center_round_k(const float* __restrict__ y, const float* __restrict__ mu,
                                                             long long n, float* __restrict__ r,
                                                             float* __restrict__ y_hat) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long done = 0;
  if (VEC) {
    const long long n4 = n >> 2;
    for (long long i = tid; i < n4; i += stride) {
      const floatx4v a = reinterpret_cast<const floatx4v*>(y)[i];
      const floatx4v b = reinterpret_cast<const floatx4v*>(mu)[i];
      floatx4v q, h;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        q[j] = residual_of(a[j], b[j]);
        h[j] = __fadd_rn(q[j], b[j]);
      }
      reinterpret_cast<floatx4v*>(r)[i] = q;
      reinterpret_cast<floatx4v*>(y_hat)[i] = h;
    }
    done = n4 << 2;
  }
  for (long long i = done + tid; i < n; i += stride) {
    const float b = mu[i];
    const float q = residual_of(y[i], b);
    r[i] = q;
    y_hat[i] = __fadd_rn(q, b);
  }
}

// y_hat = r + mu: the addition of center_round_k on the same operands
template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) add_mean_k(const float* __restrict__ r, const float* __restrict__ mu,
                                                         long long n, float* __restrict__ y_hat) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long done = 0;
  if (VEC) {
    const long long n4 = n >> 2;
    for (long long i = tid; i < n4; i += stride) {
      const floatx4v a = reinterpret_cast<const floatx4v*>(r)[i];
      const floatx4v b = reinterpret_cast<const floatx4v*>(mu)[i];
      floatx4v h;
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = __fadd_rn(a[j], b[j]);
      reinterpret_cast<floatx4v*>(y_hat)[i] = h;
    }
    done = n4 << 2;
  }
  for (long long i = done + tid; i < n; i += stride) y_hat[i] = __fadd_rn(r[i], mu[i]);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// blocks of MC_THREADS threads for n elements, four per thread on the vector path
int blocks_for(long long n, bool vec) {
  const long long work = vec ? (n + 3) / 4 : n;
  return (int)std::min<long long>((work + MC_THREADS - 1) / MC_THREADS, MC_MAXBLOCKS);
}

// ---- the host checks, before any launch (ic_codec_symbolize_seg's limits on the segments)
bool symbolize_args_ok(const float* y, const float* mu, int nseg, long long seg_len, const int* sym, const int* kmax_dev,
                       const int* kmax_host) {
  if (!y || !mu || !sym || !kmax_dev || !kmax_host) return false;
  return nseg >= 1 && nseg <= 65535 && seg_len >= 1 && seg_len <= 0x7fffffffffffffffll / nseg;
}

int symbolize_mean(const float* y, const float* mu, int nseg, long long seg_len, int* sym, int* kmax_dev, int* kmax_host,
                   hipStream_t st) {
  hipError_t e = hipMemsetAsync(kmax_dev, 0, sizeof(int) * nseg, st);
  if (e != hipSuccess) return (int)e;
  // a segment starts at s * seg_len elements: 16-byte aligned for every s only when seg_len % 4 == 0
  const bool vec = aligned16(y) && aligned16(mu) && aligned16(sym) && (nseg == 1 || seg_len % 4 == 0);
  const dim3 grid(blocks_for(seg_len, vec), nseg);
  if (vec)
    hipLaunchKernelGGL(mean_symbolize_k<true>, grid, dim3(MC_THREADS), 0, st, y, mu, seg_len, sym, kmax_dev);
  else
    hipLaunchKernelGGL(mean_symbolize_k<false>, grid, dim3(MC_THREADS), 0, st, y, mu, seg_len, sym, kmax_dev);
  IC_CHECK_LAUNCH();
  e = hipMemcpyAsync(kmax_host, kmax_dev, sizeof(int) * nseg, hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return (int)e;
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  for (int s = 0; s < nseg; ++s)
    if (kmax_host[s] > IC_CODEC_KMAX) return IC_ERR_ARG;
  return IC_OK;
}

}  // namespace

extern "C" {

int ic_codec_symbolize_mean(const float* y, const float* mu, long long n, int* sym, int* kmax_dev, int* kmax_host,
                            void* stream) {
  if (!symbolize_args_ok(y, mu, 1, n, sym, kmax_dev, kmax_host)) return IC_ERR_ARG;
  return symbolize_mean(y, mu, 1, n, sym, kmax_dev, kmax_host, (hipStream_t)stream);
}

int ic_codec_symbolize_mean_seg(const float* y, const float* mu, int nseg, long long seg_len, int* sym, int* kmax_dev,
                                int* kmax_host, void* stream) {
  if (!symbolize_args_ok(y, mu, nseg, seg_len, sym, kmax_dev, kmax_host)) return IC_ERR_ARG;
  return symbolize_mean(y, mu, nseg, seg_len, sym, kmax_dev, kmax_host, (hipStream_t)stream);
}

int ic_center_round(const float* y, const float* mu, long long n, float* r, float* y_hat, void* stream) {
  if (!y || !mu || !r || !y_hat || r == y_hat || n < 1) return IC_ERR_ARG;
  const bool vec = aligned16(y) && aligned16(mu) && aligned16(r) && aligned16(y_hat);
  const dim3 grid(blocks_for(n, vec));
  if (vec)
    hipLaunchKernelGGL(center_round_k<true>, grid, dim3(MC_THREADS), 0, (hipStream_t)stream, y, mu, n, r, y_hat);
  else
    hipLaunchKernelGGL(center_round_k<false>, grid, dim3(MC_THREADS), 0, (hipStream_t)stream, y, mu, n, r, y_hat);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_add_mean(const float* r, const float* mu, long long n, float* y_hat, void* stream) {
  if (!r || !mu || !y_hat || n < 1) return IC_ERR_ARG;
  const bool vec = aligned16(r) && aligned16(mu) && aligned16(y_hat);
  const dim3 grid(blocks_for(n, vec));
  if (vec)
    hipLaunchKernelGGL(add_mean_k<true>, grid, dim3(MC_THREADS), 0, (hipStream_t)stream, r, mu, n, y_hat);
  else
    hipLaunchKernelGGL(add_mean_k<false>, grid, dim3(MC_THREADS), 0, (hipStream_t)stream, r, mu, n, y_hat);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
