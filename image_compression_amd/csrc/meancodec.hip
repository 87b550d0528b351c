// Mean-scale hyperprior: the elementwise ops that code y about a mean mu = h_s(z_hat) (ic_codec_symbolize_mean*,
// ic_center_round, ic_add_mean).  The symbols are rint(y - mu), the reconstruction is r + mu:
//   * d = y - mu is one fp32 subtraction and y_hat = r + mu one fp32 addition (neither has a product beside it to
//     be contracted with), so the encoder's eval forward and the decoder, which holds the same r (the integers it
//     decoded, as floats) and the same mu bits, form the same y_hat bits;
//   * the symbolizers are seg_symbolize.h's walk and driver over d.
// y and mu are dense channels-last storage of the same length in the same order.  All kernels are grid-stride
// and HBM-bound: 16-byte accesses when every pointer is 16-byte aligned (and, with segments, every segment
// start is), then a scalar tail of n % 4 elements; scalar throughout otherwise.
#include "seg_symbolize.h"

namespace {

struct MeanSrc {
  const float *y, *mu;
  __device__ __forceinline__ void bind(unsigned seg, long long len, long long, long long) {
    y += (long long)seg * len;
    mu += (long long)seg * len;
  }
  template <class V>
  __device__ __forceinline__ V at(long long i) const {
    return sub_rn(load_as<V>(y, i), load_as<V>(mu, i));
  }
  __device__ __forceinline__ void next() {}
};

// rint(y - mu) as the float the decoder will hold: (float)(int) is never -0.0, so a residual that rounds to -0.0
// becomes +0.0 here (x + 0.0f is x but for that), and r + mu has the same bits on both sides even where mu is -0.0
__device__ __forceinline__ float residual_of(float y, float mu) { return __fadd_rn(rintf(__fsub_rn(y, mu)), 0.0f); }

// r = rint(y - mu) as float, y_hat = r + mu
template <bool VEC>
__global__ void __launch_bounds__(SEG_THREADS) center_round_k(const float* __restrict__ y, const float* __restrict__ mu,
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
__global__ void __launch_bounds__(SEG_THREADS) add_mean_k(const float* __restrict__ r, const float* __restrict__ mu,
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

// ---- the host checks, before any launch (ic_codec_symbolize_seg's limits on the segments)
bool symbolize_args_ok(const float* y, const float* mu, int nseg, long long seg_len, const int* sym, const int* kmax_dev,
                       const int* kmax_host) {
  if (!y || !mu || !sym || !kmax_dev || !kmax_host) return false;
  return nseg >= 1 && nseg <= 65535 && seg_len >= 1 && seg_len <= 0x7fffffffffffffffll / nseg;
}

int symbolize_mean(const float* y, const float* mu, int nseg, long long seg_len, int* sym, int* kmax_dev, int* kmax_host,
                   void* stream) {
  // a segment starts at s * seg_len elements: 16-byte aligned for every s only when seg_len % 4 == 0
  const bool vec = aligned16(y) && aligned16(mu) && aligned16(sym) && (nseg == 1 || seg_len % 4 == 0);
  return seg_symbolize(MeanSrc{y, mu}, vec, nseg, seg_len, nullptr, nullptr, sym, kmax_dev, kmax_host,
                       (hipStream_t)stream);
}

}  // namespace

extern "C" {

int ic_codec_symbolize_mean(const float* y, const float* mu, long long n, int* sym, int* kmax_dev, int* kmax_host,
                            void* stream) {
  if (!symbolize_args_ok(y, mu, 1, n, sym, kmax_dev, kmax_host)) return IC_ERR_ARG;
  return symbolize_mean(y, mu, 1, n, sym, kmax_dev, kmax_host, stream);
}

int ic_codec_symbolize_mean_seg(const float* y, const float* mu, int nseg, long long seg_len, int* sym, int* kmax_dev,
                                int* kmax_host, void* stream) {
  if (!symbolize_args_ok(y, mu, nseg, seg_len, sym, kmax_dev, kmax_host)) return IC_ERR_ARG;
  return symbolize_mean(y, mu, nseg, seg_len, sym, kmax_dev, kmax_host, stream);
}

int ic_center_round(const float* y, const float* mu, long long n, float* r, float* y_hat, void* stream) {
  if (!y || !mu || !r || !y_hat || r == y_hat || n < 1) return IC_ERR_ARG;
  const bool vec = aligned16(y) && aligned16(mu) && aligned16(r) && aligned16(y_hat);
  const dim3 grid(seg_blocks(n, vec));
  if (vec)
    hipLaunchKernelGGL(center_round_k<true>, grid, dim3(SEG_THREADS), 0, (hipStream_t)stream, y, mu, n, r, y_hat);
  else
    hipLaunchKernelGGL(center_round_k<false>, grid, dim3(SEG_THREADS), 0, (hipStream_t)stream, y, mu, n, r, y_hat);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_add_mean(const float* r, const float* mu, long long n, float* y_hat, void* stream) {
  if (!r || !mu || !y_hat || n < 1) return IC_ERR_ARG;
  const bool vec = aligned16(r) && aligned16(mu) && aligned16(y_hat);
  const dim3 grid(seg_blocks(n, vec));
  if (vec)
    hipLaunchKernelGGL(add_mean_k<true>, grid, dim3(SEG_THREADS), 0, (hipStream_t)stream, r, mu, n, y_hat);
  else
    hipLaunchKernelGGL(add_mean_k<false>, grid, dim3(SEG_THREADS), 0, (hipStream_t)stream, r, mu, n, y_hat);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
