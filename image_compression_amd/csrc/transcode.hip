// Transcoding in the latent domain: the symbols of y at M target qualities from the decoded integers of N source
// streams, in one launch (ic_requant_seg).  Target m names its source img[m]; r and mu1 are the source's decoded
// float integers and its mean, a[img[m]] the source's inverse gains, b[m] the target's gains, mu2[m] the target's
// mean; mu2 and sym are segments of P * C elements back to back:
//     sym[m][i] = symbol_of(fsub(fmul(fmul(fadd(r[img[m]][i], mu1[img[m]][i]), a[img[m]][c(i)]), b[m][c(i)]), mu2[m][i]))
//   * the sum is ic_add_mean's one fp32 addition, the two products ic_channel_scale's one fp32 multiplication
//     each, the difference ic_codec_symbolize_mean_seg's one fp32 subtraction, each rounded to nearest once and
//     none contracted with another, and the symbol is codec_sym.h's rule: bit for bit those four calls on the
//     gathered batch, without the gather copy and with neither y_hat nor the scaled latent in memory.  The arithmetic
//     is written with plain operators under `fp contract(off)`, as refine.hip: in this toolchain's headers
//     __fmul_rn / __fsub_rn are those operators compiled under the default contraction mode, which fuses the second
//     product with the difference into one FMA and so moves a difference that rounds to a tie at .5 to the other
//     integer (one symbol in 18432 on random gain tables);
//   * kmax[m] is one integer atomicMax per block: order-independent, deterministic.  No floating-point atomics.
// r, mu1, mu2 and sym are dense channels-last storage (P positions, channel fastest).  Grid-stride and HBM-bound, as
// budget.hip (20 bytes per symbol; the gain rows stay in cache): 16-byte accesses when every pointer is 16-byte
// aligned and C % 4 == 0 (then every segment and every gain row starts on a 16-byte boundary and a group of four
// never straddles a position), scalar accesses with the same arithmetic otherwise.
#include <algorithm>

#include "common.h"
#include "codec_sym.h"
#include "../../include/imgcomp.h"

#pragma clang fp contract(off)

namespace {

typedef int intx4v __attribute__((ext_vector_type(4)));

constexpr int RQ_THREADS = 256;
constexpr int RQ_MAXBLOCKS = 1024;

__device__ __forceinline__ int requant_of(float r, float m1, float a, float b, float m2) {
  // plain operators under `fp contract(off)`: IEEE round-to-nearest each, never fused (the header's __fmul_rn /
  // __fsub_rn carry the default contraction mode with them when they are inlined)
  const float y_hat = (r + m1) * a;
  const float scaled = y_hat * b;
  return symbol_of(scaled - m2);
}

// blockIdx.y = target; `len` = P * C elements per segment; kmax[target] = its max |symbol|
template <bool VEC>
__global__ void __launch_bounds__(RQ_THREADS) requant_k(const float* __restrict__ r, const float* __restrict__ mu1,
                                                        const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ mu2, const int* __restrict__ img,
                                                        long long len, int C, int* __restrict__ sym,
                                                        int* __restrict__ kmax) {
  const long long base = (long long)blockIdx.y * len;
  const long long src = (long long)img[blockIdx.y];
  const float* rs = r + src * len;
  const float* m1s = mu1 + src * len;
  const float* as = a + src * C;
  const float* bs = b + (long long)blockIdx.y * C;
  const float* m2s = mu2 + base;
  int* ss = sym + base;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  constexpr int W = VEC ? 4 : 1;
  // the channel of a thread's element advances by (stride * W) % C per iteration: no division in the loop
  const int step = (int)((stride * W) % C);
  int c = (int)((tid * W) % C);
  const long long n = len / W;   // VEC: C % 4 == 0, so len % 4 == 0
  int m = 0;
  for (long long i = tid; i < n; i += stride) {
    if (VEC) {
      const floatx4v rv = reinterpret_cast<const floatx4v*>(rs)[i];
      const floatx4v uv = reinterpret_cast<const floatx4v*>(m1s)[i];
      const floatx4v av = *reinterpret_cast<const floatx4v*>(as + c);
      const floatx4v bv = *reinterpret_cast<const floatx4v*>(bs + c);
      const floatx4v wv = reinterpret_cast<const floatx4v*>(m2s)[i];
      intx4v k;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        k[j] = requant_of(rv[j], uv[j], av[j], bv[j], wv[j]);
        m = max(m, k[j] < 0 ? -k[j] : k[j]);
      }
      reinterpret_cast<intx4v*>(ss)[i] = k;
    } else {
      const int k = requant_of(rs[i], m1s[i], as[c], bs[c], m2s[i]);
      ss[i] = k;
      m = max(m, k < 0 ? -k : k);
    }
    c += step;
    if (c >= C) c -= C;
  }
  m = block_max(m);
  if (threadIdx.x == 0) atomicMax(kmax + blockIdx.y, m);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ic_requant_seg(const float* r, const float* mu1, long long N, long long P, int C, const float* a, const float* b,
                   const float* mu2, int nseg, const int* img, int* img_dev, int* sym, int* kmax_dev, int* kmax_host,
                   void* stream) {
  if (!r || !mu1 || !a || !b || !mu2 || !img || !img_dev || !sym || !kmax_dev || !kmax_host) return IC_ERR_ARG;
  if (N < 1 || N > 65535 || P < 1 || C < 1 || nseg < 1 || nseg > 65535) return IC_ERR_ARG;
  if (P > 0x7fffffffffffffffll / C / std::max<long long>(N, nseg)) return IC_ERR_ARG;
  for (int m = 0; m < nseg; ++m)
    if (img[m] < 0 || img[m] >= N) return IC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  // the host array is consumed before this returns (a copy from pageable memory is staged by the runtime)
  hipError_t e = hipMemcpyAsync(img_dev, img, sizeof(int) * nseg, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(kmax_dev, 0, sizeof(int) * nseg, st);
  if (e != hipSuccess) return (int)e;
  const long long len = P * C;
  const bool vec = C % 4 == 0 && aligned16(r) && aligned16(mu1) && aligned16(a) && aligned16(b) && aligned16(mu2) &&
                   aligned16(sym);
  const long long work = len / (vec ? 4 : 1);
  const dim3 grid((unsigned)std::min<long long>((work + RQ_THREADS - 1) / RQ_THREADS, RQ_MAXBLOCKS), (unsigned)nseg);
  if (vec)
    hipLaunchKernelGGL(requant_k<true>, grid, dim3(RQ_THREADS), 0, st, r, mu1, a, b, mu2, img_dev, len, C, sym, kmax_dev);
  else
    hipLaunchKernelGGL(requant_k<false>, grid, dim3(RQ_THREADS), 0, st, r, mu1, a, b, mu2, img_dev, len, C, sym, kmax_dev);
  IC_CHECK_LAUNCH();
  e = hipMemcpyAsync(kmax_host, kmax_dev, sizeof(int) * nseg, hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return (int)e;
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  for (int m = 0; m < nseg; ++m)
    if (kmax_host[m] > IC_CODEC_KMAX) return IC_ERR_ARG;
  return IC_OK;
}

}  // extern "C"
