// Coding to a byte budget: the symbols of y for M candidate (image, quality) pairs in one launch
// (ic_gain_symbolize_seg).  Candidate m names its image img[m] of the N-image latent y and its own gain row g[m];
// its mean mu[m] and its symbols sym[m] are segments of P * C elements back to back:
//     sym[m][i] = symbol_of(fsub(fmul(y[img[m]][i], g[m][c(i)]), mu[m][i]))
//   * the product is ic_channel_scale's one fp32 multiplication (__fmul_rn) and the difference
//     ic_codec_symbolize_mean_seg's one fp32 subtraction (__fsub_rn), neither contracted with the other, and the
//     symbol is codec_sym.h's rule: bit for bit those two calls on the gathered batch y[img], without the gather
//     copy and without the scaled latent in memory;
//   * kmax[m] is one integer atomicMax per block: order-independent, deterministic.  No floating-point atomics.
// y, mu and sym are dense channels-last storage (P positions, channel fastest).  Grid-stride and HBM-bound, as
// meancodec.hip and gain.hip: 16-byte accesses when every pointer is 16-byte aligned and C % 4 == 0 (then every
// segment and every gain row starts on a 16-byte boundary and a group of four never straddles a position), scalar
// accesses with the same arithmetic otherwise.
#include <algorithm>

#include "common.h"
#include "codec_sym.h"
#include "../../include/imgcomp.h"

namespace {

typedef int intx4v __attribute__((ext_vector_type(4)));

constexpr int BG_THREADS = 256;
constexpr int BG_MAXBLOCKS = 1024;

// blockIdx.y = candidate; `len` = P * C elements per segment; kmax[candidate] = its max |symbol|
template <bool VEC>
__global__ void __launch_bounds__(BG_THREADS) gain_symbolize_k(const float* __restrict__ y, const float* __restrict__ g,
                                                               const float* __restrict__ mu, const int* __restrict__ img,
                                                               long long len, int C, int* __restrict__ sym,
                                                               int* __restrict__ kmax) {
  const long long base = (long long)blockIdx.y * len;
  const float* ys = y + (long long)img[blockIdx.y] * len;
  const float* gs = g + (long long)blockIdx.y * C;
  const float* ms = mu + base;
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
      const floatx4v a = reinterpret_cast<const floatx4v*>(ys)[i];
      const floatx4v b = *reinterpret_cast<const floatx4v*>(gs + c);
      const floatx4v u = reinterpret_cast<const floatx4v*>(ms)[i];
      intx4v k;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        k[j] = symbol_of(__fsub_rn(__fmul_rn(a[j], b[j]), u[j]));
        m = max(m, k[j] < 0 ? -k[j] : k[j]);
      }
      reinterpret_cast<intx4v*>(ss)[i] = k;
    } else {
      const int k = symbol_of(__fsub_rn(__fmul_rn(ys[i], gs[c]), ms[i]));
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

int ic_gain_symbolize_seg(const float* y, long long N, long long P, int C, const float* g, const float* mu, int nseg,
                          const int* img, int* img_dev, int* sym, int* kmax_dev, int* kmax_host, void* stream) {
  if (!y || !g || !mu || !img || !img_dev || !sym || !kmax_dev || !kmax_host) return IC_ERR_ARG;
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
  const bool vec = C % 4 == 0 && aligned16(y) && aligned16(g) && aligned16(mu) && aligned16(sym);
  const long long work = len / (vec ? 4 : 1);
  const dim3 grid((unsigned)std::min<long long>((work + BG_THREADS - 1) / BG_THREADS, BG_MAXBLOCKS), (unsigned)nseg);
  if (vec)
    hipLaunchKernelGGL(gain_symbolize_k<true>, grid, dim3(BG_THREADS), 0, st, y, g, mu, img_dev, len, C, sym, kmax_dev);
  else
    hipLaunchKernelGGL(gain_symbolize_k<false>, grid, dim3(BG_THREADS), 0, st, y, g, mu, img_dev, len, C, sym, kmax_dev);
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
