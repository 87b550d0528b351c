// Choosing a quality map under a byte budget (RegionGainedMeanScaleCompressor2018.compress_each_map_to): the per-block
// level choice of M candidate (image, weight) pairs in one launch (ic_block_allocate), and the symbols of y for M
// candidate (image, level map) pairs in one launch (ic_block_gain_symbolize_seg).
//   * The allocation is codec.py's rule: for block b of candidate m, J[l] = fadd(bits[img[m]][l][b], fmul(w[m],
//     sse[img[m]][l][b])), each operation rounded once (mul_rn, add_rn below: compiled with contraction off), l scanned
//     ascending from best = 0 and replaced iff J[l] < J[best] (strict: a tie keeps the lower level, a NaN never wins).
//   * The sums of the chosen bits and the chosen sse are fp64 in one fixed order, a function of nb alone: one HIP
//     block of 256 threads per candidate, thread t adds blocks t, t + 256, ... ascending, then the 256 partial sums
//     are folded in LDS, partial[t] += partial[t + s] for s = 128, 64, ..., 1.  No atomics.
//   * The symbols are sym[m][i] = symbol_of(fsub(fmul(y[img[m]][i], g[rank[m][block(i)]][c(i)]), mu[m][i])): the
//     product is ic_block_scale's one fp32 multiplication, with its walk over (row, column, channel) and its clamp of
//     a rank >= R to R - 1; the difference and the symbol are ic_codec_symbolize_mean_seg's: bit for bit those two
//     calls on the gathered batch y[img], without the gather copy and without the scaled latent in memory.  kmax[m] is
//     one integer atomicMax per block: order-independent, deterministic.  No floating-point atomics.
// y, mu and sym are dense channels-last storage (Hm, Wm, C per image, channel fastest).  The symbolizer is grid-stride
// and HBM-bound, as budget.hip and region.hip: 16-byte accesses when every pointer is 16-byte aligned and C % 4 == 0,
// scalar accesses with the same arithmetic otherwise.  The tables of the allocation are a few kilobytes (S levels of
// one value per 64 x 64 pixel block): scalar loads, coalesced along the blocks.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "codec_sym.h"
#include "../../include/imgcomp.h"

// A product and the sum that follows it, each rounded once.  The header's __fmul_rn followed by __fadd_rn / __fsub_rn
// does not say that to the compiler: they are a plain product and a plain sum compiled under its default contraction,
// and the pair becomes one v_fma_f32, one rounding instead of the two the rules state: a symbol or a level that
// differs from the two separate kernels where the product is inexact and the sum lands on a tie (one symbol of y in
// 2.4 million on the benchmark's images).  The three helpers below are compiled with contraction off, so neither
// operation carries the flag that lets the backend fuse it; the disassembly of this file holds no fused multiply-add.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

typedef int intx4v __attribute__((ext_vector_type(4)));

constexpr int MB_THREADS = 256;
constexpr int MB_MAXBLOCKS = 1024;
constexpr int MB_MAXLEVELS = 16;

// the codes of the L <= 16 levels, eight to a word: level l is byte l & 7 of word l >> 3
struct LevelCodes {
  unsigned long long w[2];
};

// blockIdx.x = candidate; bits, sse (N, L, nb); ranks, codes (M, nb); sums (2, M)
__global__ void __launch_bounds__(MB_THREADS) block_allocate_k(const float* __restrict__ bits, const float* __restrict__ sse,
                                                               int L, long long nb, const int* __restrict__ img,
                                                               const float* __restrict__ w, LevelCodes lut,
                                                               unsigned char* __restrict__ ranks,
                                                               unsigned char* __restrict__ codes,
                                                               double* __restrict__ sums) {
  __shared__ double part[2][MB_THREADS];
  const long long m = blockIdx.x;
  const long long base = (long long)img[m] * L * nb;
  const float wm = w[m];
  double sum_b = 0.0, sum_d = 0.0;
  for (long long b = threadIdx.x; b < nb; b += MB_THREADS) {
    const float* pb = bits + base + b;
    const float* pd = sse + base + b;
    int best = 0;
    float best_b = pb[0], best_d = pd[0];
    float best_j = add_rn(best_b, mul_rn(wm, best_d));
    for (int l = 1; l < L; ++l) {
      const float vb = pb[l * nb], vd = pd[l * nb];
      const float j = add_rn(vb, mul_rn(wm, vd));
      if (j < best_j) {
        best = l;
        best_j = j;
        best_b = vb;
        best_d = vd;
      }
    }
    ranks[m * nb + b] = (unsigned char)best;
    codes[m * nb + b] = (unsigned char)(lut.w[best >> 3] >> (8 * (best & 7)));
    sum_b += (double)best_b;
    sum_d += (double)best_d;
  }
  part[0][threadIdx.x] = sum_b;
  part[1][threadIdx.x] = sum_d;
  __syncthreads();
  for (int s = MB_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      part[0][threadIdx.x] += part[0][threadIdx.x + s];
      part[1][threadIdx.x] += part[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sums[m] = part[0][0];
    sums[gridDim.x + m] = part[1][0];
  }
}

// blockIdx.y = candidate; one image is Hm * Wm * C elements (< 2^31: checked on the host); kmax[candidate] = its max
// |symbol|.  The walk is region.hip's block_scale_k: (row, column, channel) of a thread's element advance by the fixed
// steps (dpi, dpj, dc) of the launch's stride, worked out on the host, with at most one carry each.
template <bool VEC>
__global__ void __launch_bounds__(MB_THREADS) block_gain_symbolize_k(const float* __restrict__ y, const float* __restrict__ g,
                                                                     int R, const unsigned char* __restrict__ rank,
                                                                     const float* __restrict__ mu,
                                                                     const int* __restrict__ img, int Hm, int Wm, int C,
                                                                     int shift, int nbh, int nbw, FastDiv by_c, FastDiv by_w,
                                                                     int dc, int dpj, int dpi, int* __restrict__ sym,
                                                                     int* __restrict__ kmax) {
  constexpr int W = VEC ? 4 : 1;
  const uint32_t len = (uint32_t)Hm * Wm * C;
  const float* ys = y + (long long)img[blockIdx.y] * len;
  const float* ms = mu + (long long)blockIdx.y * len;
  int* ss = sym + (long long)blockIdx.y * len;
  const unsigned char* ids = rank + (long long)blockIdx.y * nbh * nbw;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t p0 = fdiv(tid * W, by_c);
  int c = (int)(tid * W - p0 * C), pi = (int)fdiv(p0, by_w);
  int pj = (int)(p0 - (uint32_t)pi * Wm);
  const uint32_t n = len / W;   // VEC: C % 4 == 0, so len % 4 == 0
  int m = 0;
  for (uint32_t i = tid; i < n; i += stride) {
    const int row = min((int)ids[(pi >> shift) * nbw + (pj >> shift)], R - 1);
    const float* gs = g + (long long)row * C + c;
    if (VEC) {
      const floatx4v a = reinterpret_cast<const floatx4v*>(ys)[i];
      const floatx4v b = *reinterpret_cast<const floatx4v*>(gs);
      const floatx4v u = reinterpret_cast<const floatx4v*>(ms)[i];
      intx4v k;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        k[j] = symbol_of(sub_rn(mul_rn(a[j], b[j]), u[j]));
        m = max(m, k[j] < 0 ? -k[j] : k[j]);
      }
      reinterpret_cast<intx4v*>(ss)[i] = k;
    } else {
      const int k = symbol_of(sub_rn(mul_rn(ys[i], gs[0]), ms[i]));
      ss[i] = k;
      m = max(m, k < 0 ? -k : k);
    }
    c += dc;
    if (c >= C) {
      c -= C;
      ++pj;
    }
    pj += dpj;
    if (pj >= Wm) {
      pj -= Wm;
      ++pi;
    }
    pi += dpi;
  }
  m = block_max(m);
  if (threadIdx.x == 0) atomicMax(kmax + blockIdx.y, m);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int map_extent(int v, int shift) { return (int)(((long long)v + (1 << shift) - 1) >> shift); }

}  // namespace

extern "C" {

int ic_block_allocate(const float* bits, const float* sse, int N, int L, long long nb, int M, const int* img,
                      const float* w, const unsigned char* level_codes, void* cand_dev, unsigned char* ranks,
                      unsigned char* codes, double* sums, void* stream) {
  if (!bits || !sse || !img || !w || !level_codes || !cand_dev || !ranks || !codes || !sums) return IC_ERR_ARG;
  if (N < 1 || N > 65535 || L < 2 || L > MB_MAXLEVELS || nb < 1 || M < 1 || M > 65535) return IC_ERR_ARG;
  if (nb > 0x7fffffffffffffffll / L / std::max(N, M)) return IC_ERR_ARG;
  for (int m = 0; m < M; ++m)
    if (img[m] < 0 || img[m] >= N || !std::isfinite(w[m]) || w[m] < 0.0f) return IC_ERR_ARG;
  LevelCodes lut = {{0ull, 0ull}};
  for (int l = 0; l < L; ++l) lut.w[l >> 3] |= (unsigned long long)level_codes[l] << (8 * (l & 7));
  hipStream_t st = (hipStream_t)stream;
  int* img_dev = (int*)cand_dev;
  float* w_dev = (float*)(img_dev + M);
  // the host arrays are consumed before this returns (a copy from pageable memory is staged by the runtime)
  hipError_t e = hipMemcpyAsync(img_dev, img, sizeof(int) * M, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(w_dev, w, sizeof(float) * M, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(block_allocate_k, dim3((unsigned)M), dim3(MB_THREADS), 0, st, bits, sse, L, nb, img_dev, w_dev, lut,
                     ranks, codes, sums);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_block_gain_symbolize_seg(const float* y, int N, int Hm, int Wm, int C, const float* g, int R,
                                const unsigned char* rank, int shift, const float* mu, int nseg, const int* img,
                                int* img_dev, int* sym, int* kmax_dev, int* kmax_host, void* stream) {
  if (!y || !g || !rank || !mu || !img || !img_dev || !sym || !kmax_dev || !kmax_host) return IC_ERR_ARG;
  if (R < 1 || R > 256 || N < 1 || N > 65535 || Hm < 1 || Wm < 1 || C < 1 || shift < 0 || shift > 6) return IC_ERR_ARG;
  if (nseg < 1 || nseg > 65535) return IC_ERR_ARG;
  if ((long long)Hm * Wm > 0x7fffffffll / C) return IC_ERR_ARG;   // one image's elements are indexed in 32 bits
  for (int m = 0; m < nseg; ++m)
    if (img[m] < 0 || img[m] >= N) return IC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  // the host array is consumed before this returns (a copy from pageable memory is staged by the runtime)
  hipError_t e = hipMemcpyAsync(img_dev, img, sizeof(int) * nseg, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(kmax_dev, 0, sizeof(int) * nseg, st);
  if (e != hipSuccess) return (int)e;
  const bool vec = C % 4 == 0 && aligned16(y) && aligned16(g) && aligned16(mu) && aligned16(sym);
  const int w = vec ? 4 : 1;
  const long long work = (long long)Hm * Wm * C / w;
  const dim3 grid((unsigned)std::min<long long>((work + MB_THREADS - 1) / MB_THREADS, MB_MAXBLOCKS), (unsigned)nseg);
  const int nbh = map_extent(Hm, shift), nbw = map_extent(Wm, shift);
  // the steps of one grid stride in (row, column, channel)
  const long long se = (long long)grid.x * MB_THREADS * w, dp = se / C;
  const int dc = (int)(se % C), dpj = (int)(dp % Wm), dpi = (int)(dp / Wm);
  const FastDiv by_c = make_fastdiv((uint32_t)C), by_w = make_fastdiv((uint32_t)Wm);
  if (vec)
    hipLaunchKernelGGL(block_gain_symbolize_k<true>, grid, dim3(MB_THREADS), 0, st, y, g, R, rank, mu, img_dev, Hm, Wm, C,
                       shift, nbh, nbw, by_c, by_w, dc, dpj, dpi, sym, kmax_dev);
  else
    hipLaunchKernelGGL(block_gain_symbolize_k<false>, grid, dim3(MB_THREADS), 0, st, y, g, R, rank, mu, img_dev, Hm, Wm, C,
                       shift, nbh, nbw, by_c, by_w, dc, dpj, dpi, sym, kmax_dev);
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
