// Choosing a quality map under a byte budget (RegionGainedMeanScaleCompressor2018.compress_each_map_to): the per-block
// level choice of M candidate (image, weight) pairs in one launch (ic_block_allocate), and the symbols of y for M
// candidate (image, level map) pairs in one launch (ic_block_gain_symbolize_seg).
//   * The allocation is codec.py's rule: for block b of candidate m, J[l] = add_rn(bits[img[m]][l][b], mul_rn(w[m],
//     sse[img[m]][l][b])), each operation rounded once (fp_rn.h), l scanned ascending from best = 0 and replaced iff
//     J[l] < J[best] (strict: a tie keeps the lower level, a NaN never wins).
//   * The sums of the chosen bits and the chosen sse are fp64 in one fixed order, a function of nb alone: one HIP
//     block of 256 threads per candidate, thread t adds blocks t, t + 256, ... ascending, then the 256 partial sums
//     are folded in LDS, partial[t] += partial[t + s] for s = 128, 64, ..., 1.  No atomics.
//   * The symbols are sym[m][i] = symbol_of(sub_rn(mul_rn(y[img[m]][i], g[rank[m][block(i)]][c(i)]), mu[m][i])): the
//     product is ic_block_scale's one fp32 multiplication, with its walk over (row, column, channel) and its clamp of
//     a rank >= R to R - 1; the difference and the symbol are ic_codec_symbolize_mean_seg's: bit for bit those two
//     calls on the gathered batch y[img], without the gather copy and without the scaled latent in memory.
// y, mu and sym are dense channels-last storage (Hm, Wm, C per image, channel fastest).  The symbolizer is
// seg_symbolize.h's walk and driver over a source whose cursor is (row, column, channel): 16-byte accesses when every
// pointer is 16-byte aligned and C % 4 == 0.  The tables of the allocation are a few kilobytes (S levels of one value
// per 64 x 64 pixel block): scalar loads, coalesced along the blocks.
#include <algorithm>
#include <cmath>

#include "seg_symbolize.h"

namespace {

constexpr int MB_THREADS = 256;   // of the allocation: its fold in LDS is written for this many
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

// One image is Hm * Wm * C elements (< 2^31: checked on the host).  The walk is region.hip's block_scale_k: (row, column,
// channel) of a thread's element advance by the fixed steps (dpi, dpj, dc) of the launch's stride, worked out on the
// host, with at most one carry each.
struct BlockGainSrc {
  const float *y, *g, *mu;
  const unsigned char* rank;
  const int* img;
  int R, Wm, C, shift, nbw, nblk;   // nblk: the blocks of one candidate's map
  FastDiv by_c, by_w;
  int dc, dpj, dpi;
  int c, pj, pi;
  __device__ __forceinline__ void bind(unsigned seg, long long len, long long first, long long) {
    y += (long long)img[seg] * len;
    mu += (long long)seg * len;
    rank += (long long)seg * nblk;
    const uint32_t p0 = fdiv((uint32_t)first, by_c);
    c = (int)((uint32_t)first - p0 * C), pi = (int)fdiv(p0, by_w);
    pj = (int)(p0 - (uint32_t)pi * Wm);
  }
  template <class V>
  __device__ __forceinline__ V at(long long i) const {
    const int row = min((int)rank[(pi >> shift) * nbw + (pj >> shift)], R - 1);
    return sub_rn(mul_rn(load_as<V>(y, i), load_as<V>(g + (long long)row * C + c, 0)), load_as<V>(mu, i));
  }
  __device__ __forceinline__ void next() {
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
};

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
  const bool vec = C % 4 == 0 && aligned16(y) && aligned16(g) && aligned16(mu) && aligned16(sym);
  const long long len = (long long)Hm * Wm * C;
  const int nbh = map_extent(Hm, shift), nbw = map_extent(Wm, shift);
  // the steps of one grid stride in (row, column, channel)
  const long long se = (long long)seg_blocks(len, vec) * SEG_THREADS * (vec ? 4 : 1), dp = se / C;
  const int dc = (int)(se % C), dpj = (int)(dp % Wm), dpi = (int)(dp / Wm);
  const BlockGainSrc src{y, g, mu, rank, img_dev, R, Wm, C, shift, nbw, nbh * nbw, make_fastdiv((uint32_t)C),
                         make_fastdiv((uint32_t)Wm), dc, dpj, dpi, 0, 0, 0};
  return seg_symbolize(src, vec, nseg, len, img, img_dev, sym, kmax_dev, kmax_host, (hipStream_t)stream);
}

}  // extern "C"
