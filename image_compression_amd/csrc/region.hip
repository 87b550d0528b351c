// Region-of-interest coding (RegionGainedMeanScaleCompressor2018): the scaling of a latent by a gain row chosen per
// block of positions instead of per image, and the block-weighted squared error it is trained with
// (ic_block_scale*, ic_block_mse*).
//   * A block map holds one uint8 rank per block of 2^shift x 2^shift positions: position (i, j) of image n takes
//     row idx[n, i >> shift, j >> shift] of the R rows (gains (R, C), or weights (R)).  A rank >= R can only come
//     from a bad caller: it is clamped to R - 1, nothing is read out of bounds.
//   * out = x * g[row] is one fp32 multiplication per element (__fmul_rn), as in gain.hip.
//   * No floating-point atomics, every sum in a fixed order: dg per block over its positions in ascending (i, j),
//     then one thread per (rank, c) over the blocks in ascending (n, bi, bj); the squared errors per HIP block (a
//     function of the shape alone), then one block over the partial sums.  Bitwise the same from run to run.
// Latents are dense channels-last storage (N, Hm, Wm, C); the scaling kernels are grid-stride and HBM-bound: 16-byte
// accesses when every pointer is 16-byte aligned and C % 4 == 0, scalar otherwise.  Images are (N, C, H, W) with
// the strides given in the call, walked in the order of their storage.
#include <algorithm>

#include "common.h"
#include "../../include/imgcomp.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_MAXBLOCKS = 1024;
constexpr int RG_BATCH = 64;       // partial sums the second stage loads before it adds them
constexpr int RG_MAXPART = 4096;    // HIP blocks of the squared error's first stage over all images, about
constexpr int RG_ITEMS = 8;         // elements per thread of that stage, at least

__device__ __forceinline__ int rank_of(const unsigned char* __restrict__ ids, int at, int R) {
  return min((int)ids[at], R - 1);
}

// out = x * g[rank of the position's block]; image blockIdx.y
template <bool VEC>
__global__ void __launch_bounds__(RG_THREADS) block_scale_k(const float* __restrict__ x, const float* __restrict__ g, int R,
                                                            const unsigned char* __restrict__ idx, int Hm, int Wm, int C,
                                                            int shift, int nbh, int nbw, FastDiv by_c, FastDiv by_w,
                                                            int dc, int dpj, int dpi, float* __restrict__ out) {
  constexpr int W = VEC ? 4 : 1;
  const uint32_t len = (uint32_t)Hm * Wm * C;   // < 2^31: checked on the host
  const float* xs = x + (long long)blockIdx.y * len;
  float* os = out + (long long)blockIdx.y * len;
  const unsigned char* ids = idx + (long long)blockIdx.y * nbh * nbw;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t stride = gridDim.x * blockDim.x;
  // (row i, column j, channel c) of a thread's element advance by the fixed steps (dpi, dpj, dc) of the launch's
  // stride, worked out on the host, with at most one carry each: no division in the loop, two by multiplication
  // in front of it
  const uint32_t p0 = fdiv(tid * W, by_c);
  int c = (int)(tid * W - p0 * C), pi = (int)fdiv(p0, by_w);
  int pj = (int)(p0 - (uint32_t)pi * Wm);
  const uint32_t n = len / W;   // VEC: C % 4 == 0, so len % 4 == 0
  for (uint32_t i = tid; i < n; i += stride) {
    const float* gs = g + (long long)rank_of(ids, (pi >> shift) * nbw + (pj >> shift), R) * C + c;
    if (VEC) {
      const floatx4v a = reinterpret_cast<const floatx4v*>(xs)[i];
      const floatx4v b = *reinterpret_cast<const floatx4v*>(gs);
      floatx4v o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fmul_rn(a[j], b[j]);
      reinterpret_cast<floatx4v*>(os)[i] = o;
    } else {
      os[i] = __fmul_rn(xs[i], gs[0]);
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
}

// First stage of the gradient: one thread per (n, bi, bj, channel group).  Over the block's positions in ascending
// (i, j): dx = dy * g[rank], and part[(n, bi, bj)][c] = the sum of dy x.
template <bool VEC>
__global__ void __launch_bounds__(RG_THREADS) block_scale_bwd_k(const float* __restrict__ x, const float* __restrict__ g,
                                                                int R, const unsigned char* __restrict__ idx,
                                                                const float* __restrict__ dy, long long nblocks, int Hm,
                                                                int Wm, int C, int shift, int nbh, int nbw,
                                                                float* __restrict__ dx, float* __restrict__ part) {
  constexpr int W = VEC ? 4 : 1;
  const int G = C / W;
  const long long total = nblocks * G;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const long long b = t / G;
    const int c = (int)(t % G) * W;
    const int bj = (int)(b % nbw), bi = (int)(b / nbw % nbh);
    const long long n = b / nbw / nbh;
    const int row = min((int)idx[b], R - 1);
    const int i0 = bi << shift, i1 = min(Hm, (bi + 1) << shift), j0 = bj << shift, j1 = min(Wm, (bj + 1) << shift);
    float gv[W], acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      gv[k] = g[(long long)row * C + c + k];
      acc[k] = 0.0f;
    }
    for (int i = i0; i < i1; ++i) {
      long long at = ((n * Hm + i) * Wm + j0) * C + c;
#pragma unroll 4
      for (int j = j0; j < j1; ++j, at += C) {
        if (VEC) {
          const floatx4v a = *reinterpret_cast<const floatx4v*>(x + at);
          const floatx4v d = *reinterpret_cast<const floatx4v*>(dy + at);
          floatx4v o;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            o[k] = __fmul_rn(d[k], gv[k]);
            acc[k] += d[k] * a[k];
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
    for (int k = 0; k < W; ++k) part[b * C + c + k] = acc[k];
  }
}

// Second stage: dg[r][c] = the partial sums of the blocks of rank r, in ascending (n, bi, bj); a block of another
// rank adds +0.0, which changes no bit of a sum that starts at +0.0
__global__ void __launch_bounds__(RG_THREADS) block_scale_dg_k(const float* __restrict__ part,
                                                               const unsigned char* __restrict__ idx, long long nblocks,
                                                               int R, int C, float* __restrict__ dg) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)R * C) return;
  const int r = (int)(i / C), c = (int)(i % C);
  // RG_BATCH loads in flight, then their additions in order (gain.hip channel_scale_dg_k).  Every load is
  // unconditional, from a block index clamped into range, and the choice is made on the loaded values: a load under
  // a condition becomes a branch, and the branches wait for one another's loads
  float s = 0.0f;
  for (long long b0 = 0; b0 < nblocks; b0 += RG_BATCH) {
    float v[RG_BATCH];
    int k[RG_BATCH];
#pragma unroll
    for (int u = 0; u < RG_BATCH; ++u) {
      const long long b = b0 + u < nblocks ? b0 + u : nblocks - 1;
      k[u] = idx[b];
      v[u] = part[b * C + c];
    }
#pragma unroll
    for (int u = 0; u < RG_BATCH; ++u) s += b0 + u < nblocks && min(k[u], R - 1) == r ? v[u] : 0.0f;
  }
  dg[i] = s;
}

// ---- the block-weighted squared error of two images (N, C, H, W) with shared strides
struct ImgWalk {
  long long sn, sc, sh, sw;
  FastDiv inner, mid;   // the two faster extents of the walk: (W, H) in NCHW order, (C, W) channels last
  int H, W, C, cl, nbh, nbw;
  long long len;        // C H W < 2^31
};

// element e of an image in the order of its storage -> its offset and its block
__device__ __forceinline__ void walk(const ImgWalk& g, uint32_t e, long long& off, int& blk) {
  const uint32_t t = fdiv(e, g.inner), r0 = e - t * g.inner.d;
  const uint32_t u = fdiv(t, g.mid), r1 = t - u * g.mid.d;
  int c, h, w;
  if (g.cl) {
    c = (int)r0, w = (int)r1, h = (int)u;
  } else {
    w = (int)r0, h = (int)r1, c = (int)u;
  }
  off = c * g.sc + h * g.sh + w * g.sw;
  blk = (h >> 6) * g.nbw + (w >> 6);
}

// part[(n * gridDim.x + block)] = {sum of w[rank] d^2, sum of d^2} over the block's elements of image n
__global__ void __launch_bounds__(RG_THREADS) block_mse_partial_k(const float* __restrict__ a, const float* __restrict__ b,
                                                                  const float* __restrict__ wts, int R,
                                                                  const unsigned char* __restrict__ idx, ImgWalk g,
                                                                  float* __restrict__ part) {
  __shared__ float lds[32];
  const float* as = a + (long long)blockIdx.y * g.sn;
  const float* bs = b + (long long)blockIdx.y * g.sn;
  const unsigned char* ids = idx + (long long)blockIdx.y * g.nbh * g.nbw;
  float v[2] = {0.0f, 0.0f};
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.len; e += (long long)gridDim.x * blockDim.x) {
    long long off;
    int blk;
    walk(g, (uint32_t)e, off, blk);
    const float d = as[off] - bs[off];
    const float d2 = d * d;
    v[0] += wts[rank_of(ids, blk, R)] * d2;
    v[1] += d2;
  }
  block_sum<2>(v, lds);
  if (threadIdx.x == 0) {
    float* p = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    p[0] = v[0];
    p[1] = v[1];
  }
}

__global__ void __launch_bounds__(RG_THREADS) block_mse_final_k(const float* __restrict__ part, long long nb, float scale,
                                                                float* __restrict__ out) {
  __shared__ float lds[32];
  float v[2] = {0.0f, 0.0f};
  for (long long i = threadIdx.x; i < nb; i += blockDim.x) {
    v[0] += part[2 * i];
    v[1] += part[2 * i + 1];
  }
  block_sum<2>(v, lds);
  if (threadIdx.x == 0) {
    out[0] = v[0] * scale;
    out[1] = v[1] * scale;
  }
}

// ga = gout 2 w[rank] (a - b) / n, gb = -ga, each with the inputs' strides
__global__ void __launch_bounds__(RG_THREADS) block_mse_bwd_k(const float* __restrict__ a, const float* __restrict__ b,
                                                              const float* __restrict__ wts, int R,
                                                              const unsigned char* __restrict__ idx,
                                                              const float* __restrict__ gout, ImgWalk g, float scale,
                                                              float* __restrict__ ga, float* __restrict__ gb) {
  const long long base = (long long)blockIdx.y * g.sn;
  const unsigned char* ids = idx + (long long)blockIdx.y * g.nbh * g.nbw;
  const float s = gout[0] * scale;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.len; e += (long long)gridDim.x * blockDim.x) {
    long long off;
    int blk;
    walk(g, (uint32_t)e, off, blk);
    off += base;
    const float d = (a[off] - b[off]) * (s * wts[rank_of(ids, blk, R)]);
    if (ga) ga[off] = d;
    if (gb) gb[off] = -d;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- the host checks, before any launch
bool scale_ok(int R, int N, int Hm, int Wm, int C, int shift) {
  if (R < 1 || R > 256 || N < 1 || N > 65535 || Hm < 1 || Wm < 1 || C < 1 || shift < 0 || shift > 6) return false;
  return (long long)Hm * Wm <= 0x7fffffffll / C;   // one image's elements are indexed in 32 bits
}

int map_extent(int v, int shift) { return (int)(((long long)v + (1 << shift) - 1) >> shift); }

bool image_ok(int R, int N, int C, int H, int W, long long sn, long long sc, long long sh, long long sw) {
  if (R < 1 || R > 256 || N < 1 || N > 65535 || C < 1 || H < 1 || W < 1) return false;
  if (sn < 1 || sc < 1 || sh < 1 || sw < 1) return false;
  return (long long)C * H <= 0x7fffffffll / W;
}

ImgWalk make_walk(int C, int H, int W, long long sn, long long sc, long long sh, long long sw) {
  ImgWalk g;
  g.sn = sn, g.sc = sc, g.sh = sh, g.sw = sw;
  g.H = H, g.W = W, g.C = C;
  g.cl = sc == 1 && sw != 1 ? 1 : 0;   // channel fastest in storage: walk (h, w, c); otherwise (c, h, w)
  g.inner = make_fastdiv((uint32_t)(g.cl ? C : W));
  g.mid = make_fastdiv((uint32_t)(g.cl ? W : H));
  g.nbh = map_extent(H, 6), g.nbw = map_extent(W, 6);
  g.len = (long long)C * H * W;
  return g;
}

// HIP blocks per image of the squared error's first stage: a function of the shape alone (the workspace query and
// the launch agree on it)
long long mse_blocks(int N, long long len) {
  const long long want = (len + (long long)RG_THREADS * RG_ITEMS - 1) / ((long long)RG_THREADS * RG_ITEMS);
  return std::max<long long>(1, std::min<long long>(want, std::max<long long>(1, RG_MAXPART / N)));
}

}  // namespace

extern "C" {

int ic_block_scale(const float* x, const float* g, int R, const unsigned char* idx, int N, int Hm, int Wm, int C,
                   int shift, float* out, void* stream) {
  if (!x || !g || !idx || !out || !scale_ok(R, N, Hm, Wm, C, shift)) return IC_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(out);
  const int w = vec ? 4 : 1;
  const long long work = (long long)Hm * Wm * C / w;
  const dim3 grid((unsigned)std::min<long long>((work + RG_THREADS - 1) / RG_THREADS, RG_MAXBLOCKS), (unsigned)N);
  const int nbh = map_extent(Hm, shift), nbw = map_extent(Wm, shift);
  // the steps of one grid stride in (row, column, channel)
  const long long se = (long long)grid.x * RG_THREADS * w, dp = se / C;
  const int dc = (int)(se % C), dpj = (int)(dp % Wm), dpi = (int)(dp / Wm);
  const FastDiv by_c = make_fastdiv((uint32_t)C), by_w = make_fastdiv((uint32_t)Wm);
  if (vec)
    hipLaunchKernelGGL(block_scale_k<true>, grid, dim3(RG_THREADS), 0, (hipStream_t)stream, x, g, R, idx, Hm, Wm, C, shift,
                       nbh, nbw, by_c, by_w, dc, dpj, dpi, out);
  else
    hipLaunchKernelGGL(block_scale_k<false>, grid, dim3(RG_THREADS), 0, (hipStream_t)stream, x, g, R, idx, Hm, Wm, C,
                       shift, nbh, nbw, by_c, by_w, dc, dpj, dpi, out);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

size_t ic_block_scale_bwd_ws(int N, int Hm, int Wm, int C, int shift) {
  if (!scale_ok(1, N, Hm, Wm, C, shift)) return 0;
  return (size_t)N * map_extent(Hm, shift) * map_extent(Wm, shift) * (size_t)C * sizeof(float);
}

int ic_block_scale_bwd(const float* x, const float* g, int R, const unsigned char* idx, const float* dy, int N, int Hm,
                       int Wm, int C, int shift, float* dx, float* dg, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !g || !idx || !dy || !dx || !dg || !ws || !scale_ok(R, N, Hm, Wm, C, shift)) return IC_ERR_ARG;
  if (ws_bytes < ic_block_scale_bwd_ws(N, Hm, Wm, C, shift)) return IC_ERR_WORKSPACE;
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(dx);
  const int nbh = map_extent(Hm, shift), nbw = map_extent(Wm, shift);
  const long long nblocks = (long long)N * nbh * nbw, work = nblocks * (C / (vec ? 4 : 1));
  const dim3 grid((unsigned)std::min<long long>((work + RG_THREADS - 1) / RG_THREADS, 4 * RG_MAXBLOCKS));
  float* part = (float*)ws;
  if (vec)
    hipLaunchKernelGGL(block_scale_bwd_k<true>, grid, dim3(RG_THREADS), 0, (hipStream_t)stream, x, g, R, idx, dy, nblocks,
                       Hm, Wm, C, shift, nbh, nbw, dx, part);
  else
    hipLaunchKernelGGL(block_scale_bwd_k<false>, grid, dim3(RG_THREADS), 0, (hipStream_t)stream, x, g, R, idx, dy, nblocks,
                       Hm, Wm, C, shift, nbh, nbw, dx, part);
  IC_CHECK_LAUNCH();
  hipLaunchKernelGGL(block_scale_dg_k, dim3(ic_cdiv((long long)R * C, RG_THREADS)), dim3(RG_THREADS), 0,
                     (hipStream_t)stream, part, idx, nblocks, R, C, dg);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

size_t ic_block_mse_ws(int N, int C, int H, int W) {
  if (!image_ok(1, N, C, H, W, 1, 1, 1, 1)) return 0;
  return (size_t)(N * mse_blocks(N, (long long)C * H * W)) * 2 * sizeof(float);
}

int ic_block_mse_fwd(const float* a, const float* b, const float* w, int R, const unsigned char* idx, int N, int C, int H,
                     int W, long long sn, long long sc, long long sh, long long sw, float* out, void* ws, size_t ws_bytes,
                     void* stream) {
  if (!a || !b || !w || !idx || !out || !ws || !image_ok(R, N, C, H, W, sn, sc, sh, sw)) return IC_ERR_ARG;
  if (ws_bytes < ic_block_mse_ws(N, C, H, W)) return IC_ERR_WORKSPACE;
  const ImgWalk g = make_walk(C, H, W, sn, sc, sh, sw);
  const long long nb = mse_blocks(N, g.len);
  float* part = (float*)ws;
  hipLaunchKernelGGL(block_mse_partial_k, dim3((unsigned)nb, (unsigned)N), dim3(RG_THREADS), 0, (hipStream_t)stream, a, b,
                     w, R, idx, g, part);
  IC_CHECK_LAUNCH();
  const float scale = 1.0f / ((float)N * (float)g.len);
  hipLaunchKernelGGL(block_mse_final_k, dim3(1), dim3(RG_THREADS), 0, (hipStream_t)stream, part, nb * N, scale, out);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_block_mse_bwd(const float* a, const float* b, const float* w, int R, const unsigned char* idx, const float* gout,
                     int N, int C, int H, int W, long long sn, long long sc, long long sh, long long sw, float* ga,
                     float* gb, void* stream) {
  if (!a || !b || !w || !idx || !gout || (!ga && !gb) || !image_ok(R, N, C, H, W, sn, sc, sh, sw)) return IC_ERR_ARG;
  const ImgWalk g = make_walk(C, H, W, sn, sc, sh, sw);
  const dim3 grid((unsigned)std::min<long long>((g.len + RG_THREADS - 1) / RG_THREADS, RG_MAXBLOCKS), (unsigned)N);
  const float scale = 2.0f / ((float)N * (float)g.len);
  hipLaunchKernelGGL(block_mse_bwd_k, grid, dim3(RG_THREADS), 0, (hipStream_t)stream, a, b, w, R, idx, gout, g, scale, ga,
                     gb);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
