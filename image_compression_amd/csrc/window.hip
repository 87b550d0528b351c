// Decoding a pixel window of a per-image stream (ic_codec_decode_window, ic_crop_clamp_at;
// Compressor2018.decompress_window; the plan: image_compression_amd/codec.py).
//   * A latent's symbols lie in (row, column, channel) order and its chunks are coded independently, so the rows of
//     a window are a range of chunks.  The host brings the payload of those chunks only, with every chunk's word span,
//     and one wavefront decodes one (window, chunk) pair by codec.hip's decode_chunk (codec_chunk.h): the same
//     arithmetic, guards and table choice.  The states of a chunk are serial, so every symbol is decoded; a symbol
//     is stored only where its (row, column) lies in the window, as (float)q or, about a mean, (float)q + mu: one
//     fp32 addition never contracted with anything, the bits ic_add_mean gives after ic_codec_decode_seg.
//   * The descriptors come from untrusted streams: the entry point checks every one of them before anything
//     touches the device, and the kernel's indices are inside their buffers for every descriptor that passes.
#include <algorithm>
#include <vector>

#include "common.h"
#include "codec_chunk.h"
#include "../../include/imgcomp.h"

namespace {

// one window as the kernel reads it (the checked ic_window; dw: the divider by wy)
struct WinDev {
  long long base;
  int hy, wy, K, table, r0, c0;
  FastDiv dw;
};

// one block: its window, its chunk of the window's segment, its chunk's word span in the input
struct BlockDev {
  long long begin, end;
  int win, chunk;
};

// the workspace holds the windows, then the blocks: the second array stays 8-byte aligned
static_assert(sizeof(WinDev) % 8 == 0 && sizeof(BlockDev) % 8 == 0, "descriptor arrays lie back to back");

struct WinArgs {
  const WinDev* wins;
  const BlockDev* blocks;
  const unsigned char* rows;
  const float* mu;
  const uint32_t* pool;
  int C, nrows, R, rh, rw;
  FastDiv dc;   // the divider by C
};

// What the window decoder stores: symbol q of global index g = base + l at position l / C = (row, column), channel
// l % C, where the window holds it.  l < 2^31 (checked by the host), which the dividers need.
struct StoreWindow {
  const WinArgs& w;
  const WinDev& d;
  float* __restrict__ out;   // the block's window: (rh, rw, C) dense
  __device__ __forceinline__ void operator()(long long g, int q) const {
    const uint32_t l = (uint32_t)(g - d.base);
    const uint32_t pos = fdiv(l, w.dc), ch = l - pos * (uint32_t)w.C;
    const uint32_t row = fdiv(pos, d.dw), col = pos - row * (uint32_t)d.wy;
    const uint32_t rr = row - (uint32_t)d.r0, cc = col - (uint32_t)d.c0;   // below r0 / c0: wraps to a large value
    if (rr < (uint32_t)w.rh && cc < (uint32_t)w.rw) {
      const float v = (float)q;
      out[((size_t)rr * w.rw + cc) * w.C + ch] = w.mu ? __fadd_rn(v, w.mu[g]) : v;
    }
  }
};

__global__ void __launch_bounds__(64) codec_decode_window_k(const unsigned short* __restrict__ in, size_t in_words,
                                                            WinArgs w, float* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  const BlockDev b = w.blocks[blockIdx.x];
  const WinDev d = w.wins[b.win];
  const long long seg_len = (long long)d.hy * d.wy * w.C;
  const long long per = 64ll * w.R, l0 = (long long)b.chunk * per;
  const int nc = (int)min(per, seg_len - l0);
  const size_t begin = min((size_t)b.begin, in_words), end = min((size_t)b.end, in_words);
  const CodecArgs a{seg_len, w.rows, w.C, w.pool + d.table, w.nrows, d.K, w.R};
  const StoreWindow store{w, d, out + (size_t)b.win * w.rh * w.rw * w.C};
  if (table_bytes(a.nrows, a.K) <= CODEC_LDS_BYTES)
    decode_chunk<true>(in, begin, end, a, d.base + l0, nc, store, lds);
  else
    decode_chunk<false>(in, begin, end, a, d.base + l0, nc, store, lds);
}

// y (N, C, h, w dense) = crop_clamp_k's two bounds (elementwise.hip: upper 1, then lower 0) on the h x w of x at
// (top, left)
__global__ void crop_clamp_at_k(const float* __restrict__ x, long long sn, long long sc, long long sh, long long sw,
                                long long n, int C, int top, int left, int h, int w, float* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i % w), r = (int)((i / w) % h);
    const long long p = i / ((long long)w * h);
    const float v = x[(p / C) * sn + (p % C) * sc + (long long)(top + r) * sh + (long long)(left + j) * sw];
    const float u = v < 1.f ? v : 1.f;
    y[i] = u > 0.f ? u : 0.f;
  }
}

// ---- the host checks of ic_codec_decode_window, before anything touches the device.  On success the
// descriptors as the kernel reads them and *lds = the dynamic LDS of the launch: the largest table that is staged.
bool windows_ok(size_t in_words, const ic_window* win, int nwin, int rh, int rw, const long long* spans,
                long long nblocks, const void* rows, long long nsym, int C, size_t pool_words, int nrows, int R,
                std::vector<WinDev>* wins, std::vector<BlockDev>* blocks, size_t* lds) {
  if (nwin < 1 || nwin > 65535 || rh < 1 || rw < 1 || nblocks < 1 || nblocks > 0x7fffffffll || nsym < 1) return false;
  if (C < 1 || nrows < 1 || R < 1 || R > IC_CODEC_MAXR) return false;
  if (!rows && C > nrows) return false;
  const long long per = 64ll * R;
  wins->reserve((size_t)nwin);
  blocks->reserve((size_t)nblocks);
  *lds = 0;
  long long at = 0;
  for (int k = 0; k < nwin; ++k) {
    const ic_window& v = win[k];
    // the segment: below 2^31 symbols, inside rows / mu
    if (v.hy < 1 || v.wy < 1 || (long long)v.hy * v.wy > 0x7fffffffll / C) return false;
    const long long seg_len = (long long)v.hy * v.wy * C;
    if (v.base < 0 || v.base > nsym - seg_len) return false;
    if (!rows && v.base % C) return false;
    // K and the table inside the pool
    if (v.K < 0 || v.K > IC_CODEC_KMAX || v.table < 0 || v.table > 0x7fffffffll) return false;
    const size_t tb = table_bytes(nrows, v.K);
    if ((size_t)v.table + tb / sizeof(uint32_t) > pool_words) return false;
    if (tb <= CODEC_LDS_BYTES) *lds = std::max(*lds, tb);
    // the window inside the segment
    if (v.r0 < 0 || v.c0 < 0 || rh > v.hy || rw > v.wy || v.r0 > v.hy - rh || v.c0 > v.wy - rw) return false;
    // the chunk range inside the segment's chunk count and over the window's rows
    const long long cps = (seg_len + per - 1) / per;
    if (v.k0 < 0 || v.k1 <= v.k0 || v.k1 > cps) return false;
    const long long s0 = (long long)v.r0 * v.wy * C, s1 = (long long)(v.r0 + rh) * v.wy * C;
    if (v.k0 * per > s0 || v.k1 * per < s1) return false;
    if (v.k1 - v.k0 > nblocks - at) return false;
    wins->push_back(WinDev{v.base, v.hy, v.wy, v.K, (int)v.table, v.r0, v.c0, make_fastdiv((uint32_t)v.wy)});
    for (int c = v.k0; c < v.k1; ++c, ++at) {
      const long long b = spans[2 * at], e = spans[2 * at + 1];
      if (b < 0 || e < b || (unsigned long long)e > in_words) return false;   // the spans inside the buffer
      blocks->push_back(BlockDev{b, e, k, c});
    }
  }
  return at == nblocks;
}

}  // namespace

extern "C" {

size_t ic_codec_window_ws(int nwin, long long nblocks) {
  if (nwin < 1 || nwin > 65535 || nblocks < 1 || nblocks > 0x7fffffffll) return 0;
  return (size_t)nwin * sizeof(WinDev) + (size_t)nblocks * sizeof(BlockDev);
}

int ic_codec_decode_window(const void* in, size_t in_bytes, const ic_window* win, int nwin, int rh, int rw,
                           const long long* spans, long long nblocks, const unsigned char* rows, const float* mu,
                           long long nsym, int C, const unsigned int* pool, size_t pool_words, int nrows,
                           int steps_per_chunk, void* ws, size_t ws_bytes, float* out, void* stream) {
  if (!in || !win || !spans || !pool || !ws || !out || ((uintptr_t)in & 1) || ((uintptr_t)ws & 7)) return IC_ERR_ARG;
  std::vector<WinDev> wins;
  std::vector<BlockDev> blocks;
  size_t lds = 0;
  if (!windows_ok(in_bytes / 2, win, nwin, rh, rw, spans, nblocks, rows, nsym, C, pool_words, nrows, steps_per_chunk,
                  &wins, &blocks, &lds))
    return IC_ERR_ARG;
  const size_t wb = wins.size() * sizeof(WinDev), bb = blocks.size() * sizeof(BlockDev);
  if (ws_bytes < wb + bb) return IC_ERR_WORKSPACE;
  // one copy: the windows, then the blocks (sizeof(WinDev) is a multiple of 8, BlockDev's alignment)
  std::vector<unsigned char> host(wb + bb);
  std::copy_n((const unsigned char*)wins.data(), wb, host.begin());
  std::copy_n((const unsigned char*)blocks.data(), bb, host.begin() + wb);
  hipStream_t st = (hipStream_t)stream;
  // the host array is consumed before this returns (a copy from pageable memory is staged by the runtime)
  const hipError_t e = hipMemcpyAsync(ws, host.data(), host.size(), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  const WinArgs a{(const WinDev*)ws, (const BlockDev*)((const unsigned char*)ws + wb), rows, mu, pool, C, nrows,
                  steps_per_chunk, rh, rw, make_fastdiv((uint32_t)C)};
  hipLaunchKernelGGL(codec_decode_window_k, dim3((unsigned)nblocks), dim3(64), lds, st, (const unsigned short*)in,
                     in_bytes / 2, a, out);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_crop_clamp_at(const ic_act* x, int top, int left, int h, int w, float* y, void* stream) {
  if (!x || !x->data || !y || x->n < 1 || x->c < 1 || h < 1 || w < 1 || top < 0 || left < 0) return IC_ERR_ARG;
  if (h > x->h || w > x->w || top > x->h - h || left > x->w - w) return IC_ERR_ARG;
  if (x->sn < 0 || x->sc < 0 || x->sh < 0 || x->sw < 0) return IC_ERR_ARG;
  const long long n = (long long)x->n * x->c * h * w;
  const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(crop_clamp_at_k, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x->data, x->sn,
                     x->sc, x->sh, x->sw, n, x->c, top, left, h, w, y);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
