// The decoder of one rANS chunk, shared by the kernels that decode whole tensors (codec.hip) and the one that
// decodes a window of a latent (window.hip): the table staging, the row rule and the mirror of encode_chunk.
// The bitstream is specified in image_compression_amd/codec.py.
#pragma once
#include "common.h"
#include "../../include/imgcomp.h"

namespace {

constexpr uint32_t RANS_L = 1u << 16;                // lower bound of the state interval
constexpr size_t CODEC_LDS_BYTES = 49152;            // tables up to this size are staged in LDS

__host__ __device__ inline size_t table_bytes(int nrows, int K) { return (size_t)nrows * (2 * K + 2) * sizeof(uint32_t); }

struct CodecArgs {
  long long n;                 // symbols of the tensor
  const unsigned char* rows;   // per-symbol table row, or null: row = global index % C
  int C;
  const uint32_t* cdf;         // [nrows][M + 1]
  int nrows, K, R;
};

// the tables in LDS (LDS = true) or where they are
template <bool LDS>
__device__ __forceinline__ const uint32_t* stage_tables(const CodecArgs& a, uint32_t* lds) {
  if (!LDS) return a.cdf;
  const int words = a.nrows * (2 * a.K + 2);
  for (int j = threadIdx.x; j < words; j += 64) lds[j] = a.cdf[j];
  __syncthreads();
  return lds;
}

__device__ __forceinline__ int row_of(const CodecArgs& a, long long g) {
  const int r = a.rows ? (int)a.rows[g] : (int)(g % a.C);
  return min(r, a.nrows - 1);
}

// The mirror of encode_chunk (codec.hip).  Every read of `in` is guarded by the chunk's [begin, end); the search
// stays inside the symbol's row.  The chunk holds the nc symbols from global index c0 on; a.cdf is the table of
// those symbols.  store(g, q) receives every symbol q = j - K with its global index g, once.
template <bool LDS, class Store>
__device__ __forceinline__ void decode_chunk(const unsigned short* __restrict__ in, size_t begin, size_t end,
                                             const CodecArgs& a, long long c0, int nc, Store store, uint32_t* lds) {
  const uint32_t* tab = stage_tables<LDS>(a, lds);
  const int lane = threadIdx.x;
  auto word = [&](size_t w) -> uint32_t { return w < end ? (uint32_t)in[w] : 0u; };

  const int M = 2 * a.K + 1, M1 = M + 1;
  int iters = 0;
  while ((1 << iters) < M) ++iters;
  const int steps = (nc + 63) >> 6;
  uint32_t x = word(begin + 2 * lane) | (word(begin + 2 * lane + 1) << 16);
  size_t cur = begin + 128;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int t = 0; t < steps; ++t) {
    const int i = t * 64 + lane;
    const bool active = i < nc;
    bool refill = false;
    if (active) {
      const long long g = c0 + i;
      const uint32_t* row = tab + (size_t)row_of(a, g) * M1;
      const uint32_t slot = x & 0xffffu;
      int lo = 0, hi = M - 1;  // largest j in [0, M-1] with row[j] <= slot (row[0] = 0)
      for (int it = 0; it < iters; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (row[mid] <= slot) lo = mid; else hi = mid - 1;
      }
      const uint32_t start = row[lo], freq = row[lo + 1] - start;
      x = freq * (x >> 16) + slot - start;
      refill = x < RANS_L;
      store(g, lo - a.K);
    }
    const unsigned long long mask = __ballot(refill);
    if (refill) x = (x << 16) | word(cur + __popcll(mask & below));
    cur += __popcll(mask);
  }
}

}  // namespace
