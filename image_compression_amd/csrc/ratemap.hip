// Rate and distortion maps: the estimated bits and the squared error of every block of 2^shift x 2^shift positions
// (ic_block_bits, ic_block_sse), from tensors the eval forward already holds.  Inference only.
//   * One HIP block per map block (n, bi, bj), RM_THREADS threads, one launch, no workspace, no atomics.
//   * A map block is a set of runs, each contiguous in storage: with channels-last storage one run per row of the
//     block ((j1 - j0) C elements), with NCHW storage one run per (channel, row) (j1 - j0 elements).  A run is cut
//     into quads of 4 elements counted from its start; thread t takes the quads t, t + RM_THREADS, ... of the block
//     in (run, quad) order and adds their terms one by one, elements ascending; then block_sum (common.h).
//   * The order is therefore a function of (C, Hm, Wm, shift, layout) alone: it does not depend on N, on n, on the
//     run, or on how a quad was loaded.  A full quad whose address is 16-byte aligned is one 16-byte load, any other
//     quad up to four 4-byte loads; the arithmetic after the loads is the same code for both.
//   * out = add + s is one fp32 addition (__fadd_rn), the last operation.
#include <algorithm>

#include "bits_term.h"
#include "common.h"
#include "fp_rn.h"
#include "../../include/imgcomp.h"

namespace {

constexpr int RM_THREADS = 256;
constexpr int RM_MAXBLOCKS = 1 << 20;   // HIP blocks per image; a larger map is walked grid-stride

// One image's logical (C, Hm, Wm) elements in one of the two storage orders
struct MapWalk {
  long long sn, sc, sh, sw;   // element strides; (sc, sh, sw) are the layout's own: (1, Wm C, C) or (Hm Wm, Wm, 1)
  int Hm, Wm, C, cl, shift, nbh, nbw;
  FastDiv by_nbw, by_c;
  FastDiv quads_in, quads_edge;   // by the quads of a run: a block inside the map, a block of the last column
  FastDiv rows_in, rows_edge;     // by the rows of a block: inside the map, of the last row
};

struct MapBlock {
  int i0, j0, rows, cols, len, quads;   // len: elements of a run
  uint32_t total;                       // quads of the block
  FastDiv by_quads, by_rows;
};

__device__ __forceinline__ MapBlock block_of(const MapWalk& g, uint32_t blk) {
  MapBlock b;
  const uint32_t bi = fdiv(blk, g.by_nbw), bj = blk - bi * g.nbw;
  const int side = 1 << g.shift;
  b.i0 = (int)bi << g.shift, b.j0 = (int)bj << g.shift;
  b.rows = min(g.Hm - b.i0, side), b.cols = min(g.Wm - b.j0, side);
  b.len = g.cl ? b.cols * g.C : b.cols;
  b.quads = (b.len + 3) >> 2;
  b.by_quads = (int)bj == g.nbw - 1 ? g.quads_edge : g.quads_in;
  b.by_rows = (int)bi == g.nbh - 1 ? g.rows_edge : g.rows_in;
  b.total = (uint32_t)(g.cl ? 1 : g.C) * b.rows * b.quads;   // <= C Hm Wm < 2^31
  return b;
}

// quad `qid` of a block: the offset of its first element in the image, how many elements it holds (1 .. 4), and the
// (channel, row, column) of the first
struct Quad {
  long long off;
  int cnt, c, i, j;
};

template <bool WHERE>
__device__ __forceinline__ Quad quad_of(const MapWalk& g, const MapBlock& b, uint32_t qid) {
  Quad q;
  const uint32_t run = fdiv(qid, b.by_quads), k = qid - run * b.quads;
  const uint32_t ch = fdiv(run, b.by_rows), row = run - ch * b.rows;   // channels last: ch == 0
  const int e = (int)k * 4;
  q.cnt = min(4, b.len - e);
  q.i = b.i0 + (int)row;
  q.off = (long long)ch * g.sc + (long long)q.i * g.sh + (long long)b.j0 * g.sw + e;
  if (WHERE) {
    if (g.cl) {
      const uint32_t w = fdiv((uint32_t)e, g.by_c);
      q.c = e - (int)w * g.C, q.j = b.j0 + (int)w;
    } else {
      q.c = (int)ch, q.j = b.j0 + e;
    }
  }
  return q;
}

// v[0 .. cnt) = the quad's elements
__device__ __forceinline__ void load_quad(const float* __restrict__ p, int cnt, float (&v)[4]) {
  if (cnt == 4 && ((uintptr_t)p & 15) == 0) {
    const floatx4v t = *reinterpret_cast<const floatx4v*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = t[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < cnt ? p[k] : 0.0f;
  }
}

__global__ void __launch_bounds__(RM_THREADS) block_bits_k(const float* __restrict__ p, MapWalk g,
                                                           const float* __restrict__ add, float* __restrict__ out) {
  __shared__ float lds[16];
  const float* ps = p + (long long)blockIdx.y * g.sn;
  const uint32_t nblk = (uint32_t)g.nbh * g.nbw;
  for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const MapBlock b = block_of(g, blk);
    float s[1] = {0.0f};
    for (uint32_t qid = threadIdx.x; qid < b.total; qid += RM_THREADS) {
      const Quad q = quad_of<false>(g, b, qid);
      float v[4];
      load_quad(ps + q.off, q.cnt, v);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < q.cnt) s[0] += ic_bits_term(v[k]);
    }
    block_sum<1>(s, lds);
    if (threadIdx.x == 0) {
      const long long at = (long long)blockIdx.y * nblk + blk;
      out[at] = add ? __fadd_rn(add[at], s[0]) : s[0];
    }
  }
}

// a is walked along its storage; SAME: b has a's strides inside an image, otherwise b is read element by element
// at its own strides
template <bool SAME>
__global__ void __launch_bounds__(RM_THREADS) block_sse_k(const float* __restrict__ a, const float* __restrict__ b,
                                                          MapWalk g, long long bn, long long bc, long long bh,
                                                          long long bw, float* __restrict__ out) {
  __shared__ float lds[16];
  const float* as = a + (long long)blockIdx.y * g.sn;
  const float* bs = b + (long long)blockIdx.y * bn;
  const uint32_t nblk = (uint32_t)g.nbh * g.nbw;
  for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const MapBlock mb = block_of(g, blk);
    float s[1] = {0.0f};
    for (uint32_t qid = threadIdx.x; qid < mb.total; qid += RM_THREADS) {
      const Quad q = quad_of<!SAME>(g, mb, qid);
      float va[4], vb[4];
      load_quad(as + q.off, q.cnt, va);
      if (SAME) {
        load_quad(bs + q.off, q.cnt, vb);
      } else {
        int c = q.c, j = q.j;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          vb[k] = k < q.cnt ? bs[c * bc + q.i * bh + j * bw] : 0.0f;
          if (g.cl) {
            if (++c == g.C) c = 0, ++j;
          } else {
            ++j;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = sub_rn(va[k], vb[k]);
        if (k < q.cnt) s[0] = fmaf(d, d, s[0]);   // the difference rounded once, the square fused with the sum
      }
    }
    block_sum<1>(s, lds);
    if (threadIdx.x == 0) out[(long long)blockIdx.y * nblk + blk] = s[0];
  }
}

// ---- the host checks, before any launch
int map_extent(int v, int shift) { return (int)(((long long)v + (1 << shift) - 1) >> shift); }

// 1: channels-last storage (c fastest), 0: NCHW-dense, -1: neither.  The stride of an extent of 1 is not looked at
int layout_of(int C, int H, int W, long long sc, long long sh, long long sw) {
  if ((C == 1 || sc == 1) && (W == 1 || sw == C) && (H == 1 || sh == (long long)W * C)) return 1;
  if ((W == 1 || sw == 1) && (H == 1 || sh == W) && (C == 1 || sc == (long long)H * W)) return 0;
  return -1;
}

bool shape_ok(int N, int C, int H, int W, long long sn, int shift) {
  if (N < 1 || N > 65535 || C < 1 || H < 1 || W < 1 || sn < 0 || shift < 0 || shift > 6) return false;
  return (long long)C * H <= 0x7fffffffll / W;   // one image's elements are indexed in 32 bits
}

MapWalk make_walk(int C, int H, int W, long long sn, int cl, int shift) {
  MapWalk g;
  g.sn = sn;
  g.sc = cl ? 1 : (long long)H * W, g.sh = cl ? (long long)W * C : W, g.sw = cl ? C : 1;
  g.Hm = H, g.Wm = W, g.C = C, g.cl = cl, g.shift = shift;
  g.nbh = map_extent(H, shift), g.nbw = map_extent(W, shift);
  g.by_nbw = make_fastdiv((uint32_t)g.nbw);
  g.by_c = make_fastdiv((uint32_t)C);
  const int side = 1 << shift, per = cl ? C : 1;
  const int cols_in = std::min(side, W), cols_edge = W - ((g.nbw - 1) << shift);
  g.quads_in = make_fastdiv((uint32_t)((cols_in * per + 3) >> 2));
  g.quads_edge = make_fastdiv((uint32_t)((cols_edge * per + 3) >> 2));
  g.rows_in = make_fastdiv((uint32_t)std::min(side, H));
  g.rows_edge = make_fastdiv((uint32_t)(H - ((g.nbh - 1) << shift)));
  return g;
}

dim3 map_grid(const MapWalk& g, int N) {
  return dim3((unsigned)std::min<long long>((long long)g.nbh * g.nbw, RM_MAXBLOCKS), (unsigned)N);
}

}  // namespace

extern "C" {

int ic_block_bits(const float* p, int N, int C, int Hm, int Wm, long long sn, long long sc, long long sh, long long sw,
                  int shift, const float* add, float* out, void* stream) {
  if (!p || !out || !shape_ok(N, C, Hm, Wm, sn, shift)) return IC_ERR_ARG;
  const int cl = layout_of(C, Hm, Wm, sc, sh, sw);
  if (cl < 0) return IC_ERR_ARG;
  const MapWalk g = make_walk(C, Hm, Wm, sn, cl, shift);
  hipLaunchKernelGGL(block_bits_k, map_grid(g, N), dim3(RM_THREADS), 0, (hipStream_t)stream, p, g, add, out);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_block_sse(const float* a, const float* b, int N, int C, int H, int W, long long an, long long ac, long long ah,
                 long long aw, long long bn, long long bc, long long bh, long long bw, int shift, float* out,
                 void* stream) {
  if (!a || !b || !out || !shape_ok(N, C, H, W, an, shift) || bn < 0) return IC_ERR_ARG;
  const int cl = layout_of(C, H, W, ac, ah, aw), clb = layout_of(C, H, W, bc, bh, bw);
  if (cl < 0 || clb < 0) return IC_ERR_ARG;
  const MapWalk g = make_walk(C, H, W, an, cl, shift);
  // an extent of 1 makes a tensor both layouts: b shares a's walk whenever it can be read at a's strides
  const bool same = (C == 1 || bc == g.sc) && (H == 1 || bh == g.sh) && (W == 1 || bw == g.sw);
  if (same) {
    hipLaunchKernelGGL(block_sse_k<true>, map_grid(g, N), dim3(RM_THREADS), 0, (hipStream_t)stream, a, b, g, bn, 0LL, 0LL,
                       0LL, out);
  } else {
    const MapWalk gb = make_walk(C, H, W, bn, clb, shift);   // b's own strides, those of its layout
    hipLaunchKernelGGL(block_sse_k<false>, map_grid(g, N), dim3(RM_THREADS), 0, (hipStream_t)stream, a, b, g, bn, gb.sc,
                       gb.sh, gb.sw, out);
  }
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
