// h_s, inference: one layer of the hyperprior synthesis per launch (ic_hs_layer), every output by arithmetic that
// does not depend on the batch size, the map size or where the position lies in the map.
//
// A layer is ConvTranspose2d(Cin, Cout, k, stride=s, padding=p=k/2, output_padding=s-1, bias) on dense channels-last
// fp32 storage x (n, a, b, c) of N x H x W x Cin; the output is (n, i, j, o) of N x sH x sW x Cout.  With the weight
// (Cin, Cout, k, k) as the module holds it:
//     out[n,o,i,j] = b[o] + sum_(ky,kx) sum_c w[c,o,ky,kx] * x[n,c,(i+p-ky)/s,(j+p-kx)/s]
// over the taps for which both quotients are exact (the live taps of the output's phase (i % s, j % s)); a neighbour
// outside the map contributes a product with +0.0.
//
// Arithmetic: exact fp32 products, fp32 accumulation, whatever the model's COMPUTE_DTYPE is
// (v_mfma_f32_32x32x2_f32: each accumulator is one chain of fmaf, starting from the bias).
// THE ORDER of every accumulator is a function of (k, s, Cin) only: the live taps of its phase in ascending (ky, kx);
// inside a tap the channel groups of 8 in ascending order; inside a group the channels c0+0, c0+4, c0+1, c0+5, c0+2,
// c0+6, c0+3, c0+7 (one MFMA sums channel c0+e of lane half 0, then c0+4+e of lane half 1).  Channels past Cin and
// taps outside the map add a product of +0.0 with 0 or the weight.  K is not split, there is no atomic and nothing is
// reduced across waves or blocks, so N, H and W enter only as the number of tiles: image n's outputs are bit for
// bit the same in any batch, and an output whose taps see the same values sees the same bits in any map (a crop).
//
// Tile map.  The positions of ONE phase of ONE image are numbered q = a W + b (ascending (i, j), i = pi + s a,
// j = pj + s b) and cut into tiles of 32; a block never holds positions of two images or two phases.  The work of a
// tile is heads * ceil(Cout / 32) units, one per head and 32 output channels; one wave computes one unit, a 32 x 32
// accumulator, four waves share a block and so the tile's inputs in L1.  Grid: x = phases x tiles x
// ceil(units / 4), y = image (looping past 65,535).
//
// Epilogue, per head: none; ReLU (relu_fwd_k's expression); expf then clamp to [lo, hi] (exp_clamp_fwd_k's).
// Second head: other weights, bias, output and epilogue on the same input, in the same launch.
//
// Weights: repacked (pack_k) to [head][phase, tap][channel group of 8][output, padded to 32][8 channels], so a
// wave's B fragment of four k-steps is one 16-byte load per lane.  The pack lives in a caller-owned workspace of
// ic_hs_ws(Cin, Cout, k, s, heads) bytes; with `packed` != 0 the workspace already holds it and only the layer
// kernel is launched (the eval weight cache).  Padded slots of the pack are never used: a select drops them.
#include <algorithm>
#include <cstdint>
#include <initializer_list>

#include "common.h"
#include "../../include/imgcomp.h"

namespace {

constexpr int HS_THREADS = 256;   // four waves: four units of one tile
constexpr int HS_U = 2;           // channel groups (of 8) of one stage: 8 MFMAs
constexpr int HS_D = 6;           // stages in flight

// the live taps of one axis for outputs of residue r: ky = first, first + s, ... below k
__host__ __device__ __forceinline__ int axis_first(int s, int p, int r) { return (r + p) % s; }
__host__ __device__ __forceinline__ int axis_count(int k, int s, int p, int r) {
  const int f = axis_first(s, p, r);
  return f < k ? (k - 1 - f) / s + 1 : 0;
}
// taps of the phases in front of phase ph = pi s + pj, in the pack's order
__host__ __device__ __forceinline__ int phase_base(int k, int s, int p, int ph) {
  int base = 0;
  for (int q = 0; q < ph; ++q) base += axis_count(k, s, p, q / s) * axis_count(k, s, p, q % s);
  return base;
}

struct HsGeo {
  long long H, W, HW;       // the input map
  int Cin, Cout, k, s, p;
  int KG, NT, UB, units;    // channel groups of 8, output tiles of 32, blocks per tile, units per tile
  int heads;
  long long tiles;          // per phase
  int epi[2];
  float lo, hi;
};

struct HsTaps {
  int src[25];              // pack tap T -> ky k + kx
};

// packed[head][T][kg][o][e] = w_head[8 kg + e][o][tap T], 0 where o >= Cout or 8 kg + e >= Cin
__global__ void __launch_bounds__(HS_THREADS) pack_k(const float* __restrict__ w0, const float* __restrict__ w1,
                                                     HsTaps taps, long long Cin, long long Cout, long long KK,
                                                     long long KG, long long OP, long long total,
                                                     float* __restrict__ packed) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int e = (int)(idx & 7);
    long long rest = idx >> 3;
    const long long o = rest % OP;
    rest /= OP;
    const long long kg = rest % KG;
    rest /= KG;
    const int T = (int)(rest % KK);
    const int head = (int)(rest / KK);
    const long long c = 8 * kg + e;
    int src = 0;
#pragma unroll
    for (int t = 0; t < 25; ++t) src = t == T ? taps.src[t] : src;
    float v = 0.0f;
    if (o < Cout && c < Cin) v = (head ? w1 : w0)[(c * Cout + o) * KK + src];
    packed[idx] = v;
  }
}

struct HsFrag {
  floatx4v x[HS_U], b[HS_U];
};

// Where a stream of stages stands: tap t of the phase, stage kb of the tap, and for this lane's row whether the
// tap's neighbour lies inside the map and the element offset to read it at (the row's own position when it does
// not: a valid address whose value is dropped).
struct HsCursor {
  int t, kb;
  bool inb;
  long long at;
};

// One unit of one image: the 32 x 32 accumulator of (phase, tile, head, 32 output channels) over all of K, walked in
// stages of HS_U channel groups of one tap; the loads of HS_D stages are in flight while one is consumed.  Every load
// is unconditional and in bounds; what is not used is dropped by a select where it is used.
template <bool VEC>
__device__ __forceinline__ floatx16 unit_gemm(const float* __restrict__ xn, const float* __restrict__ wp,
                                              const HsGeo& geo, long long q, int pi, int pj, int ntaps, int ntx,
                                              int tbase, int g, int steps, int KB, float bias) {
  const long long H = geo.H, W = geo.W;
  const int C = geo.Cin, KG = geo.KG, s = geo.s, p = geo.p;
  const int OP8 = 32 * geo.NT * 8;   // floats of one (tap, channel group) of the pack: 25 * 512 * OP8 < 2^31
  const bool valid = q < geo.HW;
  const long long qa = valid ? q / W : 0, qb = valid ? q - qa * W : 0;
  const long long own = valid ? q * C : 0;
  const float* __restrict__ wg = wp + 4 * g;
  const int cg = 4 * g;
  const int ky0 = axis_first(s, p, pi), kx0 = axis_first(s, p, pj);

  auto enter = [&](HsCursor& c, int t) {
    c.t = t;
    c.kb = 0;
    const int ty = t / ntx, tx = t - ty * ntx;
    const int dy = (pi + p - (ky0 + s * ty)) / s, dx = (pj + p - (kx0 + s * tx)) / s;   // exact quotients
    const long long ni = qa + dy, nj = qb + dx;
    c.inb = valid && ni >= 0 && ni < H && nj >= 0 && nj < W;
    c.at = c.inb ? (ni * W + nj) * C : own;
  };
  auto advance = [&](HsCursor& c) {   // past the last stage: stays there
    if (c.kb + 1 < KB)
      ++c.kb;
    else if (c.t + 1 < ntaps)
      enter(c, c.t + 1);
  };
  auto load = [&](const HsCursor& c, HsFrag& f) {
    const float* __restrict__ xp = xn + c.at;
#pragma unroll
    for (int u = 0; u < HS_U; ++u) {
      const int kg = min(c.kb * HS_U + u, KG - 1);
      const int c0 = 8 * kg + cg;
      if constexpr (VEC) {   // Cin % 4 == 0: four channels exist together; past Cin the last four, dropped at use
        const int ch = c0 < C ? c0 : C - 4;
        f.x[u] = *reinterpret_cast<const floatx4v*>(xp + ch);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ch = c0 + e < C ? c0 + e : C - 1;
          f.x[u][e] = xp[ch];
        }
      }
      f.b[u] = *reinterpret_cast<const floatx4v*>(wg + ((tbase + c.t) * KG + kg) * OP8);
    }
  };

  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = bias;

  auto use = [&](const HsCursor& c, const HsFrag& f) {
#pragma unroll
    for (int u = 0; u < HS_U; ++u) {
      const int kg = c.kb * HS_U + u;
      const bool group = kg < KG;   // a group past the last one (KG not a multiple of HS_U) adds 0 * 0
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool chan = group && 8 * kg + cg + e < C;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(c.inb && chan ? f.x[u][e] : 0.0f, chan ? f.b[u][e] : 0.0f, acc, 0,
                                                   0, 0);
      }
    }
  };

  HsFrag buf[HS_D];
  HsCursor lc, uc;   // the stage being loaded runs HS_D ahead of the stage being used
  enter(lc, 0);
  enter(uc, 0);
#pragma unroll
  for (int d = 0; d < HS_D; ++d) {
    load(lc, buf[d]);
    advance(lc);
  }
  for (int base = 0; base < steps; base += HS_D) {
#pragma unroll
    for (int d = 0; d < HS_D; ++d) {
      if (base + d < steps) use(uc, buf[d]);   // wave-uniform
      advance(uc);
      load(lc, buf[d]);   // past the end: the last stage again, never used
      advance(lc);
    }
  }
  return acc;
}

__device__ __forceinline__ float epilogue(float v, int epi, float lo, float hi) {
  if (epi == IC_HS_RELU) return v > 0.f ? v : (v != v ? v : 0.f);
  if (epi == IC_HS_EXP_CLAMP) return fminf(fmaxf(expf(v), lo), hi);
  return v;
}

template <bool VEC>
__global__ void __launch_bounds__(HS_THREADS) layer_k(const float* __restrict__ x, const float* __restrict__ packed,
                                                      const float* __restrict__ b0, const float* __restrict__ b1,
                                                      int N, HsGeo geo, float* __restrict__ out0,
                                                      float* __restrict__ out1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, g = lane >> 5;
  const long long blk = blockIdx.x;
  const int ub = (int)(blk % geo.UB);
  const long long pt = blk / geo.UB;
  const long long tile = pt % geo.tiles;
  const int ph = (int)(pt / geo.tiles);
  const int unit = ub * 4 + wave;
  if (unit >= geo.units) return;   // no barrier below: a wave without a unit just leaves
  const int head = unit / geo.NT, nt = unit % geo.NT;
  const int s = geo.s, p = geo.p, k = geo.k;
  const int pi = ph / s, pj = ph % s;
  const int nty = axis_count(k, s, p, pi), ntx = axis_count(k, s, p, pj);
  const int ntaps = nty * ntx;
  const int tbase = phase_base(k, s, p, ph);
  const long long W = geo.W, Cout = geo.Cout;
  const long long o = 32ll * nt + r;   // this lane's output channel: B's column, the accumulators' column

  const long long q = tile * 32 + r;   // row r of the tile
  const bool valid = q < geo.HW;
  const long long qa = valid ? q / W : 0, qb = valid ? q - qa * W : 0;
  // the row's output position (i sW + j), -1 past the end of the phase
  const long long opos = valid ? (pi + s * qa) * (s * W) + (pj + s * qb) : -1;

  const float bias = o < Cout ? (head ? b1 : b0)[o] : 0.0f;
  const int KB = (geo.KG + HS_U - 1) / HS_U;
  const int steps = ntaps * KB;   // 0: a phase without a live tap (k < s) is the bias alone
  const float* __restrict__ wp =
      packed + (long long)head * k * k * geo.KG * (32ll * geo.NT * 8) + o * 8;
  const int epi = geo.epi[head];
  float* __restrict__ outh = head ? out1 : out0;
  const long long in_img = geo.HW * geo.Cin, out_img = geo.HW * s * s * Cout;

  for (long long n = blockIdx.y; n < N; n += gridDim.y) {
    floatx16 acc;
    if (steps == 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[v] = bias;
    } else {
      acc = unit_gemm<VEC>(x + n * in_img, wp, geo, q, pi, pj, ntaps, ntx, tbase, g, steps, KB, bias);
    }
    float* __restrict__ out = outh + n * out_img;
    // accumulator v of this lane is row (v & 3) + 8 (v >> 2) + 4 g of the tile, column o
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const long long po = __shfl(opos, (v & 3) + 8 * (v >> 2) + 4 * g);
      if (po >= 0 && o < Cout) out[po * Cout + o] = epilogue(acc[v], epi, geo.lo, geo.hi);
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// N H W C as one element count; 0: a size below 1 or a product past 2^63 - 1
long long checked_count(long long N, long long H, long long W, long long C) {
  if (N < 1 || H < 1 || W < 1 || C < 1) return 0;
  const long long lim = 0x7fffffffffffffffll;
  if (N > lim / H) return 0;
  const long long a = N * H;
  if (W > lim / C) return 0;
  const long long b = W * C;
  if (a > lim / b) return 0;
  return a * b;
}

bool served(int Cin, int Cout, int k, int s, int heads) {
  return Cin >= 1 && Cin <= IC_HS_MAXC && Cout >= 1 && Cout <= IC_HS_MAXC && k >= 1 && k <= 5 && (k & 1) &&
         (s == 1 || s == 2) && (heads == 1 || heads == 2);
}

long long pack_floats(int Cin, int Cout, int k, int heads) {
  const long long KG = ((long long)Cin + 7) / 8, OP = ((long long)Cout + 31) / 32 * 32;
  return (long long)heads * k * k * KG * OP * 8;
}

// a buffer as [base, base + bytes); empty when bytes is 0
struct Span {
  const void* base;
  long long bytes;
};
long long float_bytes(long long n) { return n > 0x7fffffffffffffffll / 4 ? 0x7fffffffffffffffll : 4 * n; }
bool overlap(const Span& a, const Span& b) {
  if (!a.base || !b.base || a.bytes <= 0 || b.bytes <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a.base, b0 = (uintptr_t)b.base;
  return a0 < b0 ? (uintptr_t)a.bytes > b0 - a0 : (uintptr_t)b.bytes > a0 - b0;
}

bool epi_ok(int e) { return e == IC_HS_NONE || e == IC_HS_RELU || e == IC_HS_EXP_CLAMP; }

}  // namespace

extern "C" {

size_t ic_hs_ws(int Cin, int Cout, int k, int s, int heads) {
  if (!served(Cin, Cout, k, s, heads)) return 0;
  return (size_t)pack_floats(Cin, Cout, k, heads) * sizeof(float);
}

int ic_hs_layer(const float* x, int N, int H, int W, int Cin, int Cout, int k, int s, const float* w, const float* b,
                int epilogue, float* out, const float* w2, const float* b2, int epilogue2, float* out2, float lo,
                float hi, void* ws, size_t ws_bytes, int packed, void* stream) {
  if (!x || !w || !b || !out || !ws) return IC_ERR_ARG;
  const bool second = w2 || b2 || out2;
  if (second && (!w2 || !b2 || !out2)) return IC_ERR_ARG;
  const int heads = second ? 2 : 1;
  if (!served(Cin, Cout, k, s, heads)) return IC_ERR_ARG;
  if (!epi_ok(epilogue) || (second && !epi_ok(epilogue2))) return IC_ERR_ARG;
  const long long n_in = checked_count(N, H, W, Cin);
  const long long n_out = checked_count(N, (long long)s * H, (long long)s * W, Cout);
  if (n_in == 0 || n_out == 0) return IC_ERR_ARG;
  // blocks read their neighbours' inputs while others write: no byte of an output may lie in an input, the
  // workspace or the other output
  const size_t need = ic_hs_ws(Cin, Cout, k, s, heads);
  const long long kk = (long long)Cin * Cout * k * k;
  const Span outs[2] = {{out, float_bytes(n_out)}, {out2, second ? float_bytes(n_out) : 0}};
  const Span ins[6] = {{x, float_bytes(n_in)}, {w, kk * 4}, {b, Cout * 4ll}, {w2, second ? kk * 4 : 0},
                       {b2, second ? Cout * 4ll : 0}, {ws, (long long)need}};
  for (const Span& o : outs)
    for (const Span& in : ins)
      if (overlap(o, in)) return IC_ERR_ARG;
  if (overlap(outs[0], outs[1])) return IC_ERR_ARG;
  if (!aligned16(ws)) return IC_ERR_ARG;
  if (ws_bytes < need) return IC_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;

  HsGeo geo;
  geo.H = H;
  geo.W = W;
  geo.HW = (long long)H * W;
  geo.Cin = Cin;
  geo.Cout = Cout;
  geo.k = k;
  geo.s = s;
  geo.p = k / 2;
  geo.KG = (Cin + 7) / 8;
  geo.NT = (Cout + 31) / 32;
  geo.heads = heads;
  geo.units = heads * geo.NT;
  geo.UB = (geo.units + 3) / 4;
  geo.tiles = (geo.HW + 31) / 32;
  geo.epi[0] = epilogue;
  geo.epi[1] = second ? epilogue2 : IC_HS_NONE;
  geo.lo = lo;
  geo.hi = hi;
  const long long phases = (long long)s * s;
  if (geo.tiles > 0x7fffffffll / (phases * geo.UB)) return IC_ERR_ARG;

  if (!packed) {
    HsTaps taps;
    int T = 0;
    for (int ph = 0; ph < s * s; ++ph)
      for (int ky = axis_first(s, geo.p, ph / s); ky < k; ky += s)
        for (int kx = axis_first(s, geo.p, ph % s); kx < k; kx += s) taps.src[T++] = ky * k + kx;
    for (; T < 25; ++T) taps.src[T] = 0;
    const long long total = pack_floats(Cin, Cout, k, heads);
    const int blocks = (int)std::min<long long>((total + HS_THREADS - 1) / HS_THREADS, 4096);
    hipLaunchKernelGGL(pack_k, dim3(blocks), dim3(HS_THREADS), 0, st, w, second ? w2 : w, taps, (long long)Cin,
                       (long long)Cout, (long long)k * k, (long long)geo.KG, 32ll * geo.NT, total, (float*)ws);
    IC_CHECK_LAUNCH();
  }
  const dim3 grid((unsigned)(phases * geo.tiles * geo.UB), (unsigned)std::min(N, 65535));
  const bool vec = Cin % 4 == 0 && aligned16(x);
  if (vec)
    hipLaunchKernelGGL(layer_k<true>, grid, dim3(HS_THREADS), 0, st, x, (const float*)ws, b, second ? b2 : b, N, geo,
                       out, second ? out2 : out);
  else
    hipLaunchKernelGGL(layer_k<false>, grid, dim3(HS_THREADS), 0, st, x, (const float*)ws, b, second ? b2 : b, N, geo,
                       out, second ? out2 : out);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // extern "C"
