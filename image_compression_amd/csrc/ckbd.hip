// Checkerboard context model (He et al. 2021): the elementwise ops that know which latent positions are anchors
// (ic_ckbd_*).  A tensor is dense channels-last storage (n, i, j, c) of N x H x W x C elements; position (i, j) is an
// anchor when i + j is even, whatever n and c are.  Parity 0 names the anchors, parity 1 the rest.
//   * ic_ckbd_input_*: the context convs' inputs u (the anchors' values) and v (their residual magnitudes
//     |y - mu|, one fp32 subtraction), +0.0 at every non-anchor;
//   * ic_ckbd_params_*: mu = mu_h + a and sigma = sigma_h * expf(clamp(b, -IC_CKBD_LOG_SCALE_LIMIT, +...)) at the
//     non-anchors, mu_h and sigma_h bit for bit at the anchors;
//   * ic_ckbd_gather / ic_ckbd_scatter: the elements at the positions of one parity, packed in ascending
//     (n, i, j, c) order (the order the two bitstreams of y are coded in), and back.
// All kernels are grid-stride and HBM-bound: 16-byte accesses when every pointer is 16-byte aligned and a
// position's C elements are whole 16-byte groups (four floats of a group then share one position), scalar
// otherwise.  The flat index is 64-bit; below 2^31 elements the position of an index is found with 32-bit
// multiply-shift divisions (common.h FastDiv), above with 64-bit ones.  Any H, W >= 1: with an odd W the
// number of positions of one parity alternates from row to row.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "../../include/imgcomp.h"

namespace {

constexpr int CK_THREADS = 256;
constexpr int CK_MAXBLOCKS = 1024;
constexpr float CK_LIM = IC_CKBD_LOG_SCALE_LIMIT;

struct alignas(16) bytes16 {
  uint32_t w[4];
};

// floor(n / d): index type uint32_t for numerators below 2^31, long long beyond
template <typename I>
struct Divider;
template <>
struct Divider<uint32_t> {
  FastDiv f;
  explicit Divider(long long d) : f(make_fastdiv((uint32_t)d)) {}
  __device__ __forceinline__ uint32_t operator()(uint32_t n) const { return fdiv(n, f); }
};
template <>
struct Divider<long long> {
  long long d;
  explicit Divider(long long d_) : d(d_ ? d_ : 1) {}
  __device__ __forceinline__ long long operator()(long long n) const { return n / d; }
};

// One tensor's geometry in units (a unit: one element, or on the vector paths one 16-byte group of one position)
template <typename I>
struct Geo {
  Divider<I> byC, byW, byH, byCnt;
  I C, W, H, cnt, first;   // C: units per position; cnt: positions of the parity in one map; first: those in an even row
  Geo(long long C_, long long W_, long long H_, long long cnt_, long long first_)
      : byC(C_), byW(W_), byH(H_), byCnt(cnt_), C((I)C_), W((I)W_), H((I)H_), cnt((I)cnt_), first((I)first_) {}
};

template <typename I>
__device__ __forceinline__ bool is_anchor(I unit, const Geo<I>& g) {
  const I p = g.byC(unit);
  const I row = g.byW(p);
  const I j = p - row * g.W;
  const I i = row - g.byH(row) * g.H;
  return ((i + j) & 1) == 0;
}

// unit `u` of the packed half of parity `par` -> its unit in the full tensor.  Two consecutive rows hold W positions
// of the parity between them: `first` in the even row (columns par, par + 2, ...), W - first in the odd one.
template <typename I>
__device__ __forceinline__ I full_unit(I u, int par, const Geo<I>& g) {
  const I ph = g.byC(u);
  const I c = u - ph * g.C;
  const I n = g.byCnt(ph);
  const I k = ph - n * g.cnt;
  const I pair = g.byW(k);
  const I rem = k - pair * g.W;
  const bool odd = rem >= g.first;
  const I i = 2 * pair + (odd ? 1 : 0);
  const I j = odd ? (I)(1 - par) + 2 * (rem - g.first) : (I)par + 2 * rem;
  return ((n * g.H + i) * g.W + j) * g.C + c;
}

template <bool VEC>
struct Vf {
  float e[VEC ? 4 : 1];
};
template <bool VEC, typename I>
__device__ __forceinline__ Vf<VEC> ld(const float* __restrict__ p, I unit) {
  Vf<VEC> r;
  if constexpr (VEC) {
    const floatx4v t = reinterpret_cast<const floatx4v*>(p)[unit];
#pragma unroll
    for (int k = 0; k < 4; ++k) r.e[k] = t[k];
  } else {
    r.e[0] = p[unit];
  }
  return r;
}
template <bool VEC, typename I>
__device__ __forceinline__ void st(float* __restrict__ p, I unit, const Vf<VEC>& v) {
  if constexpr (VEC) {
    floatx4v t;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = v.e[k];
    reinterpret_cast<floatx4v*>(p)[unit] = t;
  } else {
    p[unit] = v.e[0];
  }
}
template <bool VEC>
__device__ __forceinline__ Vf<VEC> zeros() {
  Vf<VEC> r;
#pragma unroll
  for (int k = 0; k < (VEC ? 4 : 1); ++k) r.e[k] = 0.0f;
  return r;
}

__device__ __forceinline__ float clamp_log_scale(float b) { return b < -CK_LIM ? -CK_LIM : (b > CK_LIM ? CK_LIM : b); }

#define CK_LOOP(I, u, units)                                                         \
  const I _stride = (I)gridDim.x * (I)blockDim.x;                                    \
  for (I u = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x; u < (units); u += _stride)

// u = y, v = |y - mu| at the anchors; +0.0 elsewhere
template <typename I, bool VEC>
__global__ void __launch_bounds__(CK_THREADS) input_fwd_k(const float* __restrict__ y, const float* __restrict__ mu, I units,
                                                          Geo<I> g, float* __restrict__ u, float* __restrict__ v) {
  constexpr int E = VEC ? 4 : 1;
  CK_LOOP(I, t, units) {
    Vf<VEC> a = zeros<VEC>(), b = zeros<VEC>();
    if (is_anchor(t, g)) {
      a = ld<VEC>(y, t);
      const Vf<VEC> m = ld<VEC>(mu, t);
#pragma unroll
      for (int k = 0; k < E; ++k) b.e[k] = fabsf(__fsub_rn(a.e[k], m.e[k]));
    }
    st<VEC>(u, t, a);
    st<VEC>(v, t, b);
  }
}

// at the anchors, s = sign(y - mu): dy = du + s dv, dmu = -s dv; +0.0 elsewhere
template <typename I, bool VEC>
__global__ void __launch_bounds__(CK_THREADS) input_bwd_k(const float* __restrict__ y, const float* __restrict__ mu,
                                                          const float* __restrict__ du, const float* __restrict__ dv,
                                                          I units, Geo<I> g, float* __restrict__ dy,
                                                          float* __restrict__ dmu) {
  constexpr int E = VEC ? 4 : 1;
  CK_LOOP(I, t, units) {
    Vf<VEC> gy = zeros<VEC>(), gm = zeros<VEC>();
    if (is_anchor(t, g)) {
      const Vf<VEC> a = ld<VEC>(y, t), m = ld<VEC>(mu, t), gu = ld<VEC>(du, t), gv = ld<VEC>(dv, t);
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const float d = __fsub_rn(a.e[k], m.e[k]);
        gy.e[k] = d > 0.0f ? gu.e[k] + gv.e[k] : (d < 0.0f ? gu.e[k] - gv.e[k] : gu.e[k]);
        gm.e[k] = d > 0.0f ? -gv.e[k] : (d < 0.0f ? gv.e[k] : 0.0f);
      }
    }
    st<VEC>(dy, t, gy);
    st<VEC>(dmu, t, gm);
  }
}

// mu = mu_h + a, sigma = sigma_h expf(clamp(b)) at the non-anchors; mu_h, sigma_h at the anchors
template <typename I, bool VEC>
__global__ void __launch_bounds__(CK_THREADS) params_fwd_k(const float* __restrict__ mu_h, const float* __restrict__ sigma_h,
                                                           const float* __restrict__ a, const float* __restrict__ b, I units,
                                                           Geo<I> g, float* __restrict__ mu, float* __restrict__ sigma) {
  constexpr int E = VEC ? 4 : 1;
  CK_LOOP(I, t, units) {
    Vf<VEC> m = ld<VEC>(mu_h, t), s = ld<VEC>(sigma_h, t);
    if (!is_anchor(t, g)) {
      const Vf<VEC> da = ld<VEC>(a, t), db = ld<VEC>(b, t);
#pragma unroll
      for (int k = 0; k < E; ++k) {
        m.e[k] = __fadd_rn(m.e[k], da.e[k]);
        s.e[k] = __fmul_rn(s.e[k], expf(clamp_log_scale(db.e[k])));
      }
    }
    st<VEC>(mu, t, m);
    st<VEC>(sigma, t, s);
  }
}

// dmu_h = dmu; at the non-anchors da = dmu, dsigma_h = dsigma e, db = dsigma sigma_h e inside the clamp (else 0),
// e = expf(clamp(b)); at the anchors da = db = 0, dsigma_h = dsigma
template <typename I, bool VEC>
__global__ void __launch_bounds__(CK_THREADS) params_bwd_k(const float* __restrict__ sigma_h, const float* __restrict__ b,
                                                           const float* __restrict__ dmu, const float* __restrict__ dsigma,
                                                           I units, Geo<I> g, float* __restrict__ dmu_h,
                                                           float* __restrict__ dsigma_h, float* __restrict__ da,
                                                           float* __restrict__ db) {
  constexpr int E = VEC ? 4 : 1;
  CK_LOOP(I, t, units) {
    const Vf<VEC> gm = ld<VEC>(dmu, t);
    Vf<VEC> gs = ld<VEC>(dsigma, t);
    Vf<VEC> ga = zeros<VEC>(), gb = zeros<VEC>();
    if (!is_anchor(t, g)) {
      const Vf<VEC> s = ld<VEC>(sigma_h, t), lb = ld<VEC>(b, t);
      ga = gm;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const float e = expf(clamp_log_scale(lb.e[k]));
        const bool inside = lb.e[k] >= -CK_LIM && lb.e[k] <= CK_LIM;
        gb.e[k] = inside ? __fmul_rn(__fmul_rn(gs.e[k], s.e[k]), e) : 0.0f;
        gs.e[k] = __fmul_rn(gs.e[k], e);
      }
    }
    st<VEC>(dmu_h, t, gm);
    st<VEC>(dsigma_h, t, gs);
    st<VEC>(da, t, ga);
    st<VEC>(db, t, gb);
  }
}

// T: the unit that is copied (one element, or 16 bytes of one position).  GATHER: half[u] = full[...], else back.
template <typename I, typename T, bool GATHER>
__global__ void __launch_bounds__(CK_THREADS) move_k(const T* __restrict__ src, I units, int par, Geo<I> g,
                                                     T* __restrict__ dst) {
  CK_LOOP(I, t, units) {
    const I f = full_unit(t, par, g);
    if (GATHER)
      dst[t] = src[f];
    else
      dst[f] = src[t];
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int blocks_for(long long units) {
  return (int)std::min<long long>((units + CK_THREADS - 1) / CK_THREADS, CK_MAXBLOCKS);
}

// N H W C as one element count; 0: a size below 1 or a product past 2^63 - 1
long long checked_count(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 1) return 0;
  const long long a = (long long)N * H, b = (long long)W * C;   // each below 2^62
  if (a > 0x7fffffffffffffffll / b) return 0;
  return a * b;
}

long long parity_count(long long H, long long W, int parity) {
  const long long hw = H * W;
  return parity == 0 ? (hw + 1) / 2 : hw / 2;
}

constexpr long long CK_IDX32 = 0x7fffffffll;   // FastDiv's numerators stay below 2^31

// kernel<I, VEC> over the whole tensor, `epu` elements per unit
#define CK_LAUNCH_FULL(kernel, n, C, H, W, vec, st, ...)                                                          \
  do {                                                                                                            \
    const long long _epu = (vec) ? 4 : 1, _units = (n) / _epu;                                                    \
    const dim3 _grid(blocks_for(_units));                                                                         \
    if ((n) <= CK_IDX32) {                                                                                        \
      const Geo<uint32_t> _g((C) / _epu, (W), (H), 1, 1);                                                         \
      if (vec)                                                                                                    \
        hipLaunchKernelGGL((kernel<uint32_t, true>), _grid, dim3(CK_THREADS), 0, (st), __VA_ARGS__);             \
      else                                                                                                        \
        hipLaunchKernelGGL((kernel<uint32_t, false>), _grid, dim3(CK_THREADS), 0, (st), __VA_ARGS__);            \
    } else {                                                                                                      \
      const Geo<long long> _g((C) / _epu, (W), (H), 1, 1);                                                        \
      if (vec)                                                                                                    \
        hipLaunchKernelGGL((kernel<long long, true>), _grid, dim3(CK_THREADS), 0, (st), __VA_ARGS__);            \
      else                                                                                                        \
        hipLaunchKernelGGL((kernel<long long, false>), _grid, dim3(CK_THREADS), 0, (st), __VA_ARGS__);           \
    }                                                                                                             \
  } while (0)

// gather / scatter of `elem_bytes`-wide elements between `full` and the packed `half` of one parity
template <bool GATHER>
int move_half(const void* src, void* dst, const void* full, const void* half, int elem_bytes, int N, int H, int W, int C,
              int parity, hipStream_t st) {
  const long long n = checked_count(N, H, W, C);
  if (!src || !dst || src == dst || n == 0 || (parity != 0 && parity != 1) || (elem_bytes != 1 && elem_bytes != 4))
    return IC_ERR_ARG;
  const long long cnt = parity_count(H, W, parity);
  if (cnt == 0) return IC_OK;   // a 1 x 1 map has no non-anchor: the half is empty
  const long long first = (W - parity + 1) / 2;   // positions of the parity in an even row
  const int epv = 16 / elem_bytes;
  const bool vec = C % epv == 0 && aligned16(full) && aligned16(half);
  const long long upp = vec ? C / epv : C;        // units per position
  const long long units = (long long)N * cnt * upp;
  const dim3 grid(blocks_for(units));
#define CK_MOVE(I, T)                                                                                               \
  hipLaunchKernelGGL((move_k<I, T, GATHER>), grid, dim3(CK_THREADS), 0, st, (const T*)src, (I)units, parity,        \
                     Geo<I>(upp, W, H, cnt, first), (T*)dst)
  // every index formed is below the full tensor's unit count
  if (n <= CK_IDX32) {
    if (vec)
      CK_MOVE(uint32_t, bytes16);
    else if (elem_bytes == 4)
      CK_MOVE(uint32_t, uint32_t);
    else
      CK_MOVE(uint32_t, uint8_t);
  } else {
    if (vec)
      CK_MOVE(long long, bytes16);
    else if (elem_bytes == 4)
      CK_MOVE(long long, uint32_t);
    else
      CK_MOVE(long long, uint8_t);
  }
#undef CK_MOVE
  IC_CHECK_LAUNCH();
  return IC_OK;
}

}  // namespace

extern "C" {

int ic_ckbd_input_fwd(const float* y, const float* mu, int N, int H, int W, int C, float* u, float* v, void* stream) {
  const long long n = checked_count(N, H, W, C);
  if (!y || !mu || !u || !v || u == v || n == 0) return IC_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(y) && aligned16(mu) && aligned16(u) && aligned16(v);
  CK_LAUNCH_FULL(input_fwd_k, n, C, H, W, vec, (hipStream_t)stream, y, mu, _units, _g, u, v);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_ckbd_input_bwd(const float* y, const float* mu, const float* du, const float* dv, int N, int H, int W, int C,
                      float* dy, float* dmu, void* stream) {
  const long long n = checked_count(N, H, W, C);
  if (!y || !mu || !du || !dv || !dy || !dmu || dy == dmu || n == 0) return IC_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(y) && aligned16(mu) && aligned16(du) && aligned16(dv) && aligned16(dy) &&
                   aligned16(dmu);
  CK_LAUNCH_FULL(input_bwd_k, n, C, H, W, vec, (hipStream_t)stream, y, mu, du, dv, _units, _g, dy, dmu);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_ckbd_params_fwd(const float* mu_h, const float* sigma_h, const float* a, const float* b, int N, int H, int W, int C,
                       float* mu, float* sigma, void* stream) {
  const long long n = checked_count(N, H, W, C);
  if (!mu_h || !sigma_h || !a || !b || !mu || !sigma || mu == sigma || n == 0) return IC_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(mu_h) && aligned16(sigma_h) && aligned16(a) && aligned16(b) && aligned16(mu) &&
                   aligned16(sigma);
  CK_LAUNCH_FULL(params_fwd_k, n, C, H, W, vec, (hipStream_t)stream, mu_h, sigma_h, a, b, _units, _g, mu, sigma);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

int ic_ckbd_params_bwd(const float* sigma_h, const float* b, const float* dmu, const float* dsigma, int N, int H, int W,
                       int C, float* dmu_h, float* dsigma_h, float* da, float* db, void* stream) {
  const long long n = checked_count(N, H, W, C);
  if (!sigma_h || !b || !dmu || !dsigma || !dmu_h || !dsigma_h || !da || !db || n == 0) return IC_ERR_ARG;
  if (dmu_h == dsigma_h || dmu_h == da || dmu_h == db || dsigma_h == da || dsigma_h == db || da == db) return IC_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(sigma_h) && aligned16(b) && aligned16(dmu) && aligned16(dsigma) &&
                   aligned16(dmu_h) && aligned16(dsigma_h) && aligned16(da) && aligned16(db);
  CK_LAUNCH_FULL(params_bwd_k, n, C, H, W, vec, (hipStream_t)stream, sigma_h, b, dmu, dsigma, _units, _g, dmu_h, dsigma_h,
                 da, db);
  IC_CHECK_LAUNCH();
  return IC_OK;
}

long long ic_ckbd_count(int H, int W, int parity) {
  if (H < 1 || W < 1 || (parity != 0 && parity != 1)) return -1;
  return parity_count(H, W, parity);
}

int ic_ckbd_gather(const void* src, int elem_bytes, int N, int H, int W, int C, int parity, void* dst, void* stream) {
  return move_half<true>(src, dst, src, dst, elem_bytes, N, H, W, C, parity, (hipStream_t)stream);
}

int ic_ckbd_scatter(const float* half, int N, int H, int W, int C, int parity, float* full, void* stream) {
  return move_half<false>(half, full, full, half, 4, N, H, W, C, parity, (hipStream_t)stream);
}

}  // extern "C"
