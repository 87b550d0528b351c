// The segmented symbolizer: every entry point that turns floats into the coder's symbols (codec.hip, meancodec.hip,
// budget.hip, transcode.hip, mapbudget.hip) is this walk and this driver around its own source of floats.
//   * nseg segments of `len` symbols back to back; blockIdx.y is the segment.  sym[seg][i] = symbol_of(the float the
//     source gives for element i of the segment), codec_sym.h's rule, and kmax[seg] is the segment's largest |symbol|
//     by one integer atomicMax per block: order-independent, deterministic.  No floating-point atomics.
//   * Grid-stride and HBM-bound.  VEC: 16-byte accesses, four symbols per iteration, then the len % 4 elements after
//     the last group one by one; otherwise scalar accesses with the same arithmetic.  The entry point chooses: VEC
//     needs every pointer and every segment's start on a 16-byte boundary.
//   * A source (`Src`) is a trivially copyable struct that travels as a kernel argument.  bind(seg, len, first, step)
//     moves its pointers to the segment and sets whatever cursor it keeps: the thread's first element is `first`, and
//     it moves on by `step` elements per iteration.  at<V>(i) is the float (V = float, element i) or the four floats
//     (V = floatx4v, elements 4 i .. 4 i + 3) to be symbolized, its arithmetic written with fp_rn.h's helpers, each
//     operation rounded once; next() advances the cursor by one iteration.  A source whose cursor follows the channel
//     is launched with VEC only when C % 4 == 0: then len % 4 == 0 and no element is left over for the tail.
#pragma once
#include <algorithm>

#include "common.h"
#include "codec_sym.h"
#include "fp_rn.h"
#include "../../include/imgcomp.h"

typedef int intx4v __attribute__((ext_vector_type(4)));

constexpr int SEG_THREADS = 256;
constexpr int SEG_MAXBLOCKS = 1024;

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// element i of p in units of V (a float or four of them)
template <class V>
__device__ __forceinline__ V load_as(const float* p, long long i) {
  return reinterpret_cast<const V*>(p)[i];
}

// The cursor of a source over channels-last storage: c, the channel of the thread's element, advances by
// step = (stride * W) % C per iteration, with no division in the loop
struct ChannelCursor {
  int C, c, step;
  __device__ __forceinline__ void start(long long first, long long per) { c = (int)(first % C), step = (int)(per % C); }
  __device__ __forceinline__ void next() {
    c += step;
    if (c >= C) c -= C;
  }
};

template <bool VEC, class Src>
__global__ void __launch_bounds__(SEG_THREADS) seg_symbolize_k(Src src, long long len, int* __restrict__ sym,
                                                               int* __restrict__ kmax) {
  constexpr int W = VEC ? 4 : 1;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  src.bind(blockIdx.y, len, tid * W, stride * W);
  int* ss = sym + (long long)blockIdx.y * len;
  const long long n = len / W;
  int m = 0;
  for (long long i = tid; i < n; i += stride) {
    if (VEC) {
      const floatx4v v = src.template at<floatx4v>(i);
      intx4v k;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        k[j] = symbol_of(v[j]);
        m = max(m, k[j] < 0 ? -k[j] : k[j]);
      }
      reinterpret_cast<intx4v*>(ss)[i] = k;
    } else {
      const int k = symbol_of(src.template at<float>(i));
      ss[i] = k;
      m = max(m, k < 0 ? -k : k);
    }
    src.next();
  }
  if (VEC) {   // fewer than four elements: one thread each, no loop
    const long long i = (n << 2) + tid;
    if (i < len) {
      const int k = symbol_of(src.template at<float>(i));
      ss[i] = k;
      m = max(m, k < 0 ? -k : k);
    }
  }
  m = block_max(m);
  if (threadIdx.x == 0) atomicMax(kmax + blockIdx.y, m);
}

// blocks per segment: a function of (len, vec) alone, for a source whose cursor steps are worked out on the host
static inline unsigned seg_blocks(long long len, bool vec) {
  const long long work = vec ? (len + 3) / 4 : len;
  return (unsigned)std::min<long long>((work + SEG_THREADS - 1) / SEG_THREADS, SEG_MAXBLOCKS);
}

// The launch and its bookkeeping, after the entry point's own argument checks: img (where the source names an image
// per segment; null otherwise) goes to img_dev, which `src` already points at; kmax_dev is cleared, the kernel
// launched, the maxima copied to kmax_host and the stream waited for.  IC_ERR_ARG when a segment's maximum exceeds
// the coder's limit: kmax_host then says which.
template <class Src>
int seg_symbolize(const Src& src, bool vec, int nseg, long long len, const int* img, int* img_dev, int* sym,
                  int* kmax_dev, int* kmax_host, hipStream_t st) {
  hipError_t e;
  if (img) {
    // the host array is consumed before this returns (a copy from pageable memory is staged by the runtime)
    e = hipMemcpyAsync(img_dev, img, sizeof(int) * nseg, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
  }
  e = hipMemsetAsync(kmax_dev, 0, sizeof(int) * nseg, st);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(seg_blocks(len, vec), (unsigned)nseg);
  if (vec)
    hipLaunchKernelGGL((seg_symbolize_k<true, Src>), grid, dim3(SEG_THREADS), 0, st, src, len, sym, kmax_dev);
  else
    hipLaunchKernelGGL((seg_symbolize_k<false, Src>), grid, dim3(SEG_THREADS), 0, st, src, len, sym, kmax_dev);
  IC_CHECK_LAUNCH();
  e = hipMemcpyAsync(kmax_host, kmax_dev, sizeof(int) * nseg, hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return (int)e;
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  for (int s = 0; s < nseg; ++s)
    if (kmax_host[s] > IC_CODEC_KMAX) return IC_ERR_ARG;
  return IC_OK;
}
