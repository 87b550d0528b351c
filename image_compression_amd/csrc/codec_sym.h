// The two device functions under the symbolizers' walk (seg_symbolize.h): the clamp-and-NaN rule that turns a
// float into a symbol, and the block maximum behind the one integer atomicMax per block.
#pragma once
#include "common.h"

// q = rintf(v) (the value quant_k / cond_fwd_k mode 1 produce) as int32.
// |q| beyond 2^30 (or NaN) only has to be reported as too large, not represented
__device__ __forceinline__ int symbol_of(float v) {
  const float q = fminf(fmaxf(rintf(v), -1073741824.f), 1073741824.f);
  return (q == q) ? (int)q : 1073741824;
}

// the block's maximum of m, in thread 0 (blockDim.x a multiple of 64, <= 1024)
__device__ __forceinline__ int block_max(int m) {
  __shared__ int smax[16];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = max(m, smax[w]);
  return m;
}
