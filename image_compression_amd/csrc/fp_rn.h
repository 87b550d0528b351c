// fp32 operations that are rounded to nearest once and never contracted with a neighbour: what "each operation rounded
// once" means wherever a kernel promises the bits of the separate ops it replaces.
//
// HIP's __fmul_rn / __fadd_rn / __fsub_rn do not say that to the compiler.  In this toolchain's headers they are the
// plain operators, compiled under the default contraction mode, and they carry that mode with them when they are
// inlined: a product followed by a sum or a difference becomes one v_fma_f32 / v_fmac_f32, one rounding instead of
// two, and a result whose product is inexact and whose sum lands on a tie at .5 rounds to the other integer (one
// symbol of y in 2.4 million on the benchmark's images, one in 18432 on random gain tables).  The helpers below are
// compiled with contraction off inside their own bodies, so the operation they emit carries no flag that lets the
// backend fuse it, whatever the mode of the code they are inlined into.  The pragma stands in each body, not at file
// scope: there it would go on into the including file and turn contraction off for kernels that want it.
//
// T is float or an ext_vector of floats (elementwise).  Where a fused operation is the rule, write fmaf explicitly.
#pragma once
#include <hip/hip_runtime.h>

template <class T>
__device__ __forceinline__ T mul_rn(T a, T b) {
#pragma clang fp contract(off)
  return a * b;
}

template <class T>
__device__ __forceinline__ T add_rn(T a, T b) {
#pragma clang fp contract(off)
  return a + b;
}

template <class T>
__device__ __forceinline__ T sub_rn(T a, T b) {
#pragma clang fp contract(off)
  return a - b;
}
