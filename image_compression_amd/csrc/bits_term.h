// The rate term of one likelihood, shared by the cross-entropy reduction (elementwise.hip, ic_ce_loss_fwd) and the
// block maps of it (ratemap.hip, ic_block_bits): one definition, so that a map always sums what the loss sums.
#pragma once
#include <hip/hip_runtime.h>

#define IC_LN2F 0.693147180559945309f

// clamp(-ln(p + 1e-10) / ln 2, 0, 50): the bits of one symbol of likelihood p
__device__ __forceinline__ float ic_bits_term(float p) {
  const float t = -logf(p + 1e-10f) / IC_LN2F;
  return fminf(fmaxf(t, 0.f), 50.f);
}
