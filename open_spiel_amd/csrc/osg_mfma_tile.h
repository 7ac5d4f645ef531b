// The 16 x 16 fp32 matrix tile of the fused learners (k_mlp_train, k_deep_cfr_train, k_deep_cfr_train_wide) on v_mfma_f32_16x16x4_f32: fp32
// in, fp32 accumulate.  With lane l = 16 g + i of a wavefront the instruction takes A[i][g] and B[g][i] and leaves
// D[4 g + r][i] in register r of the accumulator.
#pragma once
#include "osg_common.h"

namespace osg_mfma {

typedef float f4 __attribute__((ext_vector_type(4)));

// D += A B with both operands stored row by row along the contraction: A[i][k] at a[i * sa + k], B[k][j] at
// bt[j * sb + k].  K is a multiple of 4.
OSG_D f4 mma_rows(const float* a, int sa, const float* bt, int sb, int K, f4 acc) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const float* pa = a + i * sa + g;
  const float* pb = bt + i * sb + g;
  for (int k = 0; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[k], pb[k], acc, 0, 0, 0);
  return acc;
}
// D += A B contracting over rows: A[i][k] at a[k * sa + i], B[k][j] at b[k * sb + j] (b null: B is all ones).  K is a
// multiple of 16; one instruction contracts rows k0 + t, + 4, + 8, + 12 (the bank argument of osg_mlp_plan.h).
OSG_D f4 mma_cols(const float* a, int sa, const float* b, int sb, int K, f4 acc) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const float* pa = a + 4 * g * sa + i;
  const float* pb = b ? b + 4 * g * sb + i : nullptr;
  for (int k0 = 0; k0 < K; k0 += 16)
#pragma unroll
    for (int t = 0; t < 4; ++t)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[(k0 + t) * sa], pb ? pb[(k0 + t) * sb] : 1.0f, acc, 0, 0, 0);
  return acc;
}

// D += A B, A stored row by row along the contraction (A[i][k] at a[i * sa + k]) and B row by row across it (B[k][j] at
// b[k * sb + j]): dH = dY W without the transposed copy.  The B read collides (osg_adam_plan.h, osg_adam_wide_plan.h).  K is a multiple of 4.
OSG_D f4 mma_mixed(const float* a, int sa, const float* b, int sb, int K, f4 acc) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const float* pa = a + i * sa + g;
  const float* pb = b + g * sb + i;
  for (int k = 0; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[k], pb[k * sb], acc, 0, 0, 0);
  return acc;
}

OSG_D float sum16(float v) {   // one fixed tree over the 16 lanes of a row; each of them gets the sum
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

OSG_D float wave_sum(float v) {   // one fixed tree; every lane gets the sum
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

}  // namespace osg_mfma
