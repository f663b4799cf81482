// Split-fp16 operands of the f16 matrix pipe: the ONE definition of the vector types, the power-of-two scale rule
// and the hi / lo split.  The bit-for-bit contracts of the test suite (chain == layer-by-layer launches, fused == two-kernel
// backward, batch rows == batch-1 runs) rest on every kernel forming these pieces the same way: change them here or nowhere.
// The three products hh / hl / lh are NOT wrapped: their accumulation order is part of each kernel's bits and differs
// between kernels.
#pragma once
#include "common.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The scale rule: a block's maximum m -> [2^13, 2^14).  E = m's biased exponent clamped to [14, 254], scale = 2^(140 - E),
// unscale = 2^(E - 140).
// (sf_clamp on its own: for the kernels that also test the unclamped exponent for inf)
__device__ __forceinline__ unsigned sf_clamp(unsigned E) { return E < 14u ? 14u : (E > 254u ? 254u : E); }
__device__ __forceinline__ unsigned sf_exp(float m) { return sf_clamp((__float_as_uint(m) >> 23) & 0xffu); }
__device__ __forceinline__ float sf_scale(unsigned E) { return __uint_as_float((267u - E) << 23); }
__device__ __forceinline__ float sf_unscale(unsigned E) { return __uint_as_float((E - 13u) << 23); }

// hi = rn16(v), lo = rn16(v - hi).  (A few kernels still spell this expression in place, between their stores: the same
// bits; a call there makes the compiler schedule the kernel differently.)
__device__ __forceinline__ void sf_split(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)(v - (float)hi);
}

// (hi, lo) fp16 images of x0 * s and x1 * s, packed: v_pk_mul_f32 + v_cvt_pk_f16_f32 for the hi pieces, one v_fma_mixlo /
// mixhi_f16 per lo piece (the residual x * s - hi as one exact fma): two instructions per element where the scalar form
// took five (needs -fno-slp-vectorize: the SLP vectoriser turns the residual pair into three).  The same bits as
// hi = rn16(x s), lo = rn16(x s - hi): s is a power of two.
__device__ __forceinline__ void sf_split2(float x0, float x1, float s, unsigned& hi, unsigned& lo) {
  const float2v x = {x0, x1};
  // (the scale as a VECTOR register operand of the packed multiply: packed-FP32 instructions with SGPR-pair operands at
  // two waves per SIMD are what computed wrong values in conv_bwd_chain_kernel -- NOTEBOOK 5a; none are formed here)
  float sv = s;
  asm volatile("" : "+v"(sv));
  const half2v h = __builtin_convertvector(x * sv, half2v);
  const half2v l = {(_Float16)__builtin_fmaf(x0, s, -(float)h[0]), (_Float16)__builtin_fmaf(x1, s, -(float)h[1])};
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ void sf_split8(const float (&x)[8], float s, half8& oh, half8& ol) {
  uint4v H, Lw;
#pragma unroll
  for (int j2 = 0; j2 < 4; ++j2) {
    unsigned a, b;
    sf_split2(x[2 * j2], x[2 * j2 + 1], s, a, b);
    H[j2] = a;
    Lw[j2] = b;
  }
  oh = __builtin_bit_cast(half8, H);
  ol = __builtin_bit_cast(half8, Lw);
}
