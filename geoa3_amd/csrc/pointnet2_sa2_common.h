// Helpers shared by the PointNet++ level-2 kernels (pointnet2_sa2.hip: forward, pre-transform, the centre-major backward;
// pointnet2_sa2b.hip: the destination-ordered backward): tile geometry, v_readlane wrappers (the operand scales and the
// two-instruction fp16 hi / lo split: mfma_split.h).
#pragma once
#include "pointnet_kernels.h"

namespace {

constexpr int S2_K = 128;                // channels of a0 and a1
constexpr int S2_C = 256;                // pooled channels
constexpr int S2_PT = S2_K + 4;          // floats per row (= sample) of a tile
constexpr int S2_PF = 32;                // W2 rows in flight per lane in phase 1 (one wave per SIMD: L2 latency is exposed)

__device__ __forceinline__ int s2_rl(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float s2_rlf(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

}  // namespace
