// The pieces of the geometric objective that its kernels share (geom_loss.hip, geom_loss_wide.hip): the Hausdorff arg-max
// order, the 64-bit fixed-point gradient sums, the G-lane butterfly and the pair term.  The kernels are held to each other
// BIT FOR BIT (tests/test_gpu_geo_wide.py): change these here or nowhere.
#pragma once
#include "common.h"

namespace {

constexpr float NORM_EPS = 1e-12f;  // Lib/utility.py:30 (_normalize eps)

struct MaxIdx {
  float v;
  int i;
};
__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b) {  // larger value, then lower index
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

// ------------------------------------------------------------------------------------------
// Order-free accumulation of gradient terms: 64-bit FIXED POINT at two scales, chosen per instance.
//
// Integer addition is associative, so sums of converted terms do not depend on who adds them in which order (LDS integer
// atomics): deterministic and batch-independent without reverse lists.  Round 4 used ONE fixed scale (2^-44 per unit, every
// term clamped silently at 2^18): right for the attack loop's magnitudes, wrong for a caller-supplied dkappa, for loss
// weights far from 1 and for near-coincident pairs (a pair term is ~ 2 dk / r).  Now, with X = the instance's largest
// coefficient (2 w_curv / (N k) or max |dkappa| / k; the Chamfer coefficients) and Ex = ceil(log2 X):
//   fine    unit 2^(Ex - 40), terms up to 2^(Ex + 10):  4096 of them still fit 63 bits; X-relative precision 2^-40;
//   coarse  unit 2^(Ex - 16), terms up to 2^(Ex + 34):  pairs down to r ~ 1e-10 at the largest coefficient -- they are
//           rare, so their sums live in a small hash pool in LDS keyed by the destination point;
//   beyond that (or NaN, or a full pool): the destination's gradient is written as NaN -- loud, never a silent clamp.
// The result is fine * 2^(Ex - 40) + coarse * 2^(Ex - 16) in fp32.
// ------------------------------------------------------------------------------------------
struct GeoFix {
  float to_f, to_c, from_f, from_c, lim_f, lim_c;
};
__device__ __forceinline__ float geo_pow2(int k) { return __uint_as_float((unsigned)(k + 127) << 23); }   // -126 <= k <= 127
__device__ __forceinline__ GeoFix geo_fix_make(float X) {
  int Ex = (int)((__float_as_uint(X) >> 23) & 0xffu) - 126;        // X < 2^Ex (X = m 2^Ex, 0.5 <= m < 1)
  Ex = Ex < -80 ? -80 : (Ex > 60 ? 60 : Ex);                        // (X = 0, denormal or absurd: any scale will do)
  GeoFix f;
  f.to_f = geo_pow2(40 - Ex);
  f.to_c = geo_pow2(16 - Ex);
  f.from_f = geo_pow2(Ex - 40);
  f.from_c = geo_pow2(Ex - 16);
  f.lim_f = geo_pow2(Ex + 10);
  f.lim_c = geo_pow2(Ex + 34);
  return f;
}
__device__ __forceinline__ unsigned long long geo_fix_conv(float v, float mul) {
  return (unsigned long long)__float2ll_rn(v * mul);
}
// hash pool of destinations with coarse sums: key [cap] (-1 = empty), acc [cap][W] 64-bit words
struct GeoPool {
  int* key;
  unsigned long long* acc;
  int cap;   // a power of two
};
__device__ __forceinline__ int geo_pool_find(const GeoPool& P, int q, bool insert) {
  unsigned h = ((unsigned)q * 0x9E3779B1u) >> 8;
  for (int step = 0; step < P.cap; ++step) {
    const int s = (int)((h + (unsigned)step) & (unsigned)(P.cap - 1));
    int kk = P.key[s];
    if (kk == q) return s;
    if (kk == -1) {
      if (!insert) return -1;
      kk = atomicCAS(&P.key[s], -1, q);
      if (kk == -1 || kk == q) return s;
    }
  }
  return -1;
}
__device__ __forceinline__ void geo_mark_bad(unsigned* s_bad, int q) { atomicOr(&s_bad[q >> 5], 1u << (q & 31)); }
// one gradient term of destination q: into the per-point fine sums (planes of N, or null: everything through the pool,
// words 0-2 fine / 3-5 coarse), the pool's coarse sums, or the sticky NaN flags
template <int W>
__device__ __forceinline__ void geo_fix_add(const GeoFix& F, unsigned long long* fine, int N, const GeoPool& P, unsigned* s_bad,
                                            int q, float x, float y, float z) {
  const float m = fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z));
  if (m <= F.lim_f) {
    if (W == 3) {
      atomicAdd(&fine[q], geo_fix_conv(x, F.to_f));
      atomicAdd(&fine[N + q], geo_fix_conv(y, F.to_f));
      atomicAdd(&fine[2 * N + q], geo_fix_conv(z, F.to_f));
    } else {
      const int s = geo_pool_find(P, q, true);
      if (s < 0) return geo_mark_bad(s_bad, q);
      atomicAdd(&P.acc[s * W + 0], geo_fix_conv(x, F.to_f));
      atomicAdd(&P.acc[s * W + 1], geo_fix_conv(y, F.to_f));
      atomicAdd(&P.acc[s * W + 2], geo_fix_conv(z, F.to_f));
    }
  } else if (m <= F.lim_c) {
    const int s = geo_pool_find(P, q, true);
    if (s < 0) return geo_mark_bad(s_bad, q);
    atomicAdd(&P.acc[s * W + W - 3], geo_fix_conv(x, F.to_c));
    atomicAdd(&P.acc[s * W + W - 2], geo_fix_conv(y, F.to_c));
    atomicAdd(&P.acc[s * W + W - 1], geo_fix_conv(z, F.to_c));
  } else {
    geo_mark_bad(s_bad, q);      // out of range or NaN
  }
}
constexpr int GEO_POOL_CAP = 128;                                     // geo_fused_kernel: overflowed rows (fine + coarse sums)
constexpr size_t GEO_POOL_BYTES = GEO_POOL_CAP * (4 + 6 * 8) + 8;     // keys + sums + alignment
constexpr int GB_POOL_CAP = 256;                                      // geo_big_kernel: destinations with coarse terms
// the instance's largest coefficient: max |dkappa| / k over the block (dkappa mode) or the loss's analytic bound (kappa is a
// mean of |cosines|: |kappa_adv - kappa_ori| <= 1), and the Chamfer coefficients
__device__ __forceinline__ float geo_coef_bound(const geoa3_geo_args& A, int N, int Nr, float block_max_dkappa) {
  const float k = (float)(A.k > 0 ? A.k : 1);
  float X = A.dkappa ? block_max_dkappa / k : fabsf(A.w_curv) * 2.0f / ((float)N * k);
  X = fmaxf(X, fabsf(A.w_dis) * 2.0f / (float)(N < Nr ? N : Nr));
  return X;
}

// An entry of the neighbour table before it forms an address.  geoa3_knn / geoa3_knn_self write -1 into the row of a point
// with a NaN coordinate (and for K > N): outside [0, n) the entry is replaced by `self`, `oob` is set, and the caller gives
// the neighbour a NaN coordinate, so that the pair's term -- kappa, coefficient, both gradient shares -- counts as NaN.
__device__ __forceinline__ int geo_tab_idx(int q, int n, int self, bool& oob) {
  oob = (unsigned)q >= (unsigned)n;
  return oob ? self : q;
}
// the sign of t for d|t|: 0 at 0, and a NaN stays a NaN (with 0 for it a NaN neighbour's pull was 0 under a given dkappa)
__device__ __forceinline__ float geo_sign(float t) { return t > 0.f ? 1.f : (t < 0.f ? -1.f : (t == t ? 0.f : t)); }

template <int G>
__device__ __forceinline__ float group_sum(float v) {   // sum over aligned groups of G lanes, in every lane of the group
  if (G >= 2) v += dpp_f32<0xB1, 0xF>(v, 0.f);           // lane ^ 1
  if (G >= 4) v += dpp_f32<0x4E, 0xF>(v, 0.f);           // lane ^ 2
  if (G >= 8) v += dpp_f32<0x141, 0xF>(v, 0.f);          // row_half_mirror
  if (G >= 16) v += dpp_f32<0x140, 0xF>(v, 0.f);         // row_mirror
  if (G >= 32) v += __shfl_xor(v, 16, 64);
  if (G >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

// d |<normalize(q - p), n>| * dk / d q for the pair (centre p with normal n and coefficient dk, neighbour q): what the
// centre subtracts from its own gradient and q adds to its
// The pair kernel is bound by VALU issue on the one CU that holds an instance (~100 instructions per pair term, a third
// of them the IEEE sqrt / division sequences): v_sqrt_f32 and v_rcp_f32 (1 ulp each) take 8 us off 51 (250 instances).
// Two ulp per pair term is far inside the parity bars (values rtol 2e-5, gradients 1e-4; the summation order already
// differs from torch's); -DGEOA3_GEO_IEEE restores the correctly rounded forms.
#ifdef GEOA3_GEO_IEEE
#define GEO_SQRT(x) sqrtf(x)
#define GEO_RCP(x) (1.0f / (x))
#else
#define GEO_SQRT(x) __builtin_amdgcn_sqrtf(x)
#define GEO_RCP(x) __builtin_amdgcn_rcpf(x)
#endif
// (The multiply-adds are spelled out and contraction is OFF inside: the overflowed-row path forms a row's terms at two
// call sites -- the pair lane in phase 1, the owner in phase 2 -- whose sums must agree bit for bit whichever of them
// converts a given term; left to -ffp-contract=fast each inlined copy is fused as its surroundings suggest.)
__device__ __forceinline__ void geo_pair_grad(float px, float py, float pz, float nx, float ny, float nz, float dk, float qx,
                                              float qy, float qz, float& dvx, float& dvy, float& dvz, float& t_out) {
#pragma clang fp contract(off)
  const float vx = qx - px, vy = qy - py, vz = qz - pz;
  const float r = GEO_SQRT(__builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx)));
  const float inv = GEO_RCP(fmaxf(r, NORM_EPS));
  const float ux = vx * inv, uy = vy * inv, uz = vz * inv;
  const float t = __builtin_fmaf(uz, nz, __builtin_fmaf(uy, ny, ux * nx));
  const float sg = geo_sign(t);
  const float c = dk * sg * inv;
  if (r >= NORM_EPS) {  // d(v/|v|)/dv = (I - u u^T)/|v|
    dvx = c * __builtin_fmaf(-t, ux, nx);
    dvy = c * __builtin_fmaf(-t, uy, ny);
    dvz = c * __builtin_fmaf(-t, uz, nz);
  } else {              // clamp active: v/eps, the norm path carries no gradient
    dvx = c * nx;
    dvy = c * ny;
    dvz = c * nz;
  }
  t_out = t;
}

}  // namespace
