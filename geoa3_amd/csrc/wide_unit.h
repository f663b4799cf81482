// What wide_split_kernel (pointnet_wide_split.hip) and wide16_kernel (pointnet_wide16.hip) do in front of and around
// their k loops, stated once: unit schedule, staging pass, hand-off of a unit's packed maxima, host launcher.  The k
// loops, weight rings, LDS layouts and epilogues are each kernel's own.  256 threads (4 waves), 128 points per unit.
//
// Schedule.  A work unit is (instance, 128-point tile, all 8 groups of 128 channels).  Instance b belongs to XCD b % 8
// (workgroup x runs on XCD x % 8); an XCD's units are dealt round robin to its `slots_per_xcd` workgroups.
// The two workgroups that share a CU start together and do identical work.  The workgroup in the odd wave slot of its
// SIMD (HW_ID.wave_id) runs half of its first unit's channel groups first and the other half at the very end (one extra
// staging pass), which shifts its phases by half a period, so one workgroup's staging and epilogues run under the
// other's MFMAs.  (s_memtime trace of wide_split_kernel, tools/bench_wide.py --stamps: per unit 7 % waiting for the
// tile, 7 % splitting it, 4 x 20.7 % channel groups of which 2 % epilogue.)  Worth 0-10 % depending on the device: the
// kernels sit at the clock-limited ceiling of the 16-bit matrix pipe (1.25 PFLOP/s executed at 1.86 GHz, 66 % busy).
//
// Staging.  Every value of the tile goes through registers once: maximum -> scale -> split -> LDS.  Wave w takes the
// channel octets w, w + 4, ..; a lane one point per pass: 8 coalesced row reads and two half8 stores per octet into a
// POINT-major image ([piece][point row][128 ci] fp16).  Separate pieces: each kernel has calls of its own between them.
//
// Hand-off.  A unit's packed maxima wait in LDS and are published (atomicMax) behind the NEXT unit's tile loads: that
// keeps the atomics out of the in-order vmcnt queue in front of the weight stream.
#pragma once
#include "pointnet_kernels.h"
#include "profile.h"

constexpr int WIDE_THREADS = 256;
constexpr int WIDE_PTS = 128;     // points per unit
constexpr int WIDE_GROUPS = 8;    // channel groups of 128 per unit

struct WideSchedule {
  int xcd, slot, slots_per_xcd, tiles;
  int nmine;    // units of this workgroup
  bool late;    // the odd-slot workgroup: its first unit's second half runs as iteration `nmine`
  __device__ __forceinline__ int iterations() const { return nmine + (late ? 1 : 0); }
};
struct WideUnit {
  int b, tile, n0, g_begin, g_end;   // instance, tile, first point, channel groups of this iteration
};

// s_max: the kernel's float[4] exchange array; carries HW_ID to all waves (one barrier)
__device__ __forceinline__ WideSchedule wide_schedule(const WideArgs& a, int slots_per_xcd, float* s_max) {
  WideSchedule s;
  s.xcd = blockIdx.x & 7, s.slot = blockIdx.x >> 3, s.slots_per_xcd = slots_per_xcd;
  s.tiles = (a.N + WIDE_PTS - 1) / WIDE_PTS;
  const int units = ((a.B - s.xcd + 7) / 8) * s.tiles;
  if (threadIdx.x == 0) s_max[0] = __int_as_float(__builtin_amdgcn_s_getreg((3 << 11) | 4) & 1);   // HW_REG_HW_ID[3:0]
  __syncthreads();
  s.nmine = units > s.slot ? (units - s.slot + slots_per_xcd - 1) / slots_per_xcd : 0;
  s.late = __float_as_int(s_max[0]) != 0 && s.nmine > 0;
  return s;
}
__device__ __forceinline__ WideUnit wide_unit(const WideSchedule& s, int it) {
  const int u = s.slot + (it == s.nmine ? 0 : it) * s.slots_per_xcd;
  const int q = u / s.tiles;
  WideUnit w;
  w.b = s.xcd + 8 * q, w.tile = u - q * s.tiles, w.n0 = w.tile * WIDE_PTS;
  w.g_begin = s.late && it == s.nmine ? WIDE_GROUPS / 2 : 0;
  w.g_end = s.late && it == 0 ? WIDE_GROUPS / 2 : WIDE_GROUPS;
  return w;
}

// points n0 .. n0 + 127 of the instance at X, zero past N.  ldx: a.ldX made opaque by the caller (asm "+s"), which keeps
// the row offsets from being hoisted out of the unit loop (they were spilled to scratch)
__device__ __forceinline__ void wide_load_tile(const float* X, int ldx, int n0, int N, int lane, int wave, float (&xv)[2][4][8]) {
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int n = n0 + pass * 64 + lane;
    const bool in = n < N;
    const float* px = X + (in ? n : 0);
#pragma unroll
    for (int oc = 0; oc < 4; ++oc)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = px[(size_t)(((wave + 4 * oc) * 8 + i) * ldx)];
        xv[pass][oc][i] = in ? v : 0.f;
      }
  }
}

// the wave's absolute maximum, starting from m (>= 0).  A NaN does not survive fmaxf: wide_split_store catches it
__device__ __forceinline__ float wide_abs_max(const float (&xv)[2][4][8], float m) {
#pragma unroll
  for (int pass = 0; pass < 2; ++pass)
#pragma unroll
    for (int oc = 0; oc < 4; ++oc)
#pragma unroll
      for (int i = 0; i < 8; ++i) m = fmaxf(m, __builtin_fabsf(xv[pass][oc][i]));
  return wave_max(m);
}

// the waves' maxima -> the tile's power-of-two scale (mfma_split.h) and its inverse; returns whether the maximum is inf.
// Behind its first barrier every wave is done with the previous unit's image and s_max
__device__ __forceinline__ bool wide_tile_scale(float m, float* s_max, int lane, int wave, float& scale, float& unscale) {
  __syncthreads();
  if (lane == 0) s_max[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  unsigned E = (__float_as_uint(m) >> 23) & 0xffu;
  const bool bad = E == 255u;
  E = sf_clamp(E);
  scale = sf_scale(E);
  unscale = sf_unscale(E);
  return bad;
}

// scale, split and store the tile; row0: the hi image's row of point n0 (rows ROWB bytes apart, lo image PIECEB bytes
// behind).  Returns whether a scaled value is NaN (a NaN input, or 0 * inf, inf - inf of an inf maximum)
template <int ROWB, int PIECEB>
__device__ __forceinline__ bool wide_split_store(const float (&xv)[2][4][8], float scale, unsigned char* row0, int lane, int wave) {
  bool bad = false;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int p = pass * 64 + lane;
#pragma unroll
    for (int oc = 0; oc < 4; ++oc) {
      half8 hi, lo;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xs = xv[pass][oc][i] * scale;
        bad |= xs != xs;
        _Float16 h, l;
        sf_split(xs, h, l);
        hi[i] = h;
        lo[i] = l;
      }
      unsigned char* dst = row0 + p * ROWB + (wave + 4 * oc) * 16;
      *reinterpret_cast<half8*>(dst) = hi;
      *reinterpret_cast<half8*>(dst + PIECEB) = lo;
    }
  }
  return bad;
}

// a non-finite activation anywhere in the tile: loud, not silently wrong -- key ~0 decodes to NaN in wide_finalize_kernel
__device__ __forceinline__ void wide_poison(const WideArgs& a, int b, bool bad) {
  if (__syncthreads_or(bad))
    for (int c = threadIdx.x; c < a.Co; c += WIDE_THREADS) atomicMax(a.keys + (size_t)b * a.Co + c, ~0ull);
}

// the unit whose maxima wait in LDS: instance, the wave's first channel, channel tiles of 32 (128 channels apart)
struct WidePending {
  int b = -1, co = 0, n = 0;
};
// key_at(i, l): LDS address of the key of channel l (< 32) of the wave's pending tile i
template <class KeyAt>
__device__ __forceinline__ void wide_flush(WidePending& p, const WideArgs& a, int lane, KeyAt key_at) {
  if (p.b < 0) return;
  for (int i = lane >> 5; i < p.n; i += 2)       // the two half-waves publish two channel tiles per instruction
    atomicMax(a.keys + (size_t)p.b * a.Co + p.co + i * 128 + (lane & 31), *key_at(i, lane & 31));
  p.b = -1;
}

// key memset unless clean, kernel on 32 * occ workgroups per XCD, finalize
template <class Kernel>
int wide_launch(Kernel kernel, int lds, int occ, int taps, int prof, const WideArgs& a, hipStream_t s) {
  if (a.Co != 1024 || a.taps != taps || !a.keys || !a.Wh) return GEOA3_ENOSUPPORT;
  geoa3_prof_begin(prof, s);
  if (!a.keys_clean && hipMemsetAsync(a.keys, 0, (size_t)a.B * a.Co * sizeof(unsigned long long), s) != hipSuccess)
    return GEOA3_ELAUNCH;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  const int slots = 32 * occ;
  hipLaunchKernelGGL(kernel, dim3(slots * 8), dim3(WIDE_THREADS), lds, s, a, slots);
  launch_wide_finalize(a, s);
  geoa3_prof_end(prof, s);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
