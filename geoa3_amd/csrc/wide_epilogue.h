// The lane's part of the max-over-points epilogue of the 1024-wide MFMA kernels (pointnet_wide16.hip,
// pointnet_wide_split.hip): the first maximum of the NV accumulator values a lane holds for one channel.
//
// Two passes, no branch per element.  The single-pass form (`gt = x > v; v = gt ? x : v; col = gt ? n : col`) is one
// dependent chain of NV links, each a compare that waits for the previous select; with a validity test in front
// (`n < N && x > v`) every link became an exec-mask region with a branch (NOTEBOOK 10).  Here:
//   pass 1: m = the maximum, a chain of fmaxf that compiles to v_max3_f32 (NV / 2 instructions);
//   pass 2: the LOWEST index whose value equals m: compares against the one value m -- independent of each other --
//           and one select each, scanned in descending point order so that the lowest index is written last.
// Points past the end of a ragged tile are set to -inf by the caller first (selects, under a branch that is uniform over the workgroup), so both passes
// are the same code for full and ragged tiles.
//
// The published value keeps its bits.  v_max does not promise which zero it returns and x == m holds across +0 / -0,
// where the single-pass scan published the FIRST zero's sign (wide_key orders -0 below +0).  m differs from the selected
// element in that case only, so a wave in which some lane has m == 0 re-reads the value from the selected element (a
// wave-uniform branch that a layer with non-zero maxima never takes).
// NaN: fmaxf drops a NaN operand and x == m is false for it, as `x > v` was; a lane whose values are all NaN returns
// garbage, but an accumulator is only NaN in a unit whose staging pass saw a non-finite activation, and that unit has
// already raised all of the instance's keys to ~0 (`bad`), which no key written from here exceeds.
#pragma once

// get(i): value i of the lane in ascending point order (i < NV, compile-time after unrolling); idx(i): its local point
// index (a constant).

// pass 1: the lane's maximum
template <int NV, class Get>
__device__ __forceinline__ float wide_lane_max(Get get) {
  float m = get(NV - 1);
#pragma unroll
  for (int i = NV - 2; i >= 0; --i) m = fmaxf(m, get(i));
  return m;
}

// the value to publish for the maximum m: m itself, or the first zero's own bits where m is a zero
template <int NV, class Get>
__device__ __forceinline__ float wide_first_value(Get get, float m) {
  float v = m;
  if (__builtin_amdgcn_ballot_w64(m == 0.f) != 0ull) {
    v = get(NV - 1);
#pragma unroll
    for (int i = NV - 2; i >= 0; --i) v = get(i) == m ? get(i) : v;
  }
  return v;
}

// pass 2 over the values HI .. LO, descending: l = the lowest index among them whose value equals m, else unchanged.
// A whole scan starts from l = idx(NV - 1) and HI = NV - 2: the last point is the answer when no earlier one equals m.
template <int HI, int LO, class Get, class Idx>
__device__ __forceinline__ void wide_scan_desc(Get get, Idx idx, float m, int& l) {
#pragma unroll
  for (int i = HI; i >= LO; --i) l = get(i) == m ? idx(i) : l;
}

// both passes: the value and the local index of the lane's first maximum
template <int NV, class Get, class Idx>
__device__ __forceinline__ void wide_lane_first_max(Get get, Idx idx, float& v, int& loc) {
  const float m = wide_lane_max<NV>(get);
  v = wide_first_value<NV>(get, m);
  loc = idx(NV - 1);
  wide_scan_desc<NV - 2, 0>(get, idx, m, loc);
}

// the cross-lane merge of two (value, point) pairs: strict >, equal values to the lower point.  Bitwise on purpose:
// `a || (b && c)` compiled to an exec-mask region with a branch per merge step
__device__ __forceinline__ bool wide_merge_take(float ov, int oc, float v, int col) {
  return (ov > v) | ((ov == v) & (oc < col));
}
