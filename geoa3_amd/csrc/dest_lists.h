// The destination lists of the ordered scatter-add backward passes (knn_gather_grad and the g2 half of knn_points_grad in
// geom_knn_ops.hip, three_interpolate_grad in pointnet2_interp.hip).  All three promise that every destination adds its
// contributions sequentially in float32, from +0.0, in ascending entry number, with no float atomics -- so a plain float32
// loop on the CPU reproduces every element bit for bit, whatever the batch an instance is part of.  They keep the promise
// the same way: the E entries of an instance are sorted by destination (a counting sort), then one thread per destination
// walks its list.  The sort is stated HERE, once: change these pieces here or nowhere.
//   tables (int32): start [M+1] | cursor [M] | bucket [E] | order [E]   per instance
//   1. count:  start[j] = number of entries that point at j (integer atomics: a count has no order)
//   2. scan:   start <- its exclusive prefix sum (start[M] = the total), cursor <- start          (dl_scan)
//   3. place:  every entry takes the next free place of its destination's segment of `bucket` (integer atomic cursor: the
//              ORDER inside a segment depends on timing ...)
//   4. sort:   ... so EVERY segment is sorted by entry number into `order` by rank counting -- the rank of an entry is the
//              number of smaller ones in its segment.  The entries are distinct, so the result is unique: it does not
//              depend on who ranks, in which order, or on the order `place` left.  Up to 64 entries: one wavefront
//              (dl_rank_short).  Longer (a hub can receive all E entries): the whole workgroup, every thread
//              counting for KPT entries of its own per pass while the segment goes by, the same address in every lane
//              (dl_rank_long); any length, quadratic in it.  Its loops and barriers are uniform: no thread may leave a
//              kernel before the last of them.
//   5. the caller's sum in list order; an empty list writes +0.0.
// An index outside [0, M) is the caller's error: it is neither wrapped nor clamped, its entry is in no list (dl_valid).
// Two forms of steps 1-4, the same lists:
//   launch_dest_lists (dest_lists.hip)  four launches, the tables of the whole batch in the caller's scratch;
//   ksl_build                           ONE workgroup of KSL_T threads per instance with its tables in LDS, for a kernel
//                                       that goes on to sum in the same launch (`long`, a fifth table, lists the segments of
//                                       more than 64 entries for the workgroup to rank one after the other).
#pragma once
#include <climits>
#include <type_traits>
#include "common.h"

// the scratch form: `scratch` (dest_lists_scratch_bytes, int32: start [B][M+1] | cursor [B][M] | bucket [B][E] | order [B][E])
// <- the lists of the B x M destinations of idx [B][E]; *start / *order point into it.  I = int32_t, int64_t.
// E <= INT_MAX - 255 and M < INT_MAX are the caller's to check; B E and B M may pass 2^31.
size_t dest_lists_scratch_bytes(int B, int E, int M);
template <typename I>
int launch_dest_lists(const I* idx, int B, int E, int M, void* scratch, hipStream_t s, const int** start, const int** order);

namespace {

constexpr int DL_TILE = 1024;   // entries of a long segment per LDS tile (the staged form of dl_rank_long)

template <typename I>
__device__ __forceinline__ bool dl_valid(I j, int M) {
  return (std::make_unsigned_t<I>)j < (std::make_unsigned_t<I>)M;
}

// wave-inclusive scan
__device__ __forceinline__ int dl_wave_scan(int x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  return x;
}

// step 2 by a workgroup of T threads: the counts start[0 .. M) -> their exclusive prefix sum in start and cursor,
// start[M] = the total.  The counts must be visible on entry; the caller fences the results.
template <int T>
__device__ __forceinline__ void dl_scan(int* start, int* cursor, int M) {
  __shared__ int s_w[T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int i0 = 0; i0 < M; i0 += T) {
    const int i = i0 + tid;
    const int v = i < M ? start[i] : 0;
    const int x = dl_wave_scan(v, lane);
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    int base = carry, total = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
      if (w < wave) base += s_w[w];
      total += s_w[w];
    }
    if (i < M) {
      start[i] = base + x - v;
      cursor[i] = base + x - v;
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) start[M] = carry;
}

// step 4, a segment of 1 <= L <= 64 entries by ONE wavefront (all 64 lanes call).  IN_LDS: `in` is LDS and every lane reads
// the same address (a broadcast read, pipelined); otherwise `in` is global memory, read once, and the keys go from lane to lane.
template <bool IN_LDS>
__device__ __forceinline__ void dl_rank_short(const int* in, int* out, int L, int lane) {
  const int key = lane < L ? in[lane] : INT_MAX;
  int r = 0;
  for (int k = 0; k < L; ++k) r += (IN_LDS ? in[k] : __shfl(key, k, 64)) < key ? 1 : 0;
  if (lane < L) out[r] = key;
}

// step 4, a segment of any length by the whole workgroup of T threads (every thread calls, with the same arguments).
// IN_LDS: `in` is read in place; otherwise it is global memory and passes through `tile` (LDS, DL_TILE ints).
template <int T, int KPT, bool IN_LDS>
__device__ __forceinline__ void dl_rank_long(const int* in, int* out, int L, int* tile) {
  const int tid = threadIdx.x;
  for (int p0 = 0; p0 < L; p0 += T * KPT) {
    int key[KPT], r[KPT];
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
      const int p = p0 + u * T + tid;
      key[u] = p < L ? in[p] : INT_MIN;   // (nothing is smaller than INT_MIN: such a slot counts nothing and writes nothing)
      r[u] = 0;
    }
    for (int t0 = 0; t0 < L; t0 += IN_LDS ? L : DL_TILE) {
      const int tn = IN_LDS ? L : min(DL_TILE, L - t0);
      const int* seg = in + t0;
      if (!IN_LDS) {
        __syncthreads();
        for (int k = tid; k < tn; k += T) tile[k] = in[t0 + k];
        __syncthreads();
        seg = tile;
      }
#pragma unroll 8
      for (int k = 0; k < tn; ++k) {
        const int v = seg[k];   // the same address in every lane: a broadcast read
#pragma unroll
        for (int u = 0; u < KPT; ++u) r[u] += v < key[u] ? 1 : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < KPT; ++u)
      if (p0 + u * T + tid < L) out[r[u]] = key[u];   // r < L: a rank among L distinct entries
  }
}

// ------------------------------------------------------------------------------------------
// The LDS form: steps 1-4 for ONE instance by one workgroup of KSL_T threads.
//   sm (int32, ksl_lds_bytes): start [M+1] | cursor [M] | bucket [E] | order [E] | long [E / 65 + 1]
// At most E / 65 segments hold more than 64 of the E entries; the order of `long` does not matter.
// ------------------------------------------------------------------------------------------
constexpr int KSL_T = 1024;
constexpr int KSL_KPT = 4;
constexpr size_t KSL_LDS_MAX = 160 * 1024 - 1024;   // dynamic LDS (the static wave partials beside it)

size_t ksl_lds_bytes(int E, int M) { return sizeof(int) * ((size_t)(M + 1) + M + 2 * (size_t)E + E / 65 + 1); }

struct KslLists {
  const int* start;
  const int* order;
};

__device__ __forceinline__ KslLists ksl_build(const int64_t* __restrict__ idx, int E, int M, int* sm) {
  __shared__ int s_nlong;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* s_start = sm;
  int* s_cursor = s_start + (M + 1);
  int* s_bucket = s_cursor + M;
  int* s_order = s_bucket + E;
  int* s_long = s_order + E;
  for (int i = tid; i <= M; i += KSL_T) s_start[i] = 0;
  if (tid == 0) s_nlong = 0;
  __syncthreads();
  for (int e = tid; e < E; e += KSL_T) {
    const int64_t j = idx[e];
    if (dl_valid(j, M)) atomicAdd(s_start + (int)j, 1);
  }
  __syncthreads();
  dl_scan<KSL_T>(s_start, s_cursor, M);
  __syncthreads();
  for (int e = tid; e < E; e += KSL_T) {
    const int64_t j = idx[e];
    if (!dl_valid(j, M)) continue;
    const int pos = atomicAdd(s_cursor + (int)j, 1);   // < start[j + 1] <= E: the counts were taken from the same idx
    s_bucket[pos] = e;
  }
  __syncthreads();
  for (int i = wave; i < M; i += KSL_T / 64) {
    const int s0 = s_start[i], L = s_start[i + 1] - s0;
    if (L > 64) {
      if (lane == 0) s_long[atomicAdd(&s_nlong, 1)] = i;
    } else if (L > 0) {
      dl_rank_short<true>(s_bucket + s0, s_order + s0, L, lane);
    }
  }
  __syncthreads();
  const int nlong = s_nlong;
  for (int q = 0; q < nlong; ++q) {
    const int s0 = s_start[s_long[q]], L = s_start[s_long[q] + 1] - s0;
    dl_rank_long<KSL_T, KSL_KPT, true>(s_bucket + s0, s_order + s0, L, nullptr);
  }
  __syncthreads();
  return KslLists{s_start, s_order};
}

}  // namespace
