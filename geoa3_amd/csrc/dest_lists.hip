// The scratch form of the destination lists (dest_lists.h, steps 1-4): four launches over the whole batch.
// count, place and sort take their instance from blockIdx.y, stepping by gridDim.y (the grid's y dimension ends at 65535),
// and the entry / destination inside the instance from x: no division by E, and B E or B M may pass 2^31.
#include "dest_lists.h"

namespace {

constexpr int DL_KPT = 4;   // entries a thread ranks per pass over a long segment (256 threads: 1024 per pass)
constexpr int DL_MAX_GRID_Y = 65535;

template <typename I>
__global__ __launch_bounds__(256) void dl_count_kernel(const I* __restrict__ idx, int B, int E, int M, int* __restrict__ start) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const I j = idx[(size_t)b * E + e];
    if (dl_valid(j, M)) atomicAdd(start + (size_t)b * (M + 1) + (int)j, 1);
  }
}

// one workgroup per instance
__global__ __launch_bounds__(256) void dl_scan_kernel(int* __restrict__ start, int* __restrict__ cursor, int M) {
  const size_t b = blockIdx.x;
  dl_scan<256>(start + b * (M + 1), cursor + b * M, M);
}

template <typename I>
__global__ __launch_bounds__(256) void dl_place_kernel(const I* __restrict__ idx, int B, int E, int M, int* __restrict__ cursor,
                                                       int* __restrict__ bucket) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const I j = idx[(size_t)b * E + e];
    if (!dl_valid(j, M)) continue;
    const int pos = atomicAdd(cursor + (size_t)b * M + (int)j, 1);   // < start[j + 1] <= E: the counts were taken from the same idx
    bucket[(size_t)b * E + pos] = e;
  }
}

// A workgroup serves four destinations of ONE instance: a wavefront each while they hold up to 64 entries, the whole
// workgroup for a longer one.  Every wavefront takes all five bounds -- lanes 0-4 load them, readlane hands them round as
// scalars -- so the branches around dl_rank_long are uniform; a destination past M is an empty segment.  (Loaded as
// scalars, five s_load behind the instance's address arithmetic, the kernel takes 15.6 us instead of 13.4 at B = 16,
// M = 4096 and lists of three, where its time is one workgroup's chain of dependent loads times the workgroups per CU.)
__global__ __launch_bounds__(256) void dl_sort_kernel(const int* __restrict__ start, const int* __restrict__ bucket,
                                                      int* __restrict__ order, int B, int E, int M) {
  __shared__ int s_tile[DL_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i0 = blockIdx.x * 4;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int* in = bucket + (size_t)b * E;
    int* out = order + (size_t)b * E;
    const int v = start[(size_t)b * (M + 1) + min(i0 + min(lane, 4), M)];
    int bound[5];
#pragma unroll
    for (int w = 0; w < 5; ++w) bound[w] = __builtin_amdgcn_readlane(v, w);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int s0 = bound[w], L = bound[w + 1] - s0;
      if (L > 64)
        dl_rank_long<256, DL_KPT, false>(in + s0, out + s0, L, s_tile);
      else if (L > 0 && w == wave)
        dl_rank_short<false>(in + s0, out + s0, L, lane);
    }
  }
}

}  // namespace

size_t dest_lists_scratch_bytes(int B, int E, int M) {
  return sizeof(int) * (size_t)B * ((size_t)(M + 1) + M + 2 * (size_t)E);
}

template <typename I>
int launch_dest_lists(const I* idx, int B, int E, int M, void* scratch, hipStream_t s, const int** start_out,
                      const int** order_out) {
  int* start = static_cast<int*>(scratch);
  int* cursor = start + (size_t)B * (M + 1);
  int* bucket = cursor + (size_t)B * M;
  int* order = bucket + (size_t)B * E;
  const int gy = B < DL_MAX_GRID_Y ? B : DL_MAX_GRID_Y;
  if (hipMemsetAsync(start, 0, (size_t)B * (M + 1) * sizeof(int), s) != hipSuccess) return GEOA3_ELAUNCH;
  hipLaunchKernelGGL(dl_count_kernel<I>, dim3((E + 255) / 256, gy), dim3(256), 0, s, idx, B, E, M, start);
  hipLaunchKernelGGL(dl_scan_kernel, dim3(B), dim3(256), 0, s, start, cursor, M);
  hipLaunchKernelGGL(dl_place_kernel<I>, dim3((E + 255) / 256, gy), dim3(256), 0, s, idx, B, E, M, cursor, bucket);
  hipLaunchKernelGGL(dl_sort_kernel, dim3((M + 3) / 4, gy), dim3(256), 0, s, start, bucket, order, B, E, M);
  *start_out = start;
  *order_out = order;
  return GEOA3_OK;
}
template int launch_dest_lists<int32_t>(const int32_t*, int, int, int, void*, hipStream_t, const int**, const int**);
template int launch_dest_lists<int64_t>(const int64_t*, int, int, int, void*, hipStream_t, const int**, const int**);
