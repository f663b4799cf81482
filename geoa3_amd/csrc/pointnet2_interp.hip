// PointNet++ feature propagation operators (gfx950): the three functions of the reference's vendored CUDA extension
// `pointnet2_ops._ext` that the FP module uses (Model/pointnet2_ops_lib/pointnet2_ops/_ext-src/src/bindings.cpp:6-8,
// interpolate.cpp:14-99, interpolate_gpu.cu:9-154): three_nn, three_interpolate, three_interpolate_grad.
// Same argument layouts ([B,n,3] point-major xyz, [B,C,m] channel-major features, int32 indices) so that the autograd
// Functions of pointnet2_utils.py:104-191 bind to them unchanged.
//
// Semantics kept from interpolate_gpu.cu:
//   * three_nn (:9-59): every unknown point scans the known points IN INDEX ORDER and keeps the three smallest squared
//     distances with the strict `<` cascade: equal distances stay in ascending index order, a NaN or +inf distance is never
//     selected, slots that were never filled (m < 3) come out as (+inf, 0).
//   * three_interpolate (:72-101): out = (p[i1] * w1 + p[i2] * w2) + p[i3] * w3.
//   * three_interpolate_grad (:116-143): grad_points[b][c][i] = sum over the (j, slot) with idx[b][j][slot] == i of
//     grad_out[b][c][j] * weight[b][j][slot].  The reference scatters with float atomics (the order of the sum, and so its
//     bits, change from run to run); here every destination sums ITS list in ascending (j, slot) order (dest_lists.h): the
//     same bits on every call and for every batch an instance is part of.
// Rounding: un-fused by default (every product and sum rounded to float32, the CPU oracle's order); GEOA3_PN2_CONTRACT (the
// *_ex entry points) selects fmaf(dz, dz, fmaf(dy, dy, dx * dx)) / fmaf(p3, w3, fmaf(p2, w2, p1 * w1)), what nvcc's default
// -fmad=true most likely made of :33 and :98-99 -- the convention of geoa3_pn2_ball_query_ex.
#include "dest_lists.h"
#include "pointnet_kernels.h"

namespace {

template <bool CT>
__device__ __forceinline__ float sq3(float dx, float dy, float dz) {
#pragma clang fp contract(off)
  if (CT) return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float s = xx + yy;
  return s + zz;
}

template <bool CT>
__device__ __forceinline__ float mix3(float p1, float w1, float p2, float w2, float p3, float w3) {
#pragma clang fp contract(off)
  if (CT) return __builtin_fmaf(p3, w3, __builtin_fmaf(p2, w2, p1 * w1));
  const float a = p1 * w1, b = p2 * w2, c = p3 * w3;
  const float s = a + b;
  return s + c;
}

// ------------------------------------------------------------------------------------------
// three_nn: grid (tiles of TNN_U unknown points, B), one unknown point per thread.  The known cloud passes through LDS in
// tiles of TNN_T points (x[], y[], z[] planes); every lane reads the SAME point (a broadcast read, no bank conflict) and the
// tiles follow each other in index order, so each thread sees k = 0 .. m-1 exactly as the reference's loop does.
// The running bests are floats initialised to +inf.  That is equivalent to the reference's `double best = 1e40`
// (interpolate_gpu.cu:27): a float d is below 1e40 exactly when it is finite, i.e. exactly when d < +inf; a NaN or +inf d
// fails both tests; and a slot nobody filled is written back as (float)1e40 = +inf (:51-53).
// The cascade sits behind `d < best3` (best1 <= best2 <= best3 always): after the first few points almost no k passes it in
// any lane, and the wave skips the cascade.
// 12 KB of LDS and ~24 registers: LDS and registers leave the full 8 waves per SIMD; the scan is bound by the ~12 vector
// instructions per (point, k).
// ------------------------------------------------------------------------------------------
constexpr int TNN_U = 128;    // unknown points per workgroup (= threads)
constexpr int TNN_T = 1024;   // known points per LDS tile

template <bool CT>
__global__ __launch_bounds__(TNN_U) void three_nn_kernel(const float* __restrict__ unknown, const float* __restrict__ known,
                                                         int n, int m, float* __restrict__ dist2, int32_t* __restrict__ idx) {
  __shared__ float s_x[TNN_T], s_y[TNN_T], s_z[TNN_T];
  const int b = blockIdx.y, tid = threadIdx.x, j = blockIdx.x * TNN_U + tid;
  const bool live = j < n;
  const float* U = unknown + ((size_t)b * n + (live ? j : n - 1)) * 3;
  const float ux = U[0], uy = U[1], uz = U[2];
  const float* K = known + (size_t)b * m * 3;
  float b1 = __builtin_inff(), b2 = b1, b3 = b1;
  int i1 = 0, i2 = 0, i3 = 0;
  for (int k0 = 0; k0 < m; k0 += TNN_T) {
    const int kn = min(TNN_T, m - k0);
    __syncthreads();
    for (int e = tid; e < kn; e += TNN_U) {
      const float* p = K + (size_t)(k0 + e) * 3;
      s_x[e] = p[0];
      s_y[e] = p[1];
      s_z[e] = p[2];
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kn; ++k) {
      const float d = sq3<CT>(ux - s_x[k], uy - s_y[k], uz - s_z[k]);
      if (d < b3) {
        const int kk = k0 + k;
        if (d < b1) {
          b3 = b2; i3 = i2;
          b2 = b1; i2 = i1;
          b1 = d;  i1 = kk;
        } else if (d < b2) {
          b3 = b2; i3 = i2;
          b2 = d;  i2 = kk;
        } else {
          b3 = d;  i3 = kk;
        }
      }
    }
  }
  if (!live) return;
  float* D = dist2 + ((size_t)b * n + j) * 3;
  int32_t* I = idx + ((size_t)b * n + j) * 3;
  D[0] = b1; D[1] = b2; D[2] = b3;
  I[0] = i1; I[1] = i2; I[2] = i3;
}

// ------------------------------------------------------------------------------------------
// three_interpolate: grid (tiles of 256 unknown points, groups of TI_CG channels, B), one unknown point per thread.  The
// thread loads its idx / weight row ONCE and walks the channels of its group: per channel three gathered reads of the
// [m]-long feature row (cache hits: the row is shared by the whole workgroup) and one store, coalesced along n.
// An index outside [0, m) is the caller's error (the reference reads out of bounds); it is neither wrapped nor clamped
// nor read: the output element is NaN.
// ------------------------------------------------------------------------------------------
constexpr int TI_CG = 32;   // channels per workgroup

template <bool CT>
__global__ __launch_bounds__(256) void three_interpolate_kernel(const float* __restrict__ points, const int32_t* __restrict__ idx,
                                                                const float* __restrict__ weight, int C, int m, int n,
                                                                float* __restrict__ out) {
  const int b = blockIdx.z, c0 = blockIdx.y * TI_CG, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int32_t* I = idx + ((size_t)b * n + j) * 3;
  const float* W = weight + ((size_t)b * n + j) * 3;
  const int i1 = I[0], i2 = I[1], i3 = I[2];
  const float w1 = W[0], w2 = W[1], w3 = W[2];
  const bool ok = (unsigned)i1 < (unsigned)m && (unsigned)i2 < (unsigned)m && (unsigned)i3 < (unsigned)m;
  const int c1 = min(c0 + TI_CG, C);
  for (int c = c0; c < c1; ++c) {
    const float* P = points + ((size_t)b * C + c) * m;
    out[((size_t)b * C + c) * n + j] = ok ? mix3<CT>(P[i1], w1, P[i2], w2, P[i3], w3) : __builtin_nanf("");
  }
}

// ------------------------------------------------------------------------------------------
// three_interpolate_grad: the 3n entries e = 3 j + slot of an instance are sorted by destination into the caller's scratch
// (launch_dest_lists, dest_lists.h), then one thread per (destination, group of TG_CG channels) sums its list in ascending e:
//   tig_sum:  grad_points[b][c][i] = sum over order[start[i] .. start[i+1]) of fl(grad_out[b][c][e / 3] * weight[b][e]),
//             each product rounded, added in list order; an empty list writes +0.0.  Every element is written.
// No float atomics; a NaN or inf product is added like any other value and comes out as NaN / inf.
// An index outside [0, m) (the caller's error, as in the reference) is not wrapped: its entry is in no list.
// ------------------------------------------------------------------------------------------
constexpr int TG_CG = 8;   // channels per thread of tig_sum

__global__ __launch_bounds__(256) void tig_sum_kernel(const float* __restrict__ grad_out, const float* __restrict__ weight,
                                                      const int* __restrict__ start, const int* __restrict__ order, int C, int n,
                                                      int m, float* __restrict__ grad_points) {
#pragma clang fp contract(off)
  const int b = blockIdx.z, c0 = blockIdx.y * TG_CG, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int* S = start + (size_t)b * (m + 1);
  const int s0 = S[i], s1 = S[i + 1];
  const int* O = order + (size_t)b * 3 * n;
  const float* W = weight + (size_t)b * 3 * n;
  const float* G = grad_out + ((size_t)b * C + c0) * n;
  const int nc = min(TG_CG, C - c0);
  float acc[TG_CG];
#pragma unroll
  for (int c = 0; c < TG_CG; ++c) acc[c] = 0.f;
  for (int q = s0; q < s1; ++q) {
    const int e = O[q];
    const int j = e / 3;
    const float w = W[e];
#pragma unroll
    for (int c = 0; c < TG_CG; ++c) {
      if (c < nc) {
        const float t = G[(size_t)c * n + j] * w;
        acc[c] = acc[c] + t;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < TG_CG; ++c)
    if (c < nc) grad_points[((size_t)b * C + c0 + c) * m + i] = acc[c];
}

constexpr int MAX_GRID_YZ = 65535;

}  // namespace

static int three_nn_impl(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx, bool contract,
                         void* stream) {
  if (!unknown || !known || !dist2 || !idx || B <= 0 || n <= 0 || m <= 0 || B > MAX_GRID_YZ) return GEOA3_EINVAL;
  if (n > INT_MAX - TNN_U || m > INT_MAX - TNN_T) return GEOA3_EINVAL;   // (the tile loops count in int)
  auto kern = contract ? three_nn_kernel<true> : three_nn_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((n + TNN_U - 1) / TNN_U, B), dim3(TNN_U), 0, geoa3_stream(stream), unknown, known, n, m, dist2,
                     idx);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
extern "C" int geoa3_pn2_three_nn(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                                  void* stream) {
  return three_nn_impl(unknown, known, B, n, m, dist2, idx, false, stream);
}
extern "C" int geoa3_pn2_three_nn_ex(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                                     int flags, void* stream) {
  if (flags & ~GEOA3_PN2_CONTRACT) return GEOA3_EINVAL;
  return three_nn_impl(unknown, known, B, n, m, dist2, idx, (flags & GEOA3_PN2_CONTRACT) != 0, stream);
}
extern "C" int geoa3_pn2_three_nn_tile(int* known_tile, int* unknown_tile) {
  if (known_tile) *known_tile = TNN_T;
  if (unknown_tile) *unknown_tile = TNN_U;
  return GEOA3_OK;
}

static int three_interpolate_impl(const float* points, const int32_t* idx, const float* weight, int B, int C, int m, int n,
                                  float* out, bool contract, void* stream) {
  if (!points || !idx || !weight || !out || B <= 0 || C <= 0 || m <= 0 || n <= 0 || n > INT_MAX - 256 || B > MAX_GRID_YZ)
    return GEOA3_EINVAL;
  const int cg = (C + TI_CG - 1) / TI_CG;
  if (cg > MAX_GRID_YZ) return GEOA3_ENOSUPPORT;
  auto kern = contract ? three_interpolate_kernel<true> : three_interpolate_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((n + 255) / 256, cg, B), dim3(256), 0, geoa3_stream(stream), points, idx, weight, C, m, n, out);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
extern "C" int geoa3_pn2_three_interpolate(const float* points, const int32_t* idx, const float* weight, int B, int C, int m,
                                           int n, float* out, void* stream) {
  return three_interpolate_impl(points, idx, weight, B, C, m, n, out, false, stream);
}
extern "C" int geoa3_pn2_three_interpolate_ex(const float* points, const int32_t* idx, const float* weight, int B, int C, int m,
                                              int n, float* out, int flags, void* stream) {
  if (flags & ~GEOA3_PN2_CONTRACT) return GEOA3_EINVAL;
  return three_interpolate_impl(points, idx, weight, B, C, m, n, out, (flags & GEOA3_PN2_CONTRACT) != 0, stream);
}

extern "C" int64_t geoa3_pn2_three_interpolate_scratch_bytes(int B, int n, int m) {
  if (B <= 0 || n <= 0 || m <= 0 || n > (INT_MAX - 255) / 3 || m > INT_MAX - 256) return -1;
  return (int64_t)dest_lists_scratch_bytes(B, 3 * n, m);
}

extern "C" int geoa3_pn2_three_interpolate_grad(const float* grad_out, const int32_t* idx, const float* weight, int B, int C,
                                                int n, int m, float* grad_points, void* scratch, void* stream) {
  if (!grad_out || !idx || !weight || !grad_points || !scratch || B <= 0 || C <= 0 || B > MAX_GRID_YZ) return GEOA3_EINVAL;
  if (geoa3_pn2_three_interpolate_scratch_bytes(B, n, m) < 0) return GEOA3_EINVAL;
  const int cg = (C + TG_CG - 1) / TG_CG;
  if (cg > MAX_GRID_YZ) return GEOA3_ENOSUPPORT;
  hipStream_t s = geoa3_stream(stream);
  const int *start = nullptr, *order = nullptr;
  const int rb = launch_dest_lists(idx, B, 3 * n, m, scratch, s, &start, &order);
  if (rb != GEOA3_OK) return rb;
  hipLaunchKernelGGL(tig_sum_kernel, dim3((m + 255) / 256, cg, B), dim3(256), 0, s, grad_out, weight, start, order, C, n, m,
                     grad_points);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
