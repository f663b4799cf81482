// The neighbour half of an eval-mode EdgeConv layer (DGCNN), fused (gfx950).  The layer is
//   y[c,i] = max over the k neighbours j of i of  LeakyReLU_0.2( BN( W [x_j - x_i ; x_i] ) )[c].
// With the BatchNorm scale s and shift t folded and W = [W_a | W_b], the pre-activation of edge (i, j) is U[j] + V[i] + t,
// U = (s W_a) x and V = (s (W_b - W_a)) x: two GEMMs per POINT (the caller's).  LeakyReLU and float32 addition are monotone,
// so the maximum over the neighbours is reached at an arg-max of U[j]: the [B,2C,N,k] edge tensor never exists.
//
//   edge_max       arg[i,c] = the first slot s that maximises U[idx[i,s], c]  (a NaN, once met, stays: torch.max's rule)
//                  y[c,i]   = lrelu( fl( fl(U[idx[i,arg],c] + V[i,c]) + t[c] ) ),  lrelu(a) = a > 0 ? a : fl(0.2f a)
//                  An index outside [0,N) is never dereferenced: the point's y is NaN, arg its first such slot.
//   edge_max_grad  g'[i,c]  = y[c,i] > 0 ? g[c,i] : fl(0.2f g[c,i])
//                  dV[i,c]  = g'[i,c]
//                  dU[j,c]  = the sequential float32 sum, from +0.0, of the g'[i,c] with idx[i,arg[i,c]] == j, in ascending
//                             (i, slot) order: the destination lists of idx [B, N k] are built once per call (dest_lists.h),
//                             then every (destination, channel) walks its list and takes the entries whose slot is arg[i,c].
// No float atomics: a float32 loop on the CPU reproduces every element bit for bit, whatever the batch.
// Layouts: U, V, dU, dV, arg [B,N,C'] (point-major: a wavefront's 64 channels are 256 consecutive bytes); y, g [B,C',N] (what
// the next Conv1d takes), transposed through an LDS tile of EC_P points x EC_C channels.
#include "dest_lists.h"

namespace {

constexpr int EC_P = 32;    // points per tile
constexpr int EC_C = 64;    // channels per tile: one wavefront across
constexpr int EC_T = 256;
constexpr int EC_DJ = EC_T / EC_C;   // destinations per workgroup of edge_du_kernel

__device__ __forceinline__ float ec_lrelu(float a) {
#pragma clang fp contract(off)
  return a > 0.f ? a : a * 0.2f;
}

__global__ __launch_bounds__(EC_T) void edge_max_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                        const float* __restrict__ t, const int64_t* __restrict__ idx, int N,
                                                        int C, int K, float* __restrict__ y, int32_t* __restrict__ arg) {
#pragma clang fp contract(off)
  __shared__ float s_y[EC_C][EC_P + 1];
  const int b = blockIdx.z, i0 = blockIdx.x * EC_P, c0 = blockIdx.y * EC_C, tid = threadIdx.x;
  const float* Ub = U + (size_t)b * N * C;
  {
    const int cl = tid & (EC_C - 1), c = c0 + cl;
    for (int pl = tid / EC_C; pl < EC_P; pl += EC_T / EC_C) {
      const int i = i0 + pl;
      if (i >= N || c >= C) continue;
      const size_t row = (size_t)b * N + i;
      const int64_t* I = idx + row * K;
      float best = 0.f;
      int a = 0;
      bool bad = false;
      for (int s = 0; s < K; ++s) {
        const int64_t j = I[s];
        if (!dl_valid(j, N)) {
          a = s;
          bad = true;
          break;
        }
        const float u = Ub[(size_t)j * C + c];
        if (s == 0 || u > best || (u != u && best == best)) {
          best = u;
          a = s;
        }
      }
      float yv = __builtin_nanf("");
      if (!bad) {
        float pre = best + V[row * C + c];
        pre = pre + t[c];
        yv = ec_lrelu(pre);
      }
      arg[row * C + c] = a;
      s_y[cl][pl] = yv;
    }
  }
  __syncthreads();
  const int pl = tid & (EC_P - 1), i = i0 + pl;
  for (int cl = tid / EC_P; cl < EC_C; cl += EC_T / EC_P) {
    const int c = c0 + cl;
    if (i < N && c < C) y[((size_t)b * C + c) * N + i] = s_y[cl][pl];
  }
}

// dV [B,N,C] = g' (g, y [B,C,N])
__global__ __launch_bounds__(EC_T) void edge_dv_kernel(const float* __restrict__ g, const float* __restrict__ y, int N, int C,
                                                       float* __restrict__ dV) {
#pragma clang fp contract(off)
  __shared__ float s_g[EC_C][EC_P + 1];
  const int b = blockIdx.z, i0 = blockIdx.x * EC_P, c0 = blockIdx.y * EC_C, tid = threadIdx.x;
  {
    const int pl = tid & (EC_P - 1), i = i0 + pl;
    for (int cl = tid / EC_P; cl < EC_C; cl += EC_T / EC_P) {
      const int c = c0 + cl;
      if (i >= N || c >= C) continue;
      const size_t o = ((size_t)b * C + c) * N + i;
      const float gv = g[o];
      s_g[cl][pl] = y[o] > 0.f ? gv : gv * 0.2f;
    }
  }
  __syncthreads();
  const int cl = tid & (EC_C - 1), c = c0 + cl;
  for (int pl = tid / EC_C; pl < EC_P; pl += EC_T / EC_C) {
    const int i = i0 + pl;
    if (i < N && c < C) dV[((size_t)b * N + i) * C + c] = s_g[cl][pl];
  }
}

// dU: one thread per (destination, channel), a wavefront across 64 channels of one destination
__global__ __launch_bounds__(EC_T) void edge_du_kernel(const float* __restrict__ dV, const int32_t* __restrict__ arg,
                                                       const int* __restrict__ start, const int* __restrict__ order, int N,
                                                       int C, int K, float* __restrict__ dU) {
#pragma clang fp contract(off)
  const int b = blockIdx.z, tid = threadIdx.x;
  const int j = blockIdx.x * EC_DJ + tid / EC_C, c = blockIdx.y * EC_C + (tid & (EC_C - 1));
  if (j >= N || c >= C) return;
  const int* S = start + (size_t)b * (N + 1);
  const int s0 = S[j], s1 = S[j + 1];
  const int* O = order + (size_t)b * N * K;
  const size_t base = (size_t)b * N * C + c;
  float acc = 0.f;
  for (int q = s0; q < s1; ++q) {
    const int e = O[q];
    const int i = e / K, slot = e - i * K;
    const size_t o = base + (size_t)i * C;
    if (arg[o] == slot) acc = acc + dV[o];
  }
  dU[base + (size_t)j * C] = acc;
}

// sizes every entry accepts
int ec_sizes(int B, int N, int C, int K) {
  if (B <= 0 || N <= 0 || C <= 0 || K < 1) return GEOA3_EINVAL;
  if ((int64_t)N * K > (int64_t)INT_MAX - 256 || B > 65535 || (C - 1) / EC_C + 1 > 65535) return GEOA3_ENOSUPPORT;
  return GEOA3_OK;
}

}  // namespace

extern "C" int geoa3_edge_max(const float* U, const float* V, const float* t, const int64_t* idx, int B, int N, int C, int K,
                              float* y, int32_t* arg, void* stream) {
  if (!U || !V || !t || !idx || !y || !arg) return GEOA3_EINVAL;
  const int rc = ec_sizes(B, N, C, K);
  if (rc != GEOA3_OK) return rc;
  const dim3 grid((N + EC_P - 1) / EC_P, (C + EC_C - 1) / EC_C, B);
  hipLaunchKernelGGL(edge_max_kernel, grid, dim3(EC_T), 0, geoa3_stream(stream), U, V, t, idx, N, C, K, y, arg);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int64_t geoa3_edge_max_scratch_bytes(int B, int N, int K) {
  if (ec_sizes(B, N, 1, K) != GEOA3_OK) return -1;
  return (int64_t)dest_lists_scratch_bytes(B, N * K, N);
}

extern "C" int geoa3_edge_max_grad(const float* g, const float* y, const int32_t* arg, const int64_t* idx, int B, int N, int C,
                                   int K, float* dU, float* dV, void* scratch, void* stream) {
  if (!g || !y || !arg || !idx || !dU || !dV || !scratch) return GEOA3_EINVAL;
  const int rc = ec_sizes(B, N, C, K);
  if (rc != GEOA3_OK) return rc;
  hipStream_t s = geoa3_stream(stream);
  const int cg = (C + EC_C - 1) / EC_C;
  const int *start = nullptr, *order = nullptr;   // the lists first: when they fail, neither output has been written
  const int rb = launch_dest_lists(idx, B, N * K, N, scratch, s, &start, &order);
  if (rb != GEOA3_OK) return rb;
  hipLaunchKernelGGL(edge_dv_kernel, dim3((N + EC_P - 1) / EC_P, cg, B), dim3(EC_T), 0, s, g, y, N, C, dV);
  GEOA3_CHECK_LAUNCH();
  hipLaunchKernelGGL(edge_du_kernel, dim3((N + EC_DJ - 1) / EC_DJ, cg, B), dim3(EC_T), 0, s, dV, arg, start, order, N, C, K, dU);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
