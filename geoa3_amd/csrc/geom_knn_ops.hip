// pytorch3d.ops.knn_gather and the backward passes of knn_gather / knn_points (gfx950), in the operators' OWN layouts:
// point-major float32 ([B,M,U] features, [B,N,3] points) and int64 indices, as the operators hand them over
// (Lib/loss_utils.py:58,71,78, Attacker/geoA3_attack.py:66,81, Lib/utility.py:46,97,121).
//
//   knn_gather        out[b,l,k,:] = x[b, idx[b,l,k], :]                                   (pure data movement)
//   knn_gather_grad   gx[b,j,c]    = sum of g[b,l,k,c] over the entries with idx[b,l,k] == j
//   knn_points_grad   t(i,k,c)     = fl( fl(2 gd[i,k]) * fl(p1[i,c] - p2[idx[i,k],c]) )    (pytorch3d's knn backward)
//                     g1[i,c]      = sum over k of  t(i,k,c)
//                     g2[j,c]      = sum of -t(i,k,c) over the entries with idx[i,k] == j
//
// pytorch3d and torch.scatter_add sum these with float atomics: the order, and so the bits, change from run to run.
// Here EVERY sum is sequential in float32, starts from +0.0f and runs in ascending entry number e = l K + k (g1: ascending
// k), so a plain float32 loop on the CPU reproduces every element bit for bit, whatever the batch an instance is part of.
//
// The scatter: the E = L K entries of an instance are sorted by destination into lists (dest_lists.h: the scheme, its
// invariants and both of its forms), then one thread per (destination, group of components) walks its list (kgg_sum /
// kpg_g2; an empty list writes +0.0; every element is written).  When an instance's tables fit the LDS of one compute unit
// (ksl_lds_bytes <= KSL_LDS_MAX: every shape of the reference's objective, e.g. M = 1024, E = 1024 x 17) ONE workgroup per
// instance builds them there and sums in the same launch (*_lds_kernel; `scratch` is not touched); larger instances take the
// lists from launch_dest_lists through `scratch`.  The same bits either way.
// An index outside [0, M) is the caller's error: it is neither wrapped nor clamped nor dereferenced -- the gather writes NaN
// to that element, the backward passes drop the term (the entry is in no list).
// No float atomics; a NaN or inf term is added like any other value.
#include "dest_lists.h"

namespace {

constexpr int KGG_CG = 4;        // components per thread of kgg_sum
constexpr int MAX_GRID_Y = 65535;

// ------------------------------------------------------------------------------------------
// knn_gather: one thread per output element (flat over B E U: the stores are coalesced, the U reads of an entry are
// consecutive).  `total` < 2^32 (every shape of the reference by orders of magnitude) divides in 32 bits.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_gather_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx, int M,
                                                         int E, int U, uint64_t total, float* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x; f < total; f += stride) {
    unsigned ent, c;   // ent < B E < 2^31
    if (total <= 0xffffffffull) {
      ent = (unsigned)f / (unsigned)U;
      c = (unsigned)f - ent * (unsigned)U;
    } else {
      ent = (unsigned)(f / (unsigned)U);
      c = (unsigned)(f - (uint64_t)ent * (unsigned)U);
    }
    const unsigned b = ent / (unsigned)E;
    const int64_t j = idx[ent];
    out[f] = dl_valid(j, M) ? x[((size_t)b * M + (size_t)j) * U + c] : __builtin_nanf("");
  }
}

// U = 3 (points and normals: every call site of the reference): one thread per ENTRY -- one index read, one 12-byte row in,
// one out; a wavefront's rows are 768 consecutive bytes.
__global__ __launch_bounds__(256) void knn_gather3_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx, int M,
                                                          int E, int BE, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= BE) return;
  const int b = t / E;
  const int64_t j = idx[t];
  float v0 = __builtin_nanf(""), v1 = v0, v2 = v0;
  if (dl_valid(j, M)) {
    const float* X = x + ((size_t)b * M + (size_t)j) * 3;
    v0 = X[0];
    v1 = X[1];
    v2 = X[2];
  }
  float* O = out + (size_t)t * 3;
  O[0] = v0;
  O[1] = v1;
  O[2] = v2;
}

// ------------------------------------------------------------------------------------------
// the sums: one thread per destination (x: flat over B M) and, for the gather's gradient, group of KGG_CG components (y)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kgg_sum_kernel(const float* __restrict__ g, const int* __restrict__ start,
                                                      const int* __restrict__ order, int E, int M, int U, int BM,
                                                      float* __restrict__ gx) {
#pragma clang fp contract(off)
  const int d = blockIdx.x * 256 + threadIdx.x, c0 = blockIdx.y * KGG_CG;
  if (d >= BM) return;
  const int b = d / M, i = d - b * M;
  const int* S = start + (size_t)b * (M + 1);
  const int s0 = S[i], s1 = S[i + 1];
  const int* O = order + (size_t)b * E;
  const float* G = g + (size_t)b * E * U + c0;
  const int nc = min(KGG_CG, U - c0);
  float acc[KGG_CG];
#pragma unroll
  for (int c = 0; c < KGG_CG; ++c) acc[c] = 0.f;
  for (int q = s0; q < s1; ++q) {
    const float* Ge = G + (size_t)O[q] * U;
#pragma unroll
    for (int c = 0; c < KGG_CG; ++c)
      if (c < nc) acc[c] = acc[c] + Ge[c];
  }
  float* X = gx + (size_t)d * U + c0;
#pragma unroll
  for (int c = 0; c < KGG_CG; ++c)
    if (c < nc) X[c] = acc[c];
}

// the term of pytorch3d's knn backward, every operation rounded to float32 on its own (no fused multiply-add: the CPU
// restatement of tests/_knn_ops_ref.py is three numpy float32 operations)
__device__ __forceinline__ float kpg_term(float gd, float a, float b) {
#pragma clang fp contract(off)
  const float w = 2.0f * gd;
  const float df = a - b;
  return w * df;
}

// g1[b,i,:] = sum over k (ascending) of t(i,k,:): one thread per query
__global__ __launch_bounds__(256) void kpg_g1_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                     const int64_t* __restrict__ idx, const float* __restrict__ gd, int N1,
                                                     int N2, int K, int BN1, float* __restrict__ g1) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;   // flat query number, < B N1 <= B E
  if (t >= BN1) return;
  const int b = t / N1;
  const float* A = p1 + (size_t)t * 3;
  const float ax = A[0], ay = A[1], az = A[2];
  const float* R = p2 + (size_t)b * N2 * 3;
  const int64_t* I = idx + (size_t)t * K;
  const float* GD = gd + (size_t)t * K;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int k = 0; k < K; ++k) {
    const int64_t j = I[k];
    if (!dl_valid(j, N2)) continue;
    const float* Q = R + (size_t)j * 3;
    const float w = GD[k];
    sx = sx + kpg_term(w, ax, Q[0]);
    sy = sy + kpg_term(w, ay, Q[1]);
    sz = sz + kpg_term(w, az, Q[2]);
  }
  float* out = g1 + (size_t)t * 3;
  out[0] = sx;
  out[1] = sy;
  out[2] = sz;
}

// g2[b,j,:] = sum over j's list (ascending e = i K + k) of -t(i,k,:): one thread per searched point
__global__ __launch_bounds__(256) void kpg_g2_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                     const float* __restrict__ gd, const int* __restrict__ start,
                                                     const int* __restrict__ order, int N1, int N2, int K, int BN2,
                                                     float* __restrict__ g2) {
#pragma clang fp contract(off)
  const int d = blockIdx.x * 256 + threadIdx.x;   // flat destination number
  if (d >= BN2) return;
  const int b = d / N2, j = d - b * N2;
  const int E = N1 * K;
  const int* S = start + (size_t)b * (N2 + 1);
  const int s0 = S[j], s1 = S[j + 1];
  const int* O = order + (size_t)b * E;
  const float* A = p1 + (size_t)b * N1 * 3;
  const float* GD = gd + (size_t)b * E;
  const float* Q = p2 + (size_t)d * 3;
  const float qx = Q[0], qy = Q[1], qz = Q[2];
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int q = s0; q < s1; ++q) {
    const int e = O[q];
    const float* P = A + (size_t)(e / K) * 3;
    const float w = GD[e];
    sx = sx - kpg_term(w, P[0], qx);   // fl(s + (-t)) == fl(s - t)
    sy = sy - kpg_term(w, P[1], qy);
    sz = sz - kpg_term(w, P[2], qz);
  }
  float* out = g2 + (size_t)d * 3;
  out[0] = sx;
  out[1] = sy;
  out[2] = sz;
}

// ------------------------------------------------------------------------------------------
// the same sums behind ksl_build: one workgroup of KSL_T threads per instance, its lists in LDS
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KSL_T) void kgg_lds_kernel(const float* __restrict__ g, const int64_t* __restrict__ idx, int E,
                                                        int M, int U, float* __restrict__ gx) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) int ksl_sm[];
  const int b = blockIdx.x;
  const KslLists ls = ksl_build(idx + (size_t)b * E, E, M, ksl_sm);
  const int cg = (U - 1) / KGG_CG + 1;
  const float* G = g + (size_t)b * E * U;
  float* X = gx + (size_t)b * M * U;
  for (int w = threadIdx.x; w < M * cg; w += KSL_T) {   // (M cg fits an int: checked at the launch)
    const int i = w / cg, c0 = (w - i * cg) * KGG_CG;
    const int s0 = ls.start[i], s1 = ls.start[i + 1];
    const int nc = min(KGG_CG, U - c0);
    float acc[KGG_CG];
#pragma unroll
    for (int c = 0; c < KGG_CG; ++c) acc[c] = 0.f;
    for (int q = s0; q < s1; ++q) {
      const float* Ge = G + (size_t)ls.order[q] * U + c0;
#pragma unroll
      for (int c = 0; c < KGG_CG; ++c)
        if (c < nc) acc[c] = acc[c] + Ge[c];
    }
#pragma unroll
    for (int c = 0; c < KGG_CG; ++c)
      if (c < nc) X[(size_t)i * U + c0 + c] = acc[c];
  }
}

__global__ __launch_bounds__(KSL_T) void kpg_g2_lds_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                           const int64_t* __restrict__ idx, const float* __restrict__ gd,
                                                           int N1, int N2, int K, float* __restrict__ g2) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) int ksl_sm[];
  const int b = blockIdx.x, E = N1 * K;
  const KslLists ls = ksl_build(idx + (size_t)b * E, E, N2, ksl_sm);
  const float* A = p1 + (size_t)b * N1 * 3;
  const float* GD = gd + (size_t)b * E;
  for (int j = threadIdx.x; j < N2; j += KSL_T) {
    const float* Q = p2 + ((size_t)b * N2 + j) * 3;
    const float qx = Q[0], qy = Q[1], qz = Q[2];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int q = ls.start[j]; q < ls.start[j + 1]; ++q) {
      const int e = ls.order[q];
      const float* P = A + (size_t)(e / K) * 3;
      const float w = GD[e];
      sx = sx - kpg_term(w, P[0], qx);   // fl(s + (-t)) == fl(s - t)
      sy = sy - kpg_term(w, P[1], qy);
      sz = sz - kpg_term(w, P[2], qz);
    }
    float* out = g2 + ((size_t)b * N2 + j) * 3;
    out[0] = sx;
    out[1] = sy;
    out[2] = sz;
  }
}

// sizes every entry accepts: E = L K entries per instance, B E < 2^31, B (M + 1) < 2^31
int kso_sizes(int B, int M, int L, int K, int* E) {
  if (B <= 0 || M <= 0 || L <= 0 || K < 1) return GEOA3_EINVAL;
  const int64_t e = (int64_t)L * K;
  if (e * B > (int64_t)INT_MAX - 256 || (int64_t)B * ((int64_t)M + 1) > (int64_t)INT_MAX - 256) return GEOA3_ENOSUPPORT;
  *E = (int)e;
  return GEOA3_OK;
}

}  // namespace

extern "C" int geoa3_knn_gather(const float* x, const int64_t* idx, int B, int M, int L, int K, int U, float* out,
                                void* stream) {
  if (!x || !idx || !out || U < 1) return GEOA3_EINVAL;
  int E = 0;
  const int rc = kso_sizes(B, M, L, K, &E);
  if (rc != GEOA3_OK) return rc;
  if (U == 3) {
    const int BE = B * E;
    hipLaunchKernelGGL(knn_gather3_kernel, dim3((BE + 255) / 256), dim3(256), 0, geoa3_stream(stream), x, idx, M, E, BE, out);
    GEOA3_CHECK_LAUNCH();
    return GEOA3_OK;
  }
  const uint64_t total = (uint64_t)B * E * U;
  const uint64_t blocks = (total + 255) / 256;
  const unsigned grid = (unsigned)(blocks < (1u << 22) ? blocks : (1u << 22));   // (larger: the kernel strides)
  hipLaunchKernelGGL(knn_gather_kernel, dim3(grid), dim3(256), 0, geoa3_stream(stream), x, idx, M, E, U, total, out);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int64_t geoa3_knn_scatter_scratch_bytes(int B, int E, int M) {
  int e = 0;
  if (E <= 0 || kso_sizes(B, M, E, 1, &e) != GEOA3_OK) return -1;
  return (int64_t)dest_lists_scratch_bytes(B, E, M);
}

extern "C" int geoa3_knn_gather_grad(const float* g, const int64_t* idx, int B, int M, int L, int K, int U, float* gx,
                                     void* scratch, void* stream) {
  if (!g || !idx || !gx || !scratch || U < 1) return GEOA3_EINVAL;
  int E = 0;
  const int rc = kso_sizes(B, M, L, K, &E);
  if (rc != GEOA3_OK) return rc;
  const int cg = (U - 1) / KGG_CG + 1;
  if (cg > MAX_GRID_Y) return GEOA3_ENOSUPPORT;
  hipStream_t s = geoa3_stream(stream);
  const size_t lds = ksl_lds_bytes(E, M);
  if (lds <= KSL_LDS_MAX && (int64_t)M * cg <= INT_MAX) {
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kgg_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kgg_lds_kernel, dim3(B), dim3(KSL_T), lds, s, g, idx, E, M, U, gx);
    GEOA3_CHECK_LAUNCH();
    return GEOA3_OK;
  }
  const int *start = nullptr, *order = nullptr;
  const int rb = launch_dest_lists(idx, B, E, M, scratch, s, &start, &order);
  if (rb != GEOA3_OK) return rb;
  const int BM = B * M;
  hipLaunchKernelGGL(kgg_sum_kernel, dim3((BM + 255) / 256, cg), dim3(256), 0, s, g, start, order, E, M, U, BM, gx);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_knn_points_grad(const float* p1, const float* p2, const int64_t* idx, const float* gd, int B, int N1,
                                     int N2, int K, float* g1, float* g2, void* scratch, void* stream) {
  if (!p1 || !p2 || !idx || !gd || (!g1 && !g2) || (g2 && !scratch)) return GEOA3_EINVAL;
  int E = 0;
  const int rc = kso_sizes(B, N2, N1, K, &E);
  if (rc != GEOA3_OK) return rc;
  hipStream_t s = geoa3_stream(stream);
  if (g1) {
    const int BN1 = B * N1;
    hipLaunchKernelGGL(kpg_g1_kernel, dim3((BN1 + 255) / 256), dim3(256), 0, s, p1, p2, idx, gd, N1, N2, K, BN1, g1);
  }
  const size_t lds = ksl_lds_bytes(E, N2);
  if (g2 && lds <= KSL_LDS_MAX) {
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kpg_g2_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
    hipLaunchKernelGGL(kpg_g2_lds_kernel, dim3(B), dim3(KSL_T), lds, s, p1, p2, idx, gd, N1, N2, K, g2);
  } else if (g2) {
    const int *start = nullptr, *order = nullptr;
    const int rb = launch_dest_lists(idx, B, E, N2, scratch, s, &start, &order);
    if (rb != GEOA3_OK) return rb;
    const int BN2 = B * N2;
    hipLaunchKernelGGL(kpg_g2_kernel, dim3((BN2 + 255) / 256), dim3(256), 0, s, p1, p2, gd, start, order, N1, N2, K, BN2, g2);
  }
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
