// The neighbour half of a TRAINING-mode EdgeConv layer (DGCNN), fused (gfx950).  The layer is
//   y[c,i] = max over the k neighbours j of i of  LeakyReLU_0.2( BN_batch( W [x_j - x_i ; x_i] ) )[c]
// with BatchNorm's BATCH statistics, which sit between the convolution and the max: the fold of edgeconv.hip does not apply.
// With W = [W_a | W_b], U0 = h W_a^T and V0 = h (W_b - W_a)^T (two GEMMs per POINT, the caller's, unscaled) the pre-BN value of
// edge (i, s), j = idx[i,s], is z = U0[j] + V0[i].  Per channel, over the M = B N K edges:
//   mu = mean z,  var = mean (z - mu)^2 (biased),  r = 1 / sqrt(var + eps)
//   y[c,i] = lrelu( gamma r (u_sel + V0[i] - mu) + beta ),  lrelu(a) = a > 0 ? a : 0.2 a
// BN followed by LeakyReLU is monotone in z, so u_sel = U0[idx[i,arg]] with arg the first maximum of U0[idx[i,.],c] where
// gamma > 0, the first minimum where gamma < 0, slot 0 where gamma == 0 (the float32 inputs themselves are compared: exact).
// The [B,2C,N,k] edge tensor and the three [B,C',N,k] tensors behind it never exist, forward or backward.
//
//   et_stats_kernel   the ONE gather of the K rows of U0 per point: arg, S1[i,c] = sum_s U0[idx[i,s],c] (sequential float32
//                     from +0.0), u_sel (left in y's storage), and per (tile, channel) the sum and the sum of squares of the
//                     EXACT double value of u + v, accumulated in double in ascending (point, slot) order
//   et_reduce_kernel  the tiles' partial sums in a fixed order (et_column_sum) -> mu, var, r
//   et_apply_kernel   y <- lrelu(gamma r (y + V0 - mu) + beta), formed in double, rounded once
//   et_gprime_kernel  g' = y > 0 ? g : fl(0.2f g) (left in dV0's storage), and per (tile, channel) the double partial sums of
//                     dbeta = sum g' and dgamma = sum g' zhat_sel, zhat = (z - mu) r
//   et_du_kernel      dU0[j] = gamma r ( sum_{(i,s)->j, s == arg[i]} g'[i] - indeg(j) dbeta / M
//                                        - (dgamma / M) r ( indeg(j) (U0[j] - mu) + sum_{(i,s)->j} V0[i] ) ):
//                     one thread per (destination, channel) walks the destination list of j (dest_lists.h: with multiplicity,
//                     ascending (i, slot)); both sums sequential float32 from +0.0, the combination in double, rounded once
//   et_dv_kernel      dV0[i] = gamma r ( g' - K dbeta / M - (dgamma / M) r ( S1[i] + K V0[i] - K mu ) ), in place over g'
// No atomics on floating-point values anywhere: the same call twice gives the same bits.
// An index outside [0,N) is never dereferenced (dl_valid).  In the forward it poisons the layer: its point adds NaN to every
// channel's sums, so every y, mean and var of the call is NaN.  The backward skips such entries as the destination lists do.
// A non-finite U0 / V0 value makes its channel's sums non-finite: that channel's mean, var and y are NaN, nothing faults.
// Layouts: U0, V0, S1, arg, dU0, dV0 [B,N,C'] (point-major: a wavefront's 64 channels are 256 consecutive bytes); y, g [B,C',N],
// transposed through an LDS tile of ET_P points x ET_C channels (edge_max_kernel's tiling).
#include "dest_lists.h"

namespace {

constexpr int ET_P = 32;    // points per tile
constexpr int ET_C = 64;    // channels per tile: one wavefront across
constexpr int ET_T = 256;
constexpr int ET_G = ET_T / ET_C;    // point groups of a tile's first phase = destinations per workgroup of et_du_kernel
constexpr int ET_RW = 16;            // wavefronts of et_reduce_kernel

// the workgroup's ET_G partial sums per channel, added in group order by the first wavefront -> part[unit][c][0..1]
__device__ __forceinline__ void et_tile_sums(double a, double b, double* __restrict__ part, size_t unit, int Cpad, int c) {
#pragma clang fp contract(off)
  __shared__ double s_a[ET_G][ET_C], s_b[ET_G][ET_C];
  const int tid = threadIdx.x, cl = tid & (ET_C - 1), gr = tid / ET_C;
  s_a[gr][cl] = a;
  s_b[gr][cl] = b;
  __syncthreads();
  if (gr == 0) {
    double A = s_a[0][cl], Bv = s_b[0][cl];
#pragma unroll
    for (int w = 1; w < ET_G; ++w) {
      A = A + s_a[w][cl];
      Bv = Bv + s_b[w][cl];
    }
    double* p = part + (unit * Cpad + c) * 2;
    p[0] = A;
    p[1] = Bv;
  }
}

// the tiles' partials of one channel in an order that depends on `units` only: wavefront w of the ET_RW adds the units
// w, w + ET_RW, .. in ascending order, then the ET_RW sums are added in wavefront order.  Valid in wavefront 0.
__device__ __forceinline__ void et_column_sum(const double* __restrict__ part, int units, int Cpad, int c, double& A, double& Bv) {
#pragma clang fp contract(off)
  __shared__ double s_a[ET_RW][64], s_b[ET_RW][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a = 0., b = 0.;
  for (int u = wave; u < units; u += ET_RW) {
    const double* p = part + ((size_t)u * Cpad + c) * 2;
    a = a + p[0];
    b = b + p[1];
  }
  s_a[wave][lane] = a;
  s_b[wave][lane] = b;
  __syncthreads();
  A = 0.;
  Bv = 0.;
  if (wave == 0) {
    for (int w = 0; w < ET_RW; ++w) {
      A = A + s_a[w][lane];
      Bv = Bv + s_b[w][lane];
    }
  }
}

__global__ __launch_bounds__(ET_T) void et_stats_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                        const int64_t* __restrict__ idx, const float* __restrict__ gamma,
                                                        int N, int C, int K, int Cpad, float* __restrict__ y,
                                                        int32_t* __restrict__ arg, float* __restrict__ S1,
                                                        double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float s_y[ET_C][ET_P + 1];
  const int b = blockIdx.z, i0 = blockIdx.x * ET_P, c0 = blockIdx.y * ET_C, tid = threadIdx.x;
  const float* Ub = U + (size_t)b * N * C;
  double sum = 0., sq = 0.;
  const int cl = tid & (ET_C - 1), c = c0 + cl;
  if (c < C) {
    const float ga = gamma[c];
    for (int pl = tid / ET_C; pl < ET_P; pl += ET_G) {
      const int i = i0 + pl;
      if (i >= N) break;
      const size_t row = (size_t)b * N + i;
      const int64_t* I = idx + row * K;
      const float v = V[row * C + c];
      const double vd = (double)v;
      float best = 0.f, s1 = 0.f;
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
        s1 = s1 + u;
        const double z = (double)u + vd;   // exact
        sum = sum + z;
        sq = sq + z * z;
        const bool take = s == 0 || (ga > 0.f ? u > best : (ga < 0.f ? u < best : false));   // strict: ties to the lower slot
        best = take ? u : best;
        a = take ? s : a;
      }
      if (bad) {
        const float nan = __builtin_nanf("");
        best = nan;
        s1 = nan;
        sum = (double)nan;
        sq = (double)nan;
      }
      arg[row * C + c] = a;
      S1[row * C + c] = s1;
      s_y[cl][pl] = best;
    }
  }
  et_tile_sums(sum, sq, part, (size_t)b * gridDim.x + blockIdx.x, Cpad, c);   // (its barrier also covers s_y)
  const int pl = tid & (ET_P - 1), i = i0 + pl;
  for (int k = tid / ET_P; k < ET_C; k += ET_T / ET_P) {
    const int cc = c0 + k;
    if (i < N && cc < C) y[((size_t)b * C + cc) * N + i] = s_y[k][pl];
  }
}

// fstat (double [3][C], the forward's, kept by the caller for the backward): mu | var | r
__global__ __launch_bounds__(ET_RW * 64) void et_reduce_kernel(const double* __restrict__ part, int units, int C, int Cpad,
                                                               double M, double eps, double* __restrict__ fstat,
                                                               float* __restrict__ mean, float* __restrict__ var) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  double S, Q;
  et_column_sum(part, units, Cpad, c, S, Q);
  if (threadIdx.x >= 64) return;
  const double big = 1.7976931348623157e308, nan = (double)__builtin_nanf("");
  const bool bad = !(__builtin_fabs(S) <= big) || !(__builtin_fabs(Q) <= big);
  double mu = S / M;
  double v = Q / M - mu * mu;
  v = v < 0. ? 0. : v;
  if (bad) {
    mu = nan;
    v = nan;
  }
  if (c < C) {
    fstat[c] = mu;
    fstat[C + c] = v;
    fstat[2 * C + c] = 1. / __builtin_sqrt(v + eps);
    mean[c] = (float)mu;
    var[c] = (float)v;
  }
}

__global__ __launch_bounds__(ET_RW * 64) void et_reduce_grad_kernel(const double* __restrict__ part, int units, int C, int Cpad,
                                                                    double* __restrict__ gstat, float* __restrict__ dgamma,
                                                                    float* __restrict__ dbeta) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  double db, dg;
  et_column_sum(part, units, Cpad, c, db, dg);
  if (threadIdx.x >= 64) return;
  gstat[c] = db;   // gstat (double [2][Cpad], workspace): dbeta | dgamma
  gstat[Cpad + c] = dg;
  if (c < C) {
    dbeta[c] = (float)db;
    dgamma[c] = (float)dg;
  }
}

// y [B,C,N] holds u_sel on entry
__global__ __launch_bounds__(ET_T) void et_apply_kernel(const float* __restrict__ V, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const double* __restrict__ fstat, int N,
                                                        int C, float* __restrict__ y) {
#pragma clang fp contract(off)
  __shared__ float s_v[ET_C][ET_P + 1];
  const int b = blockIdx.z, i0 = blockIdx.x * ET_P, c0 = blockIdx.y * ET_C, tid = threadIdx.x;
  {
    const int cl = tid & (ET_C - 1), c = c0 + cl;
    for (int pl = tid / ET_C; pl < ET_P; pl += ET_G) {
      const int i = i0 + pl;
      if (i < N && c < C) s_v[cl][pl] = V[((size_t)b * N + i) * C + c];
    }
  }
  __syncthreads();
  const int pl = tid & (ET_P - 1), i = i0 + pl;
  for (int cl = tid / ET_P; cl < ET_C; cl += ET_T / ET_P) {
    const int c = c0 + cl;
    if (i >= N || c >= C) continue;
    const size_t o = ((size_t)b * C + c) * N + i;
    const double mu = fstat[c], r = fstat[2 * C + c];
    double a = ((double)y[o] + (double)s_v[cl][pl]) - mu;
    a = (double)gamma[c] * r * a + (double)beta[c];
    y[o] = (float)(a > 0. ? a : a * 0.2);
  }
}

// gp [B,N,C] = g' (g, y [B,C,N]); part <- the tile's sums of g' and g' zhat_sel
__global__ __launch_bounds__(ET_T) void et_gprime_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                         const float* __restrict__ U, const float* __restrict__ V,
                                                         const int32_t* __restrict__ arg, const int64_t* __restrict__ idx,
                                                         const double* __restrict__ fstat, int N, int C, int K, int Cpad,
                                                         float* __restrict__ gp, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float s_g[ET_C][ET_P + 1];
  const int b = blockIdx.z, i0 = blockIdx.x * ET_P, c0 = blockIdx.y * ET_C, tid = threadIdx.x;
  {
    const int pl = tid & (ET_P - 1), i = i0 + pl;
    for (int cl = tid / ET_P; cl < ET_C; cl += ET_T / ET_P) {
      const int c = c0 + cl;
      if (i >= N || c >= C) continue;
      const size_t o = ((size_t)b * C + c) * N + i;
      const float gv = g[o];
      // the gate is the STORED float32 y (what the caller holds), not the double pre-activation: the two differ only where a
      // positive pre-activation rounds to 0 in float32 (below 2^-150), which then takes the 0.2 branch
      s_g[cl][pl] = y[o] > 0.f ? gv : gv * 0.2f;
    }
  }
  __syncthreads();
  const int cl = tid & (ET_C - 1), c = c0 + cl;
  double db = 0., dg = 0.;
  if (c < C) {
    const double mu = fstat[c], r = fstat[2 * C + c];
    for (int pl = tid / ET_C; pl < ET_P; pl += ET_G) {
      const int i = i0 + pl;
      if (i >= N) break;
      const size_t row = (size_t)b * N + i;
      const float gv = s_g[cl][pl];
      gp[row * C + c] = gv;
      db = db + (double)gv;
      const int a = arg[row * C + c];
      if ((unsigned)a >= (unsigned)K) continue;
      const int64_t j = idx[row * K + a];
      if (!dl_valid(j, N)) continue;
      const double z = (double)U[((size_t)b * N + (size_t)j) * C + c] + (double)V[row * C + c];
      dg = dg + (double)gv * ((z - mu) * r);
    }
  }
  et_tile_sums(db, dg, part, (size_t)b * gridDim.x + blockIdx.x, Cpad, c);
}

// dU0: one thread per (destination, channel), a wavefront across 64 channels of one destination
__global__ __launch_bounds__(ET_T) void et_du_kernel(const float* __restrict__ gp, const float* __restrict__ U,
                                                     const float* __restrict__ V, const int32_t* __restrict__ arg,
                                                     const int* __restrict__ start, const int* __restrict__ order,
                                                     const float* __restrict__ gamma, const double* __restrict__ fstat,
                                                     const double* __restrict__ gstat, int N, int C, int K, int Cpad, double M,
                                                     float* __restrict__ dU) {
#pragma clang fp contract(off)
  const int b = blockIdx.z, tid = threadIdx.x;
  const int j = blockIdx.x * ET_G + tid / ET_C, c = blockIdx.y * ET_C + (tid & (ET_C - 1));
  if (j >= N || c >= C) return;
  const int* S = start + (size_t)b * (N + 1);
  const int s0 = S[j], s1 = S[j + 1];
  const int* O = order + (size_t)b * N * K;
  const size_t base = (size_t)b * N * C + c;
  float accg = 0.f, accv = 0.f;
  for (int q = s0; q < s1; ++q) {
    const int e = O[q];
    const int i = e / K, slot = e - i * K;
    const size_t o = base + (size_t)i * C;
    accv = accv + V[o];
    if (arg[o] == slot) accg = accg + gp[o];
  }
  const double mu = fstat[c], r = fstat[2 * C + c], db = gstat[c], dg = gstat[Cpad + c];
  const double deg = (double)(s1 - s0);
  const size_t oj = base + (size_t)j * C;
  const double inner = deg * ((double)U[oj] - mu) + (double)accv;
  const double d = ((double)accg - deg * db / M) - (dg / M) * r * inner;
  dU[oj] = (float)((double)gamma[c] * r * d);
}

// dV0 [B,N,C], g' on entry
__global__ __launch_bounds__(ET_T) void et_dv_kernel(const float* __restrict__ V, const float* __restrict__ S1,
                                                     const float* __restrict__ gamma, const double* __restrict__ fstat,
                                                     const double* __restrict__ gstat, int N, int C, int K, int Cpad, double M,
                                                     float* __restrict__ dV) {
#pragma clang fp contract(off)
  const int b = blockIdx.z, tid = threadIdx.x;
  const int i = blockIdx.x * ET_G + tid / ET_C, c = blockIdx.y * ET_C + (tid & (ET_C - 1));
  if (i >= N || c >= C) return;
  const size_t o = ((size_t)b * N + i) * C + c;
  const double mu = fstat[c], r = fstat[2 * C + c], db = gstat[c], dg = gstat[Cpad + c];
  const double kk = (double)K;
  const double inner = ((double)S1[o] + kk * (double)V[o]) - kk * mu;
  const double d = ((double)dV[o] - kk * db / M) - (dg / M) * r * inner;
  dV[o] = (float)((double)gamma[c] * r * d);
}

inline size_t et_align(size_t x) { return (x + 255) & ~(size_t)255; }
struct EtLayout {
  size_t part, stat, lists, total;
  int Cpad, tiles;
};
inline EtLayout et_layout(int B, int N, int C, int K) {
  EtLayout l;
  l.Cpad = (C + ET_C - 1) / ET_C * ET_C;
  l.tiles = (N + ET_P - 1) / ET_P;
  l.part = 0;
  l.stat = et_align((size_t)B * l.tiles * l.Cpad * 2 * sizeof(double));
  l.lists = l.stat + et_align((size_t)2 * l.Cpad * sizeof(double));
  l.total = l.lists + et_align(dest_lists_scratch_bytes(B, N * K, N));
  return l;
}
// sizes every entry accepts (B N K < 2: BatchNorm has no variance to normalise by)
int et_sizes(int B, int N, int C, int K) {
  if (B <= 0 || N <= 0 || C <= 0 || K < 1 || (int64_t)B * N * K < 2) return GEOA3_EINVAL;
  if ((int64_t)N * K > (int64_t)INT_MAX - 256 || B > 65535 || (C - 1) / ET_C + 1 > 65535 ||
      (int64_t)B * ((N + ET_P - 1) / ET_P) > (int64_t)INT_MAX)
    return GEOA3_ENOSUPPORT;
  return GEOA3_OK;
}

}  // namespace

extern "C" int64_t geoa3_edge_train_workspace_bytes(int B, int N, int C, int K) {
  const int rc = et_sizes(B, N, C, K);
  if (rc != GEOA3_OK) return rc;
  return (int64_t)et_layout(B, N, C, K).total;
}

extern "C" int geoa3_edge_train_forward(const float* U0, const float* V0, const int64_t* idx, const float* gamma,
                                        const float* beta, float eps, int B, int N, int C, int K, float* y, int32_t* arg,
                                        float* S1, float* mean, float* var, double* stats, void* workspace, void* stream) {
  if (!U0 || !V0 || !idx || !gamma || !beta || !y || !arg || !S1 || !mean || !var || !stats || !workspace) return GEOA3_EINVAL;
  const int rc = et_sizes(B, N, C, K);
  if (rc != GEOA3_OK) return rc;
  hipStream_t s = geoa3_stream(stream);
  const EtLayout l = et_layout(B, N, C, K);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  double* part = reinterpret_cast<double*>(ws + l.part);
  const dim3 grid(l.tiles, l.Cpad / ET_C, B);
  hipLaunchKernelGGL(et_stats_kernel, grid, dim3(ET_T), 0, s, U0, V0, idx, gamma, N, C, K, l.Cpad, y, arg, S1, part);
  GEOA3_CHECK_LAUNCH();
  hipLaunchKernelGGL(et_reduce_kernel, dim3(l.Cpad / 64), dim3(ET_RW * 64), 0, s, part, B * l.tiles, C, l.Cpad,
                     (double)B * (double)N * (double)K, (double)eps, stats, mean, var);
  GEOA3_CHECK_LAUNCH();
  hipLaunchKernelGGL(et_apply_kernel, grid, dim3(ET_T), 0, s, V0, gamma, beta, stats, N, C, y);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_edge_train_grad(const float* g, const float* y, const float* U0, const float* V0, const int32_t* arg,
                                     const float* S1, const int64_t* idx, const float* gamma, const double* stats,
                                     int B, int N, int C, int K, float* dU0, float* dV0, float* dgamma, float* dbeta,
                                     void* workspace, void* stream) {
  if (!g || !y || !U0 || !V0 || !arg || !S1 || !idx || !gamma || !stats || !dU0 || !dV0 || !dgamma || !dbeta || !workspace)
    return GEOA3_EINVAL;
  const int rc = et_sizes(B, N, C, K);
  if (rc != GEOA3_OK) return rc;
  hipStream_t s = geoa3_stream(stream);
  const EtLayout l = et_layout(B, N, C, K);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  double* part = reinterpret_cast<double*>(ws + l.part);
  double* gstat = reinterpret_cast<double*>(ws + l.stat);
  const int cg = l.Cpad / ET_C;
  const int *start = nullptr, *order = nullptr;   // the lists first: when they fail, no output has been written
  const int rb = launch_dest_lists(idx, B, N * K, N, ws + l.lists, s, &start, &order);
  if (rb != GEOA3_OK) return rb;
  hipLaunchKernelGGL(et_gprime_kernel, dim3(l.tiles, cg, B), dim3(ET_T), 0, s, g, y, U0, V0, arg, idx, stats, N, C, K, l.Cpad,
                     dV0, part);
  GEOA3_CHECK_LAUNCH();
  hipLaunchKernelGGL(et_reduce_grad_kernel, dim3(l.Cpad / 64), dim3(ET_RW * 64), 0, s, part, B * l.tiles, C, l.Cpad, gstat,
                     dgamma, dbeta);
  GEOA3_CHECK_LAUNCH();
  const double M = (double)B * (double)N * (double)K;
  const dim3 pgrid((N + ET_G - 1) / ET_G, cg, B);
  hipLaunchKernelGGL(et_du_kernel, pgrid, dim3(ET_T), 0, s, dV0, U0, V0, arg, start, order, gamma, stats, gstat, N, C, K, l.Cpad, M,
                     dU0);
  GEOA3_CHECK_LAUNCH();
  hipLaunchKernelGGL(et_dv_kernel, pgrid, dim3(ET_T), 0, s, V0, S1, gamma, stats, gstat, N, C, K, l.Cpad, M, dV0);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
