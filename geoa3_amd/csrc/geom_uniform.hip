// The PU-GAN uniformity term of the reference (Lib/loss_utils.py:151-189, `uniform_loss`), its value and its gradient
// d U / d adv_pc, for all percentages in one call (geoa3_uniform_loss), and the fold of w * U into the attack's
// constrain loss and of w * (sum_b c_b) / B * dU/dx into its unscaled gradient (geoa3_uniform_fold,
// Attacker/geoA3_attack.py:168-178).
//
// Per call:
//   1. the planar cloud [B,3,N] is copied point-major ([B,N,3], the sampler's layout);
//   2. furthest_point_sample(adv_pc, npoint) through the sampler of pointnet2_ops.hip (launch_pn2_fps_range): the same
//      bits as geoa3_pn2_furthest_point_sampling(_ex), |p|^2 <= 1e-3 skip and tie order included.  The reference calls it
//      once per percentage on the same input: one run serves all of them;
//   3. uniform_main_kernel, one workgroup per instance: the cloud in LDS, one wavefront per centre.  The ball query is
//      the ballot form of ball_query_wave_kernel (first `nsample` in-radius indices in index order, the first hit
//      pre-filling every slot); the group's K-NN (K = k + 1, squared distances un-fused as geoa3_sqdist, equal distances
//      to the lower slot) is one row per lane over the group's slots, read through the index row from the cloud in LDS.
//      Row terms (u - e)^2 / (e + 1e-12), u = mean_k sqrt(|d_k| + 1e-12) over k = 1..K-1, are summed per lane in double
//      in a fixed order, then over lanes and waves in a fixed order.  Each (row, neighbour) pair adds c (p_r - p_n) to
//      the row's cloud point and subtracts it from the neighbour's (p1 and p2 of knn_points are the same tensor); c = 0
//      where d = 0 (abs's subgradient), so the self pair and padded duplicates carry no gradient.  The per-point sums are
//      64-bit fixed point (2^-32; a pair adds at most |2 (u - e) / e| * scale / nsample in magnitude): integer adds, so
//      the order the atomics land in does not change a bit.  They live in LDS when the cloud and three int64 per point
//      fit, otherwise in the workspace (N > ~4200);
//   4. uniform_final_kernel: U = (1/P) sum_p scale_p / (B npoint nsample_p) sum_b partial[b][p], in double, fixed order.
#include "pointnet_kernels.h"

namespace {

constexpr int UNI_MAX_P = 8;        // percentages per call
constexpr int UNI_MAX_NS = 512;     // samples per group
constexpr int UNI_MAX_K = 8;        // neighbours kept per row (the K-NN keeps k + 1)
constexpr int UNI_THREADS = 512;    // 8 wavefronts per instance
constexpr int UNI_WAVES = UNI_THREADS / 64;
constexpr size_t UNI_LDS_MAX = 160 * 1024 - 1024;   // dynamic LDS (the static wave partials beside it)
constexpr double UNI_FX = 4294967296.0;   // fixed-point scale of the gradient sums (2^32)

struct UniformParams {
  int P, npoint, K;                 // K = k + 1 neighbours per row (the first one is dropped)
  int ns[UNI_MAX_P];                // nsample per percentage
  int ns_off[UNI_MAX_P];            // offset of percentage p's rows in group_idx, in units of B * npoint
  float r2[UNI_MAX_P];              // float(r) * float(r)
  float e[UNI_MAX_P];               // expect_len
  float cp[UNI_MAX_P];              // scale_p / nsample_p: the per-pair factor of the gradient
  double gscale;                    // 1 / (P * B * npoint): the common factor of every gradient sum
};

template <bool CT = false>
__device__ __forceinline__ float uni_sq3(float dx, float dy, float dz) {
#pragma clang fp contract(off)
  if (CT) return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float s = xx + yy;
  return s + zz;
}

__global__ __launch_bounds__(256) void uniform_transpose_kernel(const float* __restrict__ pc, float* __restrict__ xyz,
                                                                int N) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float* P = pc + (size_t)b * 3 * N;
  float* O = xyz + ((size_t)b * N + i) * 3;
  O[0] = P[i];
  O[1] = P[N + i];
  O[2] = P[2 * N + i];
}

__device__ __forceinline__ void uni_add(unsigned long long* a, float v) {
  const long long q = __double2ll_rn((double)v * UNI_FX);
  if (q != 0) atomicAdd(a, (unsigned long long)q);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One row of a group: the KP nearest slots (ascending, equal distances to the lower slot) of slot r, then the row term
// and the pair gradients.  KP == UNI_MAX_K + 1 keeps the nine nearest and uses the first K of them.
template <int KP>
__device__ __forceinline__ double uniform_row(const float* __restrict__ s_x, const float* __restrict__ s_y,
                                              const float* __restrict__ s_z, const int* __restrict__ row, int ns, int r,
                                              int K, float e, float cp, unsigned long long* __restrict__ acc, int N) {
  const int ir = row[r];
  const float px = s_x[ir], py = s_y[ir], pz = s_z[ir];
  float d[KP];
  int id[KP];
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    d[q] = __builtin_inff();
    id[q] = 0;
  }
  for (int t = 0; t < ns; ++t) {
    const int it = row[t];
    const float dd = geoa3_sqdist(px, py, pz, s_x[it], s_y[it], s_z[it]);
    if (dd < d[KP - 1]) {
#pragma unroll
      for (int q = KP - 1; q >= 0; --q) {
        const bool sh = q > 0 && dd < d[q > 0 ? q - 1 : 0];
        if (dd < d[q]) {
          d[q] = sh ? d[q > 0 ? q - 1 : 0] : dd;
          id[q] = sh ? id[q > 0 ? q - 1 : 0] : t;
        }
      }
    }
  }
  // u = mean over the K - 1 kept neighbours of sqrt(|d| + 1e-12) (a sum, then the division, as torch.mean)
  float s = 0.f;
#pragma unroll
  for (int q = 1; q < KP; ++q)
    if (q < K) s += sqrtf(fabsf(d[q]) + 1e-12f);
  const float km = (float)(K - 1);
  const float u = s / km;
  const float den = e + 1e-12f;
  const float diff = u - e;
  const float term = diff * diff / den;
  // d term / d u = 2 (u - e) / (e + 1e-12); d u / d d_k = 0.5 / (K-1) / sqrt(|d_k| + 1e-12) * sign(d_k); d d / d p_r = 2 (p_r - p_n)
  const float g = 2.f * diff / den * cp / km;
#pragma unroll
  for (int q = 1; q < KP; ++q) {
    if (q < K && d[q] != 0.f) {
      const float c = g / sqrtf(fabsf(d[q]) + 1e-12f);
      const int in = row[id[q]];
      const float gx = c * (px - s_x[in]), gy = c * (py - s_y[in]), gz = c * (pz - s_z[in]);
      uni_add(acc + ir, gx);
      uni_add(acc + N + ir, gy);
      uni_add(acc + 2 * N + ir, gz);
      uni_add(acc + in, -gx);
      uni_add(acc + N + in, -gy);
      uni_add(acc + 2 * N + in, -gz);
    }
  }
  return (double)term;
}

template <int KP, bool CT, bool LDS_ACC>
__global__ __launch_bounds__(UNI_THREADS) void uniform_main_kernel(const float* __restrict__ pc, int N, int nsmax,
                                                                   UniformParams prm, const int32_t* __restrict__ fps,
                                                                   unsigned long long* __restrict__ gacc,
                                                                   double* __restrict__ partial,
                                                                   float* __restrict__ grad,
                                                                   int32_t* __restrict__ group_idx, int B) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_part[UNI_MAX_P][UNI_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // [acc 3N int64 (LDS_ACC)] [x N] [y N] [z N] [rows UNI_WAVES x nsmax int]
  unsigned long long* acc = LDS_ACC ? reinterpret_cast<unsigned long long*>(s_raw) : gacc + (size_t)b * 3 * N;
  float* s_x = reinterpret_cast<float*>(s_raw + (LDS_ACC ? (size_t)N * 3 * 8 : 0));
  float *s_y = s_x + N, *s_z = s_x + 2 * N;
  int* row = reinterpret_cast<int*>(s_z + N) + wave * nsmax;
  const float* P = pc + (size_t)b * 3 * N;
  bool bad = false;
  for (int i = tid; i < N; i += UNI_THREADS) {
    const float x = P[i], y = P[N + i], z = P[2 * N + i];
    s_x[i] = x;
    s_y[i] = y;
    s_z[i] = z;
    bad = bad || geoa3_nonfinite(x) || geoa3_nonfinite(y) || geoa3_nonfinite(z);
  }
  for (int i = tid; i < 3 * N; i += UNI_THREADS) {
    if (LDS_ACC) acc[i] = 0ull;
    else __hip_atomic_store(acc + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // a non-finite coordinate: NaN loss and gradient for the instance (a NaN point would otherwise fall out of every ball)
  if (__syncthreads_or(bad)) {
    if (tid < prm.P) partial[(size_t)b * prm.P + tid] = __builtin_nan("");
    for (int i = tid; i < 3 * N; i += UNI_THREADS) grad[(size_t)b * 3 * N + i] = __builtin_nanf("");
    if (group_idx)
      for (int p = 0; p < prm.P; ++p)
        for (int i = tid; i < prm.npoint * prm.ns[p]; i += UNI_THREADS)
          group_idx[(size_t)prm.ns_off[p] * B + (size_t)b * prm.npoint * prm.ns[p] + i] = 0;
    return;
  }
  const int32_t* F = fps + (size_t)b * prm.npoint;
  for (int p = 0; p < prm.P; ++p) {
    const int ns = prm.ns[p];
    const float r2 = prm.r2[p], e = prm.e[p], cp = prm.cp[p];
    double tsum = 0.0;
    for (int j = wave; j < prm.npoint; j += UNI_WAVES) {
      const int c0 = F[j];
      const float cx = s_x[c0], cy = s_y[c0], cz = s_z[c0];
      // ball query: ballot per 64-point chunk, a hit's slot = running count + hits below its lane
      int cnt = 0;
      for (int k0 = 0; k0 < N && cnt < ns; k0 += 64) {
        const int k = k0 + lane;
        bool hit = false;
        if (k < N) hit = uni_sq3<CT>(cx - s_x[k], cy - s_y[k], cz - s_z[k]) < r2;
        const unsigned long long mask = __ballot(hit);
        if (mask == 0ull) continue;
        if (cnt == 0) {
          const int first = k0 + (int)__builtin_ctzll(mask);   // the first hit pre-fills every slot
          for (int l = lane; l < ns; l += 64) row[l] = first;
        }
        const int slot = cnt + (int)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (hit && slot < ns) row[slot] = k;
        cnt += (int)__builtin_popcountll(mask);
      }
      if (cnt == 0)
        for (int l = lane; l < ns; l += 64) row[l] = 0;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (group_idx) {
        int32_t* G = group_idx + (size_t)prm.ns_off[p] * B + ((size_t)b * prm.npoint + j) * ns;
        for (int l = lane; l < ns; l += 64) G[l] = row[l];
      }
      for (int r = lane; r < ns; r += 64) tsum += uniform_row<KP>(s_x, s_y, s_z, row, ns, r, prm.K, e, cp, acc, N);
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the row is re-filled by the next centre
    }
    tsum = wave_sum_f64(tsum);
    if (lane == 0) s_part[p][wave] = tsum;
  }
  __syncthreads();
  if (tid < prm.P) {
    double s = 0.0;
    for (int w = 0; w < UNI_WAVES; ++w) s += s_part[tid][w];
    partial[(size_t)b * prm.P + tid] = s;
  }
  const double gs = prm.gscale / UNI_FX;
  for (int i = tid; i < 3 * N; i += UNI_THREADS) {
    const unsigned long long a = LDS_ACC ? acc[i] : __hip_atomic_load(acc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    grad[(size_t)b * 3 * N + i] = (float)((double)(long long)a * gs);
  }
}

// U = (1/P) sum_p scale_p / (B npoint ns_p) * sum_b partial[b][p]: per percentage, thread t sums instances t, t + 256, ...
// and a fixed tree adds the threads
struct UniformWeights {
  double wp[UNI_MAX_P];   // scale_p / (B npoint ns_p)
};
__global__ __launch_bounds__(256) void uniform_final_kernel(const double* __restrict__ partial, int B, int P,
                                                            UniformWeights fw, float* __restrict__ loss) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int p = 0; p < P; ++p) {
    double v = 0.0;
    for (int b = tid; b < B; b += 256) v += partial[(size_t)b * P + p];
    s[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) s[tid] += s[tid + o];
      __syncthreads();
    }
    total += s[0] * fw.wp[p];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(total / (double)P);
}

// constrain[b] (+)= w * U;  g[b] (+)= w * (sum_b c_b / B) * dU [b]
__global__ __launch_bounds__(256) void uniform_fold_kernel(const float* __restrict__ loss, const float* __restrict__ dU,
                                                           const float* __restrict__ scale_const, float w, int B, int n3,
                                                           float* __restrict__ constrain, int constrain_add,
                                                           float* __restrict__ g, int g_add) {
  const int tid = threadIdx.x;
  if (constrain) {
    const size_t i = (size_t)blockIdx.x * 256 + tid;
    if (i < (size_t)B) {
      const float wu = w * loss[0];
      constrain[i] = constrain_add ? constrain[i] + wu : wu;
    }
  }
  if (!g) return;
  __shared__ float s[256];
  const float invB = 1.f / (float)B;
  float v = 0.f;
  for (int b = tid; b < B; b += 256) v += scale_const[b] * invB;
  s[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  const float coef = w * s[0];
  const size_t total = (size_t)B * n3;
  for (size_t i = (size_t)blockIdx.x * 256 + tid; i < total; i += (size_t)gridDim.x * 256)
    g[i] = g_add ? g[i] + coef * dU[i] : coef * dU[i];
}

struct UniformPlan {
  UniformParams prm;
  UniformWeights fw;
  int nsmax, ns_total;
  bool lds_acc;
  size_t lds;
};

// the host scalars of Lib/loss_utils.py:155-162 in double, as the reference's Python forms them
int uniform_plan(int B, int N, const double* percentages, int P, double radius, int k, UniformPlan* pl) {
  if (B <= 0 || N <= 0 || !percentages || P <= 0 || k < 1 || !(radius > 0.0)) return GEOA3_EINVAL;
  if (P > UNI_MAX_P || k > UNI_MAX_K || N > 512 * 16) return GEOA3_ENOSUPPORT;
  UniformParams& q = pl->prm;
  q.P = P;
  q.K = k + 1;
  q.npoint = (int)(N * 0.05);
  if (q.npoint < 1) return GEOA3_ENOSUPPORT;
  pl->nsmax = 0;
  pl->ns_total = 0;
  for (int i = 0; i < P; ++i) {
    const double p = percentages[i] * 4;
    if (!(p > 0.0)) return GEOA3_EINVAL;
    const double nsd = N * p;
    if (!(nsd < 1e9)) return GEOA3_ENOSUPPORT;
    const int ns = (int)nsd;
    if (ns < k + 1 || ns > UNI_MAX_NS) return GEOA3_ENOSUPPORT;
    const double r = sqrt(p * radius);
    const float rf = (float)r;
    const double disk_area = M_PI * (radius * radius) * p / ns;
    const float e = sqrtf((float)disk_area);
    const double scale = pow(p * 100, 2);
    q.ns[i] = ns;
    q.ns_off[i] = pl->ns_total * q.npoint;
    q.r2[i] = rf * rf;
    q.e[i] = e;
    q.cp[i] = (float)(scale / ns);
    pl->fw.wp[i] = scale / ((double)B * q.npoint * ns);
    pl->nsmax = ns > pl->nsmax ? ns : pl->nsmax;
    pl->ns_total += ns;
  }
  q.gscale = 1.0 / ((double)P * B * q.npoint);
  const size_t base = (size_t)N * 3 * sizeof(float) + (size_t)UNI_WAVES * pl->nsmax * sizeof(int);
  pl->lds_acc = base + (size_t)N * 3 * 8 <= UNI_LDS_MAX;
  pl->lds = base + (pl->lds_acc ? (size_t)N * 3 * 8 : 0);
  if (pl->lds > UNI_LDS_MAX) return GEOA3_ENOSUPPORT;
  return GEOA3_OK;
}

// the one predicate of launch_uniform_main and geoa3_debug_uniform_route
int uniform_route(const UniformPlan& pl) { return pl.lds_acc ? GEOA3_UNIFORM_ROUTE_LDS : GEOA3_UNIFORM_ROUTE_WORKSPACE; }

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: [partial B x UNI_MAX_P double] [xyz B x N x 3 float] [fps B x N int] [acc B x 3N int64 (large clouds)]
struct UniformWs {
  double* partial;
  float* xyz;
  int32_t* fps;
  unsigned long long* acc;
};
UniformWs uniform_ws(void* ws, int B, int N) {
  unsigned char* p = static_cast<unsigned char*>(ws);
  UniformWs w;
  w.partial = reinterpret_cast<double*>(p);
  p += align256((size_t)B * UNI_MAX_P * sizeof(double));
  w.xyz = reinterpret_cast<float*>(p);
  p += align256((size_t)B * N * 3 * sizeof(float));
  w.fps = reinterpret_cast<int32_t*>(p);
  p += align256((size_t)B * N * sizeof(int32_t));
  w.acc = reinterpret_cast<unsigned long long*>(p);
  return w;
}

template <int KP, bool CT>
int launch_uniform_main(const UniformPlan& pl, const float* pc, int B, int N, const UniformWs& w, float* grad,
                        int32_t* group_idx, hipStream_t s) {
  if (uniform_route(pl) == GEOA3_UNIFORM_ROUTE_LDS) {
    auto kern = uniform_main_kernel<KP, CT, true>;
    if (pl.lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    hipLaunchKernelGGL(kern, dim3(B), dim3(UNI_THREADS), pl.lds, s, pc, N, pl.nsmax, pl.prm, w.fps, w.acc, w.partial,
                       grad, group_idx, B);
  } else {
    auto kern = uniform_main_kernel<KP, CT, false>;
    if (pl.lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    hipLaunchKernelGGL(kern, dim3(B), dim3(UNI_THREADS), pl.lds, s, pc, N, pl.nsmax, pl.prm, w.fps, w.acc, w.partial,
                       grad, group_idx, B);
  }
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

}  // namespace

extern "C" int64_t geoa3_uniform_loss_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0) return 0;
  size_t n = align256((size_t)B * UNI_MAX_P * sizeof(double)) + align256((size_t)B * N * 3 * sizeof(float)) +
             align256((size_t)B * N * sizeof(int32_t));
  // the gradient sums of clouds whose three int64 per point do not fit in LDS beside the cloud
  const size_t lds_all = (size_t)N * 3 * sizeof(float) + (size_t)UNI_WAVES * UNI_MAX_NS * sizeof(int) + (size_t)N * 3 * 8;
  if (lds_all > UNI_LDS_MAX) n += (size_t)B * 3 * N * sizeof(unsigned long long);
  return (int64_t)n;
}

extern "C" int geoa3_debug_uniform_route(int B, int N, const double* percentages, int P, double radius, int k) {
  UniformPlan pl;
  const int rc = uniform_plan(B, N, percentages, P, radius, k, &pl);
  return rc != GEOA3_OK ? rc : uniform_route(pl);
}

extern "C" int geoa3_uniform_loss(const float* pc, int B, int N, const double* percentages, int num_percentages,
                                  double radius, int k, int flags, float* loss, float* grad, int32_t* fps_idx,
                                  int32_t* group_idx, void* workspace, void* stream) {
  if (!pc || !loss || !grad || !workspace || (flags & ~GEOA3_PN2_CONTRACT)) return GEOA3_EINVAL;
  UniformPlan pl;
  const int rc = uniform_plan(B, N, percentages, num_percentages, radius, k, &pl);
  if (rc != GEOA3_OK) return rc;
  // the plan keeps the gradient sums in LDS exactly where the workspace query left them out
  const size_t lds_all = (size_t)N * 3 * sizeof(float) + (size_t)UNI_WAVES * UNI_MAX_NS * sizeof(int) + (size_t)N * 3 * 8;
  if (!pl.lds_acc && lds_all <= UNI_LDS_MAX) return GEOA3_EINVAL;   // (cannot happen: nsmax <= UNI_MAX_NS)
  const bool ct = (flags & GEOA3_PN2_CONTRACT) != 0;
  hipStream_t s = geoa3_stream(stream);
  const UniformWs w = uniform_ws(workspace, B, N);
  hipLaunchKernelGGL(uniform_transpose_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, pc, w.xyz, N);
  GEOA3_CHECK_LAUNCH();
  int32_t* fps = fps_idx ? fps_idx : w.fps;
  int r = launch_pn2_fps_range(w.xyz, B, N, pl.prm.npoint, 0, pl.prm.npoint, nullptr, fps, s, ct);
  if (r != GEOA3_OK) return r;
  UniformWs wm = w;
  wm.fps = fps;
  if (pl.prm.K == 3)
    r = ct ? launch_uniform_main<3, true>(pl, pc, B, N, wm, grad, group_idx, s)
           : launch_uniform_main<3, false>(pl, pc, B, N, wm, grad, group_idx, s);
  else
    r = ct ? launch_uniform_main<UNI_MAX_K + 1, true>(pl, pc, B, N, wm, grad, group_idx, s)
           : launch_uniform_main<UNI_MAX_K + 1, false>(pl, pc, B, N, wm, grad, group_idx, s);
  if (r != GEOA3_OK) return r;
  hipLaunchKernelGGL(uniform_final_kernel, dim3(1), dim3(256), 0, s, w.partial, B, pl.prm.P, pl.fw, loss);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_uniform_fold(const float* loss, const float* grad, const float* scale_const, float w, int B, int N,
                                  float* constrain, int constrain_add, float* g, int g_add, void* stream) {
  if (!loss || B <= 0 || N <= 0 || (!constrain && !g) || (g && (!grad || !scale_const))) return GEOA3_EINVAL;
  const size_t total = (size_t)B * 3 * N;
  int blocks = g ? (int)((total + 255) / 256) : (B + 255) / 256;
  if (blocks < (B + 255) / 256) blocks = (B + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(uniform_fold_kernel, dim3(blocks), dim3(256), 0, geoa3_stream(stream), loss, grad, scale_const, w, B,
                     3 * N, constrain, constrain_add, g, g_add);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
