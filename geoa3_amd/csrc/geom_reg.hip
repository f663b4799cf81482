// The neighbour-based regularisers of the reference's Lib/loss_utils.py that are functions of a self K-NN table:
//   kNN_smoothing_loss (:135-149), repulsion_loss (:119-123), displacement_loss (:99-107),
// each as a forward and a backward entry point, and the fold of w * S into the attack's constrain loss and gradient
// (geoa3_reg_fold: a per-row term; geoa3_reg_fold_points: a per-point term through its row mean).
// corresponding_normal_loss (:109-117): the forward is geoa3_kappa with the point's own normal; its backward is a mode of
// reg_bwd_kernel here (pair terms in double; the dkappa path of geoa3_geo_loss_grad is the float32 alternative).
//
// The table is geoa3_knn_self's: dists / idx [B,N,ld] ascending by (distance, index), column 0 dropped as the reference's
// [:, :, 1:].  The caller hands it over (knn_d, knn_i, knn_ld >= k + 1: the first k + 1 columns of a wider table serve)
// or the entry point runs geoa3_knn_self (all pairs, no prior) into the workspace.
//
// Forward kernels: one workgroup per instance.  The per-instance statistics of kNN_smoothing_loss (mean and unbiased
// standard deviation of s_i over the cloud, the masked mean) are summed in double in a fixed order: thread t takes points
// t, t + 512, ..., a fixed tree adds the threads.
//
// Backward kernel (reg_bwd_kernel, one workgroup per instance): every (point i, neighbour j) pair has a coefficient; it
// adds coefficient * 2 (x_i - x_j) to point i and subtracts it from point j (displacement_loss: a scalar, to d theta).
// The per-point sums are 64-bit fixed point, so the order the atomics land in does not change a bit: repeated calls are
// bit identical and a row does not depend on the rest of the batch.  The scale is the instance's own: pass 1 takes the
// largest |term| of the instance (a maximum: order free), the unit is 2^(e - 40) with e its exponent, pass 2 forms the
// terms again and adds them.  Coefficients and terms are formed in double (B N k pairs: the cost is not arithmetic).
// A point of a search's table sums at most N + k terms of at most 2^41 units each; a handed-in table may name one point in
// every entry, which then sums N k + k terms: at most 8192 * 63 + 63 < 2^19 terms, below 2^60 units, no overflow.
// A non-finite term or coordinate, or a
// neighbour index outside the cloud, makes the whole instance's gradient NaN (displace_fwd_kernel: an index outside the
// cloud makes that point's value NaN, the others keep their bits).
// kNN_smoothing_loss reads distances only: a non-finite distance in columns 1..k of a handed-in table over a finite cloud
// (any input that makes the threshold NaN) gives the instance loss NaN, mask 0 and gradient NaN -- never a silent
// "nothing exceeds the threshold".  Column 0 and the columns beyond k are read by no kernel.
// The sums live in LDS beside the cloud (N <= ~4200); beyond that in the workspace, the cloud read from global memory.
#include "common.h"

namespace {

constexpr int REG_T = 512;                              // 8 wavefronts per instance
constexpr size_t REG_LDS_MAX = 160 * 1024 - 6144;       // dynamic LDS (the static reduction buffer beside it)
constexpr int REG_FX_BITS = 40;
constexpr int REG_MAX_N = 8192;

enum { REG_SMOOTH = 0, REG_REPULSE = 1, REG_DISPLACE = 2, REG_NORMAL = 3 };
constexpr double REG_NORM_EPS = 1e-12;                  // Lib/utility.py:30 (_normalize eps)

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// sum / maximum over the workgroup in a fixed order; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  for (int o = REG_T / 2; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  return s_red[0];
}
__device__ __forceinline__ double block_max(double v, double* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  for (int o = REG_T / 2; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] = fmax(s_red[tid], s_red[tid + o]);
    __syncthreads();
  }
  return s_red[0];
}

// s_i = mean_m d[i,m], m = 1..k, into s_s [N]; returns thr = mean_i s + coef * std_i s (unbiased, as torch.std).
// A thread reads back only the entries it wrote.
__device__ float smooth_stats(const float* __restrict__ D, int N, int k, int ld, float coef, float* s_s, double* s_red) {
  const int tid = threadIdx.x;
  const float kf = (float)k;
  double v = 0.0;
  for (int i = tid; i < N; i += REG_T) {
    const float* r = D + (size_t)i * ld;
    double acc = 0.0;                                   // (k terms in double: s_i is the rounded exact mean)
    for (int m = 1; m <= k; ++m) acc += (double)r[m];
    const float a = (float)(acc / (double)kf);
    s_s[i] = a;
    v += (double)a;
  }
  const double mean = block_sum(v, s_red) / (double)N;
  double q = 0.0;
  for (int i = tid; i < N; i += REG_T) {
    const double t = (double)s_s[i] - mean;
    q += t * t;
  }
  const double var = block_sum(q, s_red) / (double)(N - 1);
  return (float)mean + coef * (float)sqrt(var);
}

__device__ __forceinline__ bool cloud_bad(const float* __restrict__ P, int N) {
  bool bad = false;
  for (int i = threadIdx.x; i < 3 * N; i += REG_T) bad = bad || geoa3_nonfinite(P[i]);
  return bad;
}

// kNN_smoothing_loss: loss[b] = (1/N) sum_i s_i [s_i > thr]; cond [B,N] (optional) = the mask
__global__ __launch_bounds__(REG_T) void smooth_fwd_kernel(const float* __restrict__ pc, const float* __restrict__ knn_d,
                                                           int N, int k, int ld, float coef, float* __restrict__ loss,
                                                           uint8_t* __restrict__ cond) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_red[REG_T];
  float* s_s = reinterpret_cast<float*>(s_raw);
  const int b = blockIdx.x, tid = threadIdx.x;
  if (__syncthreads_or(cloud_bad(pc + (size_t)b * 3 * N, N))) {
    if (tid == 0) loss[b] = __builtin_nanf("");
    if (cond)
      for (int i = tid; i < N; i += REG_T) cond[(size_t)b * N + i] = 0;
    return;
  }
  const float thr = smooth_stats(knn_d + (size_t)b * N * ld, N, k, ld, coef, s_s, s_red);
  if (thr != thr) {                                     // (the same in every thread: block_sum's result)
    if (tid == 0) loss[b] = __builtin_nanf("");
    if (cond)
      for (int i = tid; i < N; i += REG_T) cond[(size_t)b * N + i] = 0;
    return;
  }
  double v = 0.0;
  for (int i = tid; i < N; i += REG_T) {
    const float s = s_s[i];
    const bool c = s > thr;
    if (cond) cond[(size_t)b * N + i] = c ? 1 : 0;
    if (c) v += (double)s;
  }
  const double tot = block_sum(v, s_red);
  if (tid == 0) loss[b] = (float)(tot / (double)N);
}

// repulsion_loss: out[b,i] = -mean_m d exp(-d^2 / h^2)   (d: the SQUARED distance, squared again, as the reference)
__global__ __launch_bounds__(REG_T) void repulse_fwd_kernel(const float* __restrict__ pc, const float* __restrict__ knn_d,
                                                            int N, int k, int ld, float h2, float* __restrict__ out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool bad = __syncthreads_or(cloud_bad(pc + (size_t)b * 3 * N, N));
  const float* D = knn_d + (size_t)b * N * ld;
  const float kf = (float)k;
  for (int i = tid; i < N; i += REG_T) {
    const float* r = D + (size_t)i * ld;
    double a = 0.0;
    for (int m = 1; m <= k; ++m) {
      const float d = r[m];
      a += (double)(d * expf(-(d * d) / h2));
    }
    out[(size_t)b * N + i] = bad ? __builtin_nanf("") : -(float)(a / (double)kf);
  }
}

// displacement_loss: theta_i = |adv_i - ori_i|^2, out[b,i] = mean_m (theta_j(i,m) - theta_i)^2, j from ori's table
__global__ __launch_bounds__(REG_T) void displace_fwd_kernel(const float* __restrict__ adv, const float* __restrict__ ori,
                                                             const int32_t* __restrict__ knn_i, int N, int k, int ld,
                                                             float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float* s_th = reinterpret_cast<float*>(s_raw);
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* A = adv + (size_t)b * 3 * N;
  const float* O = ori + (size_t)b * 3 * N;
  bool bad = false;
  for (int i = tid; i < N; i += REG_T) {
    const float th = geoa3_sqdist(A[i], A[N + i], A[2 * N + i], O[i], O[N + i], O[2 * N + i]);
    s_th[i] = th;
    bad = bad || geoa3_nonfinite(th);
  }
  const int32_t* I = knn_i + (size_t)b * N * ld;
  const float kf = (float)k;
  // (the barrier of __syncthreads_or also publishes theta)
  bad = __syncthreads_or(bad);
  for (int i = tid; i < N; i += REG_T) {
    const int32_t* r = I + (size_t)i * ld;
    const float ti = s_th[i];
    double a = 0.0;
    bool oob = false;
    for (int m = 1; m <= k; ++m) {
      const int j = r[m];
      if ((unsigned)j >= (unsigned)N) {
        oob = true;
        continue;
      }
      const float t = s_th[j] - ti;
      a += (double)(t * t);
    }
    out[(size_t)b * N + i] = (bad || oob) ? __builtin_nanf("") : (float)(a / (double)kf);
  }
}

struct RegBwd {
  const float* pc;         // the cloud the gradient is taken at (displacement_loss: adv)
  const float* ori;        // displacement_loss: the clean cloud; corresponding_normal_loss: the normals [B,3,N]
  const float* knn_d;      // [B,N,ld]
  const int32_t* knn_i;    // [B,N,ld]
  const float* g;          // upstream gradient: [B] (kNN_smoothing_loss) / [B,N]; NULL = ones
  float* grad;             // [B,3,N]
  unsigned long long* gacc;   // [B,3,N] fixed-point sums of the !LDS form
  int N, k, ld;
  float coef, h2;
};

// LDS: [sums NA x N int64 (LDS)] [x y z, N floats each (LDS, not displacement)] [aux]
//   aux of kNN_smoothing_loss: the mask, N bytes (s_i, N floats, sits in the sums' space before they are cleared; !LDS: in
//   front of the mask); of displacement_loss: theta, N doubles
template <int MODE, bool LDS>
__global__ __launch_bounds__(REG_T) void reg_bwd_kernel(RegBwd p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_red[REG_T];
  constexpr int NA = MODE == REG_DISPLACE ? 1 : 3;
  constexpr bool CLOUD = LDS && MODE != REG_DISPLACE;
  const int b = blockIdx.x, tid = threadIdx.x, N = p.N, k = p.k, ld = p.ld;
  unsigned long long* acc = LDS ? reinterpret_cast<unsigned long long*>(s_raw) : p.gacc + (size_t)b * 3 * N;
  unsigned char* q = s_raw + (LDS ? (size_t)NA * N * 8 : 0);
  const float* X = p.pc + (size_t)b * 3 * N;
  float* s_x = reinterpret_cast<float*>(q);
  if (CLOUD) q += (size_t)3 * N * sizeof(float);
  const float* cx = CLOUD ? s_x : X;                    // planes x, y, z at cx, cx + N, cx + 2N
  float* s_s = LDS ? reinterpret_cast<float*>(s_raw) : reinterpret_cast<float*>(q);   // (kNN_smoothing_loss)
  if (MODE == REG_SMOOTH && !LDS) q += (size_t)N * sizeof(float);
  unsigned char* s_c = q;                               // (kNN_smoothing_loss)
  double* s_th = reinterpret_cast<double*>(q);          // (displacement_loss: theta in double, its differences cancel)
  const float* D = p.knn_d + (size_t)b * N * ld;
  const int32_t* I = p.knn_i + (size_t)b * N * ld;
  float* G = p.grad + (size_t)b * 3 * N;

  bool bad = false;
  if (MODE == REG_DISPLACE) {
    const float* O = p.ori + (size_t)b * 3 * N;
    for (int i = tid; i < N; i += REG_T) {
      const double dx = (double)X[i] - (double)O[i], dy = (double)X[N + i] - (double)O[N + i],
                   dz = (double)X[2 * N + i] - (double)O[2 * N + i];
      const double th = dx * dx + dy * dy + dz * dz;
      s_th[i] = th;
      bad = bad || geoa3_nonfinite((float)th);           // (NaN, infinite, or beyond what the forward's float theta holds)
    }
  } else {
    for (int i = tid; i < 3 * N; i += REG_T) {
      const float v = X[i];
      if (CLOUD) s_x[i] = v;
      bad = bad || geoa3_nonfinite(v);
    }
  }
  if (MODE == REG_SMOOTH) {
    const float thr = smooth_stats(D, N, k, ld, p.coef, s_s, s_red);
    bad = bad || thr != thr;                             // (a non-finite distance in the table: the instance is refused below)
    for (int i = tid; i < N; i += REG_T) s_c[i] = s_s[i] > thr ? 1 : 0;
  }
  __syncthreads();                                      // s_s is dead: its space becomes the sums
  for (int i = tid; i < NA * N; i += REG_T) {
    if (LDS) acc[i] = 0ull;
    else __hip_atomic_store(acc + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();

  // pair coefficients and terms in double: the coordinates' differences are exact there, and a term goes to fixed point
  // without a float rounding in between
  const double kd = (double)k;
  const double gb = (MODE == REG_SMOOTH) ? (double)(p.g ? p.g[b] : 1.f) / ((double)N * kd) : 0.0;
  const float* gp = (MODE != REG_SMOOTH && p.g) ? p.g + (size_t)b * N : nullptr;
  const double h2 = (double)p.h2;
  const int pairs = N * k;
  // the term of pair e = (i, m): false when the neighbour index lies outside the cloud
  auto term = [&](int e, int& i, int& j, double& t0, double& t1, double& t2) -> bool {
    i = e / k;
    const int m = e - i * k + 1;
    j = I[(size_t)i * ld + m];
    if ((unsigned)j >= (unsigned)N) return false;
    if (MODE == REG_DISPLACE) {
      t0 = (2.0 / kd) * (s_th[j] - s_th[i]) * (double)(gp ? gp[i] : 1.f);
      t1 = t2 = 0.0;
      return true;
    }
    const double dx = (double)cx[i] - (double)cx[j], dy = (double)cx[N + i] - (double)cx[N + j],
                 dz = (double)cx[2 * N + i] - (double)cx[2 * N + j];
    if (MODE == REG_NORMAL) {
      // out_i = mean_m |t|, t = <v / max(|v|, eps), n_i>, v = x_j - x_i:  d|t|/dx_j = sign(t) (n_i - t v^) / |v| (|v| > eps;
      // sign(0) = 0 as torch.abs's backward), and the opposite on x_i -- the term ADDED to point i
      const float* Nm = p.ori + (size_t)b * 3 * N;
      const double nx = (double)Nm[i], ny = (double)Nm[N + i], nz = (double)Nm[2 * N + i];
      const double r = sqrt(dx * dx + dy * dy + dz * dz);
      const double inv = 1.0 / fmax(r, REG_NORM_EPS);
      const double ux = -dx * inv, uy = -dy * inv, uz = -dz * inv;       // v^
      const double t = ux * nx + uy * ny + uz * nz;
      const double sg = t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : 0.0);
      const double c = -(sg * inv / kd) * (double)(gp ? gp[i] : 1.f);
      const double tt = r > REG_NORM_EPS ? t : 0.0;                       // (clamped length: v^ = v / eps is linear in v)
      t0 = c * (nx - tt * ux);
      t1 = c * (ny - tt * uy);
      t2 = c * (nz - tt * uz);
      return true;                                        // (a NaN normal gives NaN terms: the instance is refused below)
    }
    double w;
    if (MODE == REG_SMOOTH) {
      w = s_c[i] ? gb : 0.0;
    } else {                                              // (repulsion: the squared distance again in double, from the cloud)
      const double d = dx * dx + dy * dy + dz * dz;
      const double u = (d * d) / h2;
      w = (double)(gp ? gp[i] : 1.f) * (-(1.0 / kd)) * exp(-u) * (1.0 - 2.0 * u);
    }
    const double w2 = 2.0 * w;
    t0 = w2 * dx;
    t1 = w2 * dy;
    t2 = w2 * dz;
    return true;
  };

  double mx = 0.0;
  for (int e = tid; e < pairs; e += REG_T) {
    int i, j;
    double t0, t1, t2;
    if (!term(e, i, j, t0, t1, t2)) {
      bad = true;
      continue;
    }
    const double a0 = fabs(t0), a1 = fabs(t1), a2 = fabs(t2);
    bad = bad || !(a0 <= 1e300) || !(a1 <= 1e300) || !(a2 <= 1e300);   // NaN, infinite, or beyond any float gradient
    mx = fmax(mx, fmax(a0, fmax(a1, a2)));
  }
  if (__syncthreads_or(bad)) {
    for (int i = tid; i < 3 * N; i += REG_T) G[i] = __builtin_nanf("");
    return;
  }
  mx = block_max(mx, s_red);
  const int ex = mx > 0.0 ? ilogb(mx) : 0;
  const double scale = ldexp(1.0, REG_FX_BITS - ex), inv = ldexp(1.0, ex - REG_FX_BITS);
  for (int e = tid; e < pairs; e += REG_T) {
    int i, j;
    double t[3];
    term(e, i, j, t[0], t[1], t[2]);
    if (i == j) continue;                                // +t and -t on the same point
#pragma unroll
    for (int c = 0; c < NA; ++c) {
      const long long v = __double2ll_rn(t[c] * scale);
      if (v != 0) {
        if (MODE == REG_DISPLACE) {                      // d theta_i -= t, d theta_j += t
          atomicAdd(acc + i, (unsigned long long)(-v));
          atomicAdd(acc + j, (unsigned long long)v);
        } else {
          atomicAdd(acc + c * N + i, (unsigned long long)v);
          atomicAdd(acc + c * N + j, (unsigned long long)(-v));
        }
      }
    }
  }
  __syncthreads();
  auto sum_of = [&](int i) -> double {
    const unsigned long long a = LDS ? acc[i] : __hip_atomic_load(acc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (double)(long long)a * inv;
  };
  if (MODE == REG_DISPLACE) {                            // d adv_i = 2 (adv_i - ori_i) d theta_i
    const float* O = p.ori + (size_t)b * 3 * N;
    for (int i = tid; i < N; i += REG_T) {
      const double dth = sum_of(i);
#pragma unroll
      for (int c = 0; c < 3; ++c) G[c * N + i] = (float)(2.0 * ((double)X[c * N + i] - (double)O[c * N + i]) * dth);
    }
  } else {
    for (int i = tid; i < 3 * N; i += REG_T) G[i] = (float)sum_of(i);
  }
}

// constrain[b] (+)= w * loss[b];  g (+)= w * grad
__global__ __launch_bounds__(256) void reg_fold_kernel(const float* __restrict__ loss, const float* __restrict__ grad, float w,
                                                       int B, size_t total, float* __restrict__ constrain, int constrain_add,
                                                       float* __restrict__ g, int g_add) {
  const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (constrain && t0 < (size_t)B) {
    const float v = w * loss[t0];
    constrain[t0] = constrain_add ? constrain[t0] + v : v;
  }
  if (!g) return;
  for (size_t i = t0; i < total; i += (size_t)gridDim.x * 256) {
    const float v = w * grad[i];
    g[i] = g_add ? g[i] + v : v;
  }
}

// A per-point term out [B,N] through its row mean: one workgroup per row.  The mean is summed in double as block_sum
// does (thread t takes points t, t + 512, ...: the order depends on N only) and rounded to float once; w * term and
// (w / N) * grad are formed and added in double and rounded once.  A NaN mean (a non-finite coordinate upstream) makes the
// row's whole g NaN, whatever grad holds: "a NaN row stays NaN".  VEC: rows of g / grad are float4-addressable.
template <bool VEC>
__global__ __launch_bounds__(REG_T) void reg_fold_points_kernel(const float* __restrict__ out, const float* __restrict__ grad,
                                                                float w, int N, float* __restrict__ term,
                                                                float* __restrict__ constrain, int constrain_add,
                                                                float* __restrict__ g, int g_add) {
  __shared__ double s_red[REG_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  bool nan_row = false;
  if (out) {
    const float* O = out + (size_t)b * N;
    double v = 0.0;
    for (int i = tid; i < N; i += REG_T) v += (double)O[i];
    const float mean = (float)(block_sum(v, s_red) / (double)N);
    nan_row = mean != mean;
    if (tid == 0) {
      if (term) term[b] = mean;
      if (constrain) constrain[b] = (float)((constrain_add ? (double)constrain[b] : 0.0) + (double)w * (double)mean);
    }
  }
  if (!g) return;
  const double wn = (double)w / (double)N;
  const float qnan = __builtin_nanf("");
  const float* S = grad + (size_t)b * 3 * N;
  float* G = g + (size_t)b * 3 * N;
  auto fold = [&](float gv, float sv) -> float {
    return nan_row ? qnan : (float)((g_add ? (double)gv : 0.0) + wn * (double)sv);
  };
  if (VEC) {
    const float4* S4 = reinterpret_cast<const float4*>(S);
    float4* G4 = reinterpret_cast<float4*>(G);
    for (int i = tid; i < 3 * (N / 4); i += REG_T) {
      const float4 s = S4[i];
      float4 r = g_add ? G4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      r.x = fold(r.x, s.x);
      r.y = fold(r.y, s.y);
      r.z = fold(r.z, s.z);
      r.w = fold(r.w, s.w);
      G4[i] = r;
    }
  } else {
    for (int i = tid; i < 3 * N; i += REG_T) G[i] = fold(g_add ? G[i] : 0.f, S[i]);
  }
}

size_t reg_lds_bwd(int mode, int N) {   // dynamic LDS of the LDS form
  if (mode == REG_DISPLACE) return (size_t)N * 16;
  return (size_t)N * (mode == REG_SMOOTH ? 37 : 36);
}

// the one predicate of launch_reg_bwd, geoa3_reg_workspace_bytes and geoa3_debug_reg_route
bool reg_sums_in_lds(int mode, int N) { return reg_lds_bwd(mode, N) <= REG_LDS_MAX; }

int reg_check(int B, int N, int k) {
  if (B <= 0 || N <= 0 || k < 1) return GEOA3_EINVAL;
  if (k + 1 > GEOA3_KNN_MAX_K || N > REG_MAX_N) return GEOA3_ENOSUPPORT;
  if (N < k + 1) return GEOA3_EINVAL;
  return GEOA3_OK;
}

// workspace: [table dists B x N x (k+1) float] [table idx] [sums B x 3N int64 (clouds whose sums do not fit in LDS)]
struct RegWs {
  float* d;
  int32_t* i;
  unsigned long long* acc;
};
RegWs reg_ws(void* ws, int B, int N, int k) {
  unsigned char* p = static_cast<unsigned char*>(ws);
  RegWs w;
  w.d = reinterpret_cast<float*>(p);
  p += align256((size_t)B * N * (k + 1) * sizeof(float));
  w.i = reinterpret_cast<int32_t*>(p);
  p += align256((size_t)B * N * (k + 1) * sizeof(int32_t));
  w.acc = reinterpret_cast<unsigned long long*>(p);
  return w;
}

// the caller's table, or geoa3_knn_self of `cloud` into the workspace
int reg_table(const float* cloud, int B, int N, int k, const float** d, const int32_t** i, int* ld, void* ws, void* stream) {
  if (*d && *i) {
    if (*ld == 0) *ld = k + 1;
    return *ld < k + 1 ? GEOA3_EINVAL : GEOA3_OK;
  }
  if (*d || *i || !ws) return GEOA3_EINVAL;
  const RegWs w = reg_ws(ws, B, N, k);
  *d = w.d;
  *i = w.i;
  *ld = k + 1;
  return geoa3_knn_self(cloud, B, N, k + 1, nullptr, w.d, w.i, nullptr, 0, stream);
}

template <int MODE>
int launch_reg_bwd(RegBwd p, int B, void* ws, hipStream_t s) {
  const size_t lds = reg_lds_bwd(MODE, p.N);
  if (reg_sums_in_lds(MODE, p.N)) {
    auto kern = reg_bwd_kernel<MODE, true>;
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(B), dim3(REG_T), lds, s, p);
  } else {
    if (!ws) return GEOA3_EINVAL;
    p.gacc = reg_ws(ws, B, p.N, p.k).acc;
    const size_t small = MODE == REG_SMOOTH ? (size_t)p.N * 5 : 0;
    hipLaunchKernelGGL((reg_bwd_kernel<MODE, false>), dim3(B), dim3(REG_T), small, s, p);
  }
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

}  // namespace

extern "C" int64_t geoa3_reg_workspace_bytes(int B, int N, int k) {
  if (reg_check(B, N, k) != GEOA3_OK) return 0;
  size_t n = 2 * align256((size_t)B * N * (k + 1) * sizeof(float));
  // (kNN_smoothing_loss has the largest footprint per point: the first mode to leave LDS)
  if (!reg_sums_in_lds(REG_SMOOTH, N)) n += (size_t)B * 3 * N * sizeof(unsigned long long);
  return (int64_t)n;
}

extern "C" int geoa3_debug_reg_route(int mode, int N, int k) {
  if (mode < REG_SMOOTH || mode > REG_NORMAL || reg_check(1, N, k) != GEOA3_OK) return GEOA3_REG_ROUTE_REFUSED;
  return reg_sums_in_lds(mode, N) ? GEOA3_REG_ROUTE_LDS : GEOA3_REG_ROUTE_WORKSPACE;
}

extern "C" int geoa3_knn_smoothing_loss(const float* pc, int B, int N, int k, float coef, const float* knn_d,
                                        const int32_t* knn_i, int knn_ld, float* loss, uint8_t* cond, void* workspace,
                                        void* stream) {
  if (!pc || !loss) return GEOA3_EINVAL;
  int rc = reg_check(B, N, k);
  if (rc != GEOA3_OK) return rc;
  rc = reg_table(pc, B, N, k, &knn_d, &knn_i, &knn_ld, workspace, stream);
  if (rc != GEOA3_OK) return rc;
  hipLaunchKernelGGL(smooth_fwd_kernel, dim3(B), dim3(REG_T), (size_t)N * sizeof(float), geoa3_stream(stream), pc, knn_d, N,
                     k, knn_ld, coef, loss, cond);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_knn_smoothing_loss_grad(const float* pc, int B, int N, int k, float coef, const float* knn_d,
                                             const int32_t* knn_i, int knn_ld, const float* g, float* grad, void* workspace,
                                             void* stream) {
  if (!pc || !grad) return GEOA3_EINVAL;
  int rc = reg_check(B, N, k);
  if (rc != GEOA3_OK) return rc;
  rc = reg_table(pc, B, N, k, &knn_d, &knn_i, &knn_ld, workspace, stream);
  if (rc != GEOA3_OK) return rc;
  RegBwd p = {pc, nullptr, knn_d, knn_i, g, grad, nullptr, N, k, knn_ld, coef, 0.f};
  return launch_reg_bwd<REG_SMOOTH>(p, B, workspace, geoa3_stream(stream));
}

extern "C" int geoa3_repulsion_loss(const float* pc, int B, int N, int k, float h, const float* knn_d, const int32_t* knn_i,
                                    int knn_ld, float* out, void* workspace, void* stream) {
  if (!pc || !out || !(h > 0.f)) return GEOA3_EINVAL;
  int rc = reg_check(B, N, k);
  if (rc != GEOA3_OK) return rc;
  rc = reg_table(pc, B, N, k, &knn_d, &knn_i, &knn_ld, workspace, stream);
  if (rc != GEOA3_OK) return rc;
  const float h2 = (float)((double)h * (double)h);
  hipLaunchKernelGGL(repulse_fwd_kernel, dim3(B), dim3(REG_T), 0, geoa3_stream(stream), pc, knn_d, N, k, knn_ld, h2, out);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_repulsion_loss_grad(const float* pc, int B, int N, int k, float h, const float* knn_d,
                                         const int32_t* knn_i, int knn_ld, const float* g, float* grad, void* workspace,
                                         void* stream) {
  if (!pc || !grad || !(h > 0.f)) return GEOA3_EINVAL;
  int rc = reg_check(B, N, k);
  if (rc != GEOA3_OK) return rc;
  rc = reg_table(pc, B, N, k, &knn_d, &knn_i, &knn_ld, workspace, stream);
  if (rc != GEOA3_OK) return rc;
  RegBwd p = {pc, nullptr, knn_d, knn_i, g, grad, nullptr, N, k, knn_ld, 0.f, (float)((double)h * (double)h)};
  return launch_reg_bwd<REG_REPULSE>(p, B, workspace, geoa3_stream(stream));
}

extern "C" int geoa3_corr_normal_loss_grad(const float* pc, const float* normal, int B, int N, int k, const float* knn_d,
                                           const int32_t* knn_i, int knn_ld, const float* g, float* grad, void* workspace,
                                           void* stream) {
  if (!pc || !normal || !grad) return GEOA3_EINVAL;
  int rc = reg_check(B, N, k);
  if (rc != GEOA3_OK) return rc;
  rc = reg_table(pc, B, N, k, &knn_d, &knn_i, &knn_ld, workspace, stream);
  if (rc != GEOA3_OK) return rc;
  RegBwd p = {pc, normal, knn_d, knn_i, g, grad, nullptr, N, k, knn_ld, 0.f, 0.f};
  return launch_reg_bwd<REG_NORMAL>(p, B, workspace, geoa3_stream(stream));
}

extern "C" int geoa3_displacement_loss(const float* adv, const float* ori, int B, int N, int k, const float* knn_d,
                                       const int32_t* knn_i, int knn_ld, float* out, void* workspace, void* stream) {
  if (!adv || !ori || !out) return GEOA3_EINVAL;
  int rc = reg_check(B, N, k);
  if (rc != GEOA3_OK) return rc;
  rc = reg_table(ori, B, N, k, &knn_d, &knn_i, &knn_ld, workspace, stream);
  if (rc != GEOA3_OK) return rc;
  hipLaunchKernelGGL(displace_fwd_kernel, dim3(B), dim3(REG_T), (size_t)N * sizeof(float), geoa3_stream(stream), adv, ori,
                     knn_i, N, k, knn_ld, out);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_displacement_loss_grad(const float* adv, const float* ori, int B, int N, int k, const float* knn_d,
                                            const int32_t* knn_i, int knn_ld, const float* g, float* grad, void* workspace,
                                            void* stream) {
  if (!adv || !ori || !grad) return GEOA3_EINVAL;
  int rc = reg_check(B, N, k);
  if (rc != GEOA3_OK) return rc;
  rc = reg_table(ori, B, N, k, &knn_d, &knn_i, &knn_ld, workspace, stream);
  if (rc != GEOA3_OK) return rc;
  RegBwd p = {adv, ori, knn_d, knn_i, g, grad, nullptr, N, k, knn_ld, 0.f, 0.f};
  return launch_reg_bwd<REG_DISPLACE>(p, B, workspace, geoa3_stream(stream));
}

extern "C" int geoa3_reg_fold(const float* loss, const float* grad, float w, int B, int N, float* constrain,
                              int constrain_add, float* g, int g_add, void* stream) {
  if (B <= 0 || N <= 0 || (!constrain && !g) || (constrain && !loss) || (g && !grad)) return GEOA3_EINVAL;
  const size_t total = (size_t)B * 3 * N;
  size_t blocks = g ? (total + 255) / 256 : (size_t)(B + 255) / 256;
  if (blocks < (size_t)(B + 255) / 256) blocks = (size_t)(B + 255) / 256;
  if (blocks > 2048 && (size_t)B <= 2048 * 256) blocks = 2048;
  hipLaunchKernelGGL(reg_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, geoa3_stream(stream), loss, grad, w, B, total,
                     constrain, constrain_add, g, g_add);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_reg_fold_points(const float* out, const float* grad, float w, int B, int N, float* term,
                                     float* constrain, int constrain_add, float* g, int g_add, void* stream) {
  if (B <= 0 || N <= 0 || (!term && !constrain && !g) || ((term || constrain) && !out) || (g && !grad)) return GEOA3_EINVAL;
  if (N > (1 << 28)) return GEOA3_ENOSUPPORT;           // (3 N stays an int)
  const bool vec = g && N % 4 == 0 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(grad)) & 15) == 0;
  auto kern = vec ? reg_fold_points_kernel<true> : reg_fold_points_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(REG_T), 0, geoa3_stream(stream), out, grad, w, N, term, constrain,
                     constrain_add, g, g_add);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
