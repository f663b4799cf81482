// The 1024-wide PointNet layers in TRAINING mode, fused with BatchNorm's batch statistics and the max over points
// (gfx950, fp32 MFMA): conv(128 -> 1024, TAPS) -> BatchNorm1d(train) -> [relu] -> max, Model/PointNet.py:81-82 (T-Net
// conv3 + bn3, one tap) and :146-147 (conv5 + bn5, three taps, zero padded).  y = W U [B,1024,N] is never written.
//
// Forward, one MFMA pass (wt_fwd_kernel): a workgroup owns (instance, 64-point tile, all 1024 channels), stages the
// activation tile once (the LDS image and the operand roles of wide_max2_kernel, pointnet_wide.hip: activations as A,
// weight fragments from L2 as B, so a lane holds ONE channel and 32 of the tile's points) and leaves per (tile, channel):
//   sum and sum of squares of d = y - shift[c] over the tile's valid points (shift = W mean(U): the caller's estimate of
//   the channel mean, which keeps the variance a sum of squares of SMALL numbers), the first maximum and the first minimum
//   of y with their points, and y at the tile's first point.
// The conv bias is not an input: BatchNorm removes it (out and every gradient are independent of it).
// BN followed by relu is monotone in y, so the pooled output needs one y per (instance, channel): the maximum where
// gamma > 0, the minimum where gamma < 0, point 0 where gamma == 0 (torch's max of a constant row takes index 0).
// No atomics: the tiles' partial results are combined in tile order (wt_stats_kernel: double sums in a fixed order that
// depends on B and N only; wt_select_kernel: strict comparisons in ascending tile order, so equal values go to the lower
// point).  The same input gives the same bits.
// Non-finite: fmaxf drops a NaN, the sums do not -- a channel whose sum or sum of squares is not finite gets NaN in
// every out[:, c] (and NaN statistics), as torch's batch_norm gives.
//
// Backward, the two sparse pieces (the dense 128 / 384-wide products are the caller's):
//   wt_gather_kernel:  dWg[c][k] = sum_b coef[b][c] U[b][k][arg[b][c]], b ascending;
//   wt_scatter_kernel: dX[b][ci][q] = sum_{c, tap: arg[b][c] + tap - TAPS/2 == q} coef[b][c] W[c][tap*128 + ci], summed in
//                      (c, tap) ascending order.  (launch_wide_max_bwd computes the same sum but multiplies by the relu
//                      gate of the layer INPUT, which belongs to the eval-mode chain; this layer's input gate is autograd's.)
#include "pointnet_kernels.h"
#include "wide_epilogue.h"

namespace {

constexpr int WT_CO = 1024, WT_CI = 128, WT_THREADS = 256;
constexpr int WT_COLS = 64, WT_HALO = 4, WT_XP = WT_COLS + 2 * WT_HALO;   // 72
constexpr int WT_PF = 5, WT_PI = 2;   // floats / ints per (tile, channel): sum, sumsq, max, min, y(first point); arg max, arg min

// [Co][TAPS*128] -> the fragment order of pointnet_wide.hip (pack_wide_fragments of geoa3_amd/pointnet.py), on the device:
// the weights change every optimiser step
__global__ __launch_bounds__(256) void wt_pack_kernel(const float* __restrict__ W, float4* __restrict__ Wp, int taps) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // ((T*taps + tap)*16 + j)*64 + lane
  if (e >= WT_CO * taps * 32) return;
  const int lane = e & 63, j = (e >> 6) & 15, tt = e >> 10, tap = tt % taps, T = tt / taps;
  Wp[e] = *reinterpret_cast<const float4*>(W + (size_t)(32 * T + (lane & 31)) * (taps * 128) + tap * 128 + 8 * j + 4 * (lane >> 5));
}

template <int TAPS>
__global__ __launch_bounds__(WT_THREADS, 2) void wt_fwd_kernel(const float* __restrict__ Xall, const float4* __restrict__ Wp,
                                                               const float* __restrict__ shift, int N,
                                                               float* __restrict__ pf, int* __restrict__ pi) {
  constexpr int NGT = TAPS * 16;   // fragment groups (8 k each) of one channel tile
  constexpr int PF = 4;            // fragment loads in flight
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [128][WT_XP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 5, l31 = lane & 31;
  const int tile = blockIdx.x, b = blockIdx.y, n0 = tile * WT_COLS;
  const size_t unit = (size_t)b * gridDim.x + tile;
  const float* X = Xall + (size_t)b * WT_CI * N;
  {
    const bool xvec = (N & 3) == 0;
    for (int e = tid; e < WT_CI * (WT_XP / 4); e += WT_THREADS) {
      const int qd = e % (WT_XP / 4), c = e / (WT_XP / 4);
      const int n = n0 - WT_HALO + qd * 4;
      const float* src = X + (size_t)c * N;
      float4 v;
      if (xvec && n >= 0 && n + 3 < N) {
        v = *reinterpret_cast<const float4*>(src + n);
      } else {
        v.x = (n >= 0 && n < N) ? src[n] : 0.f;
        v.y = (n + 1 >= 0 && n + 1 < N) ? src[n + 1] : 0.f;
        v.z = (n + 2 >= 0 && n + 2 < N) ? src[n + 2] : 0.f;
        v.w = (n + 3 >= 0 && n + 3 < N) ? src[n + 3] : 0.f;
      }
      *reinterpret_cast<float4*>(smem + c * WT_XP + qd * 4) = v;
    }
  }
  __syncthreads();
  const float* xb = smem + kh * 4 * WT_XP + WT_HALO + l31 - TAPS / 2;
  auto wbase = [&](int g) { return Wp + (size_t)((g * 128 + wave * 32) / 32) * NGT * 64 + lane; };
  float4 wf[PF];
  {
    const float4* W0 = wbase(0);
#pragma unroll
    for (int f = 0; f < PF; ++f) wf[f] = W0[(size_t)f * 64];
  }
  const int left = N - n0 - 4 * kh;   // the lane's local point i (below) is valid when i < left
#pragma unroll 1
  for (int g = 0; g < 8; ++g) {
    const int c = g * 128 + wave * 32 + l31;
    const float4* Wg = wbase(g);
    const float4* Wn = wbase(g + 1 < 8 ? g + 1 : g);
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acc[0][i] = 0.f;
      acc[1][i] = 0.f;
    }
    float bq[8], bn[8];
    auto read_b = [&](int f, float* d) {   // fragment group f = tap*16 + jj: rows 8jj + 4kh + i, column shift tap
      const int tap = f >> 4, jj = f & 15;
      const float* xp = xb + jj * 8 * WT_XP + tap;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        d[2 * i] = xp[i * WT_XP];
        d[2 * i + 1] = xp[i * WT_XP + 32];
      }
    };
    read_b(0, bq);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < NGT; ++f) {
      const float4 w = wf[f % PF];
      if (f + PF < NGT) wf[f % PF] = Wg[(size_t)(f + PF) * 64];
      else wf[f % PF] = Wn[(size_t)(f + PF - NGT) * 64];
      if (f + 1 < NGT) read_b(f + 1, bn);
      __builtin_amdgcn_sched_barrier(0);
      const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[0] = mfma32(bq[2 * i], wv[i], acc[0]);   // rows = points, columns = channels
        acc[1] = mfma32(bq[2 * i + 1], wv[i], acc[1]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 8; ++i) bq[i] = bn[i];
    }
    // lane: channel c; value i (< 32, ascending point order): acc[i >> 4][i & 15] at local point loc(i) + 4 kh
    auto loc = [](int i) { return 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2); };
    const float sh = shift[c];
    const float y0 = acc[0][0];
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const float d = loc(i) < left ? acc[i >> 4][i & 15] - sh : 0.f;
      s += d;
      q = __builtin_fmaf(d, d, q);
    }
    float vmax, vmin;
    int imax, imin;
    wide_lane_first_max<32>([&](int i) { return loc(i) < left ? acc[i >> 4][i & 15] : -__builtin_inff(); }, loc, vmax, imax);
    wide_lane_first_max<32>([&](int i) { return loc(i) < left ? -acc[i >> 4][i & 15] : -__builtin_inff(); }, loc, vmin, imin);
    imax += n0 + 4 * kh;
    imin += n0 + 4 * kh;
    {
      s += __shfl_xor(s, 32, 64);
      q += __shfl_xor(q, 32, 64);
      float ov = __shfl_xor(vmax, 32, 64);
      int oc = __shfl_xor(imax, 32, 64);
      bool take = wide_merge_take(ov, oc, vmax, imax);
      vmax = take ? ov : vmax;
      imax = take ? oc : imax;
      ov = __shfl_xor(vmin, 32, 64);
      oc = __shfl_xor(imin, 32, 64);
      take = wide_merge_take(ov, oc, vmin, imin);
      vmin = take ? ov : vmin;
      imin = take ? oc : imin;
    }
    if (lane < 32) {
      float* f = pf + unit * (WT_PF * WT_CO) + c;
      f[0] = s;
      f[WT_CO] = q;
      f[2 * WT_CO] = vmax;
      f[3 * WT_CO] = -vmin;
      f[4 * WT_CO] = y0;
      int* ip = pi + unit * (WT_PI * WT_CO) + c;
      ip[0] = imax;
      ip[WT_CO] = imin;
    }
  }
}

// per channel: the tiles' sums -> dm = mean(y) - shift and the biased variance, in double, in a fixed order: wave w of
// the 16 adds the units w, w + 16, .. in ascending order, then the 16 partial sums are added in wave order.
// stat[c] = {dm, var, bad}
__global__ __launch_bounds__(1024) void wt_stats_kernel(const float* __restrict__ pf, int units, double M, double* __restrict__ stat) {
  __shared__ double s_s[16][64], s_q[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  double S = 0., Q = 0.;
  for (int u = wave; u < units; u += 16) {
    const float* f = pf + (size_t)u * (WT_PF * WT_CO) + c;
    S += (double)f[0];
    Q += (double)f[WT_CO];
  }
  s_s[wave][lane] = S;
  s_q[wave][lane] = Q;
  __syncthreads();
  if (wave == 0) {
    S = 0., Q = 0.;
    for (int w = 0; w < 16; ++w) {
      S += s_s[w][lane];
      Q += s_q[w][lane];
    }
    const bool bad = !(__builtin_fabs(S) <= 1.7976931348623157e308) || !(__builtin_fabs(Q) <= 1.7976931348623157e308);
    const double dm = S / M;
    double var = Q / M - dm * dm;
    var = var < 0. ? 0. : var;
    stat[c] = dm;
    stat[WT_CO + c] = var;
    stat[2 * WT_CO + c] = bad ? 1. : 0.;
  }
}

// per (instance, channel): the selected y over the tiles in ascending order, normalised and activated
__global__ __launch_bounds__(256) void wt_select_kernel(const float* __restrict__ pf, const int* __restrict__ pi,
                                                        const double* __restrict__ stat, const float* __restrict__ shift,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, int relu, int tiles, float* __restrict__ out,
                                                        int* __restrict__ arg, float* __restrict__ xhat,
                                                        float* __restrict__ mean, float* __restrict__ var) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const double dm = stat[c], v = stat[WT_CO + c];
  const bool bad = stat[2 * WT_CO + c] != 0.;
  const float ga = gamma[c];
  const float* f = pf + (size_t)b * tiles * (WT_PF * WT_CO) + c;
  const int* ip = pi + (size_t)b * tiles * (WT_PI * WT_CO) + c;
  float ys = f[4 * WT_CO];   // point 0
  int as = 0;
  if (ga != 0.f) {
    const int vo = ga > 0.f ? 2 * WT_CO : 3 * WT_CO, io = ga > 0.f ? 0 : WT_CO;
    ys = f[vo];
    as = ip[io];
    for (int t = 1; t < tiles; ++t) {
      const float yt = f[(size_t)t * (WT_PF * WT_CO) + vo];
      const bool take = ga > 0.f ? yt > ys : yt < ys;   // strict: an equal value keeps the earlier tile's lower point
      as = take ? ip[(size_t)t * (WT_PI * WT_CO) + io] : as;
      ys = take ? yt : ys;
    }
  }
  const double xh = (((double)ys - (double)shift[c]) - dm) / __builtin_sqrt(v + (double)eps);
  float o = (float)((double)ga * xh + (double)beta[c]);
  if (relu) o = fmaxf(o, 0.f);
  const float nan = __builtin_nanf("");
  const size_t e = (size_t)b * WT_CO + c;
  out[e] = bad ? nan : o;
  arg[e] = as;
  xhat[e] = bad ? nan : (float)xh;
  if (b == 0) {
    mean[c] = bad ? nan : (float)((double)shift[c] + dm);
    var[c] = bad ? nan : (float)v;
  }
}

// dWg[c][k] = sum_b coef[b][c] U[b][k][arg[b][c]]: one workgroup per channel, one thread per k = tap*128 + ci, b ascending
__global__ void wt_gather_kernel(const float* __restrict__ X, const float* __restrict__ coef, const int* __restrict__ arg,
                                 int B, int N, int taps, float* __restrict__ dW) {
  const int c = blockIdx.x, k = threadIdx.x, tap = k >> 7, ci = k & 127;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float g = coef[(size_t)b * WT_CO + c];
    const int p = arg[(size_t)b * WT_CO + c] + tap - taps / 2;
    if (g != 0.f && p >= 0 && p < N) acc = __builtin_fmaf(g, X[((size_t)b * WT_CI + ci) * N + p], acc);
  }
  dW[(size_t)c * (taps * 128) + k] = acc;
}

// dX[b][ci][q]: one workgroup per (64-column tile, instance), thread = input channel; the tile's sums live in LDS, each row
// owned by one thread, and take their terms in (channel, tap) ascending order
__global__ __launch_bounds__(WT_CI) void wt_scatter_kernel(const float* __restrict__ W, const float* __restrict__ coef,
                                                           const int* __restrict__ arg, int N, int taps,
                                                           float* __restrict__ dX) {
  __shared__ float s_acc[WT_CI * 65];
  __shared__ float s_g[WT_CO];
  __shared__ int s_a[WT_CO];
  const int ci = threadIdx.x, b = blockIdx.y, q0 = blockIdx.x * 64;
  for (int c = ci; c < WT_CO; c += WT_CI) {
    s_g[c] = coef[(size_t)b * WT_CO + c];
    s_a[c] = arg[(size_t)b * WT_CO + c];
  }
  for (int j = 0; j < 64; ++j) s_acc[ci * 65 + j] = 0.f;
  __syncthreads();
  for (int c = 0; c < WT_CO; ++c) {
    const float g = s_g[c];
    const int rel = s_a[c] - taps / 2 - q0;   // column of tap 0 inside the tile
    if (g == 0.f || rel + taps <= 0 || rel >= 64) continue;   // uniform over the workgroup
    for (int tap = 0; tap < taps; ++tap) {
      const int col = rel + tap;
      if (col < 0 || col >= 64 || q0 + col >= N) continue;
      s_acc[ci * 65 + col] = __builtin_fmaf(g, W[(size_t)c * (taps * 128) + tap * 128 + ci], s_acc[ci * 65 + col]);
    }
  }
  __syncthreads();
  float* dst = dX + ((size_t)b * WT_CI) * N;
  for (int e = ci; e < WT_CI * 64; e += WT_CI) {   // coalesced over the columns
    const int row = e >> 6, col = e & 63;
    if (q0 + col < N) dst[(size_t)row * N + q0 + col] = s_acc[row * 65 + col];
  }
}

inline size_t wt_align(size_t x) { return (x + 255) & ~(size_t)255; }
struct WtLayout {
  size_t wp, pf, pi, stat, total;
};
inline WtLayout wt_layout(int B, int N, int taps) {
  const size_t units = (size_t)B * ((N + WT_COLS - 1) / WT_COLS);
  WtLayout l;
  l.wp = 0;
  l.pf = wt_align((size_t)WT_CO * taps * 128 * sizeof(float));
  l.pi = l.pf + wt_align(units * WT_PF * WT_CO * sizeof(float));
  l.stat = l.pi + wt_align(units * WT_PI * WT_CO * sizeof(int));
  l.total = l.stat + wt_align((size_t)3 * WT_CO * sizeof(double));
  return l;
}
inline bool wt_sizes_ok(int B, int N, int taps) {
  return B >= 1 && N >= 1 && B <= 65535 && (taps == 1 || taps == 3) && (long long)B * N >= 2 && (long long)B * N < (1ll << 31) / WT_CI;
}

}  // namespace

extern "C" int64_t geoa3_wide_train_workspace_bytes(int B, int N, int taps) {
  if (!wt_sizes_ok(B, N, taps)) return GEOA3_EINVAL;
  return (int64_t)wt_layout(B, N, taps).total;
}

extern "C" int geoa3_wide_train_forward(const float* X, const float* W, const float* shift, const float* gamma,
                                        const float* beta, float eps, int relu, int B, int N, int taps, float* out,
                                        int32_t* arg, float* xhat, float* mean, float* var, void* workspace, void* stream) {
  if (!X || !W || !shift || !gamma || !beta || !out || !arg || !xhat || !mean || !var || !workspace) return GEOA3_EINVAL;
  if (!wt_sizes_ok(B, N, taps)) return GEOA3_EINVAL;   // (B N < 2: BatchNorm has no variance to normalise by)
  hipStream_t s = geoa3_stream(stream);
  const WtLayout l = wt_layout(B, N, taps);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  float4* Wp = reinterpret_cast<float4*>(ws + l.wp);
  float* pf = reinterpret_cast<float*>(ws + l.pf);
  int* pi = reinterpret_cast<int*>(ws + l.pi);
  double* stat = reinterpret_cast<double*>(ws + l.stat);
  const int tiles = (N + WT_COLS - 1) / WT_COLS;
  hipLaunchKernelGGL(wt_pack_kernel, dim3((WT_CO * taps * 32 + 255) / 256), dim3(256), 0, s, W, Wp, taps);
  const size_t lds = (size_t)WT_CI * WT_XP * sizeof(float);
  if (taps == 1) hipLaunchKernelGGL(wt_fwd_kernel<1>, dim3(tiles, B), dim3(WT_THREADS), lds, s, X, Wp, shift, N, pf, pi);
  else hipLaunchKernelGGL(wt_fwd_kernel<3>, dim3(tiles, B), dim3(WT_THREADS), lds, s, X, Wp, shift, N, pf, pi);
  hipLaunchKernelGGL(wt_stats_kernel, dim3(WT_CO / 64), dim3(1024), 0, s, pf, B * tiles, (double)B * (double)N, stat);
  hipLaunchKernelGGL(wt_select_kernel, dim3(WT_CO / 256, B), dim3(256), 0, s, pf, pi, stat, shift, gamma, beta, eps, relu,
                     tiles, out, arg, xhat, mean, var);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_wide_train_gather(const float* X, const float* coef, const int32_t* arg, int B, int N, int taps,
                                       float* dW, void* stream) {
  if (!X || !coef || !arg || !dW || !wt_sizes_ok(B, N, taps)) return GEOA3_EINVAL;
  hipLaunchKernelGGL(wt_gather_kernel, dim3(WT_CO), dim3(taps * 128), 0, geoa3_stream(stream), X, coef, arg, B, N, taps, dW);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_wide_train_scatter(const float* W, const float* coef, const int32_t* arg, int B, int N, int taps,
                                        float* dX, void* stream) {
  if (!W || !coef || !arg || !dX || !wt_sizes_ok(B, N, taps)) return GEOA3_EINVAL;
  hipLaunchKernelGGL(wt_scatter_kernel, dim3((N + 63) / 64, B), dim3(WT_CI), 0, geoa3_stream(stream), W, coef, arg, N, taps, dX);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
