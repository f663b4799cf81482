// The fused geometric objective + gradient for clouds whose positions and 64-bit sums no longer fit ONE workgroup's LDS
// (gfx950): 5840 .. 8192 points through geoa3_geo_loss_grad, 64 .. 8192 through geoa3_debug_geo_wide.
// Reference: Lib/loss_utils.py:25-97 as combined by Attacker/geoA3_attack.py:131-166 (see geom_loss.hip).
//
// geo_big_kernel (geom_loss.hip) keeps an instance's positions (12 N bytes) and three planes of 64-bit fixed-point sums
// (24 N bytes) in LDS: 144 KB at 4096 points, 288 KB at 8192.  Here the instance is split twice:
//   pass A  geo_wide_pair_kernel<G>, grid (chunks of GW_CHUNK centres, B): positions of the whole cloud in LDS (96 KB at
//           8192), one lane per (centre, neighbour) pair, geo_big_kernel's pair phase with the same expressions up to the
//           centre's coefficient dk.  Writes kappa_adv, one 16-byte record per point (normal of the nearest clean point, dk)
//           and the chunk's partial loss sums and Hausdorff (max, index).  The chunks are a function of N alone and every
//           partial is reduced in a fixed order, so the loss values depend on nothing but N.
//   pass B  geo_wide_sum_kernel<G>, grid (S, B): workgroup s OWNS the destinations r0 .. r0 + R - 1, R = ceil(N / S).  LDS:
//           positions of the whole cloud + the three 64-bit planes of its own range (R = 2048: 48 KB) + the coarse pool and
//           the NaN flags: 152 KB at 8192 points, S = 4.  It streams table and records once, forms every pair's term with
//           geo_pair_grad and adds what lands in its range -- the pull on q, the centre's own (negative, group-summed) term
//           -- through geo_fix_add; then the clean points' Chamfer pulls; then writes grad for its range.  Integer sums have
//           no order: the gradient does not depend on S, the batch, the workgroup ids or the run.  The loss values are the
//           chunks' partials added in chunk order.
// Every pair term is formed S times (once per range): the price of keeping the sums in LDS -- global 64-bit atomics run at
// ~50 G/s here, several ms per launch at 250 instances, and gathering pull records by destination was measured and
// dropped before (geom_loss.hip, above geo_big_kernel).
//
// The fixed-point range.  A term of the fine scale is at most 2^(Ex + 10 - h) at unit 2^(Ex - 40): 2^(50 - h) units.  A
// destination receives at most N + Nr terms that are not exactly zero: one from every OTHER row of the table that lists it
// (a K-NN row lists a point at most once; a point listed in its own row pulls with sign(0) = 0), its own centre term, and
// one from every clean point whose nearest adversarial point it is.  h = 0 up to 4096 points -- geo_big_kernel's scale and
// bits, 8192 terms x 2^50 as there -- and beyond, h = 1 + ceil(log2((N + Nr) / 16384)) with both limits one ulp BELOW the
// power of two: at most 2^(13 + h) terms of less than 2^(50 - h) units stay inside 63 bits, so a sum cannot wrap; what
// exceeds the fine limit goes to the coarse pool (limit and count scaled alike), what exceeds that raises the NaN flag.
#include "common.h"
#include "geom_internal.h"
#include "geom_loss_fix.h"

namespace {

constexpr int GW_T = 1024;
constexpr int GW_CHUNK = 1024;   // centres per workgroup of pass A
constexpr int GW_PART = 8;       // floats per chunk partial: sum d_ao (or L2), sum d_oa, sum e^2, Hausdorff max, its index
constexpr int GW_RED = 16 * 5 + 4;

__host__ __device__ inline int gw_chunks(int N) { return (N + GW_CHUNK - 1) / GW_CHUNK; }

// < normalize(v), n > of kappa_point(), with the multiply-adds spelled out as geo_big_kernel is COMPILED: there the length
// is shared with geo_pair_grad's (z^2 + (y^2 + x^2), fused) and the dot product is contracted as z + (x + y); left to
// -ffp-contract=fast this kernel, which has no geo_pair_grad beside it, fuses the length as z^2 + (x^2 + y^2) and kappa_adv
// differs in the last bit.
__device__ __forceinline__ float gw_kappa_term(float vx, float vy, float vz, float nx, float ny, float nz) {
#pragma clang fp contract(off)
  const float r = GEO_SQRT(__builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx)));
  const float inv = GEO_RCP(fmaxf(r, NORM_EPS));
  const float ux = vx * inv, uy = vy * inv, uz = vz * inv;
  return __builtin_fmaf(uz, nz, __builtin_fmaf(ux, nx, uy * ny));
}

template <int G>
__global__ __launch_bounds__(GW_T) void geo_wide_pair_kernel(geoa3_geo_args A, float4* __restrict__ rec,
                                                             float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int N = A.N, k = A.k, k1 = k + 1, ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Nr = A.Nr > 0 ? A.Nr : N;
  float* s_pos = sm;               // [N][3]
  float* s_red = s_pos + 3 * N;    // [GW_RED]
  const size_t bN = (size_t)b * N, bNr = (size_t)b * Nr;
  const float* adv = A.adv + bN * 3;
  const float* ori = A.ori + bNr * 3;
  const bool do_curv = (A.w_curv != 0.f || A.dkappa != nullptr) && A.knn_adv != nullptr;
  const bool do_cd = A.dis_type == 1, do_l2 = A.dis_type == 2;
  const bool two_side = do_cd && !A.single_side && A.d_oa != nullptr;
  const bool do_hd = A.w_hd != 0.f && A.d_ao != nullptr;
  for (int i = tid; i < N; i += GW_T) {
    s_pos[3 * i] = adv[i];
    s_pos[3 * i + 1] = adv[N + i];
    s_pos[3 * i + 2] = adv[2 * N + i];
  }
  __syncthreads();
  const int lo = ch * GW_CHUNK, hi = min(N, lo + GW_CHUNK);
  const float invN = 1.0f / (float)N;
  // ---- pairs: lane = (centre c, neighbour m); kappa_adv[c] and the centre's coefficient by a G-lane butterfly
  // (geo_big_kernel's pair phase, same expressions)
  float sum_e2 = 0.f;
  if (do_curv) {
    constexpr int CPP = GW_T / G, U = 4;
    const int32_t* tab = A.knn_adv + bN * (size_t)k1;
    const float* Nm = A.normal_ori + bNr * 3;
    const int m = tid % G, cl = tid / G;
    const bool lane_on = m < k;
    for (int c0 = lo; c0 < hi; c0 += CPP * U) {
      int q[U], nn[U];
      float4 cv[U];
      float dkp[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u * CPP + cl;
        const int cc = c < hi ? c : hi - 1;
        q[u] = (c < hi && lane_on) ? tab[(size_t)c * k1 + 1 + m] : cc;
        bool nn_oob;   // (geo_tab_idx: an entry of i_ao outside [0, Nr) is not followed, its normal is NaN: nn = -1 - index)
        nn[u] = geo_tab_idx(A.i_ao[bN + cc], Nr, 0, nn_oob);
        nn[u] = nn_oob ? -1 : nn[u];
        dkp[u] = A.dkappa ? A.dkappa[bN + cc] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
      {
        const int ni = nn[u] < 0 ? 0 : nn[u];
        cv[u] = make_float4(nn[u] < 0 ? __builtin_nanf("") : Nm[ni], Nm[Nr + ni], Nm[2 * Nr + ni], A.kappa_ori ? A.kappa_ori[bNr + ni] : 0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u * CPP + cl;
        const bool cvalid = c < hi, active = cvalid && lane_on;
        const int cc = cvalid ? c : hi - 1;
        const float cx = s_pos[3 * cc], cy = s_pos[3 * cc + 1], cz = s_pos[3 * cc + 2];
        bool oob;   // (geom_loss_fix.h: an entry outside the cloud is not followed, the pair's term is NaN)
        q[u] = geo_tab_idx(q[u], N, cc, oob);
        const float qx = oob ? __builtin_nanf("") : s_pos[3 * q[u]], qy = s_pos[3 * q[u] + 1], qz = s_pos[3 * q[u] + 2];
        const float4 nv = cv[u];
        const float t = gw_kappa_term(qx - cx, qy - cy, qz - cz, nv.x, nv.y, nv.z);
        const float kap = group_sum<G>(active ? fabsf(t) : 0.f) / (float)k;
        const float e = kap - nv.w;
        const float dk = (A.dkappa ? dkp[u] : A.w_curv * invN * 2.0f * e) / (float)k;
        if (m == 0 && cvalid) {
          sum_e2 += e * e;
          if (A.kappa_adv) A.kappa_adv[bN + c] = kap;
          rec[bN + c] = make_float4(nv.x, nv.y, nv.z, dk);
        }
      }
    }
  }
  // ---- the chunk's share of the loss sums and of the Hausdorff arg-max, fixed order
  float sum_ao = 0.f, sum_oa = 0.f;
  MaxIdx hd{-__builtin_inff(), 0x7fffffff};
  for (int i = lo + tid; i < hi; i += GW_T) {
    if (do_cd || do_hd) {
      const float d = A.d_ao[bN + i];
      if (do_cd) sum_ao += d;
      if (do_hd) hd = better(hd, MaxIdx{d, i});
    }
    if (do_l2) {
      const float dx = s_pos[3 * i] - ori[i], dy = s_pos[3 * i + 1] - ori[Nr + i], dz = s_pos[3 * i + 2] - ori[2 * Nr + i];
      sum_ao += dx * dx + dy * dy + dz * dz;
    }
  }
  if (two_side) {   // the clean points in as many chunks as the adversarial ones
    const int per = (Nr + (int)gridDim.x - 1) / (int)gridDim.x, rlo = ch * per, rhi = min(Nr, rlo + per);
    for (int i = rlo + tid; i < rhi; i += GW_T)   // (an entry of i_oa outside [0, N) names no point: its term is NaN)
      sum_oa += (A.i_oa && (unsigned)A.i_oa[bNr + i] >= (unsigned)N) ? __builtin_nanf("") : A.d_oa[bNr + i];
  }
  sum_ao = wave_sum(sum_ao);
  sum_oa = wave_sum(sum_oa);
  sum_e2 = wave_sum(sum_e2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MaxIdx other{__shfl_xor(hd.v, o, 64), __shfl_xor(hd.i, o, 64)};
    hd = better(hd, other);
  }
  if (lane == 0) {
    s_red[wave * 5 + 0] = sum_ao;
    s_red[wave * 5 + 1] = sum_oa;
    s_red[wave * 5 + 2] = sum_e2;
    s_red[wave * 5 + 3] = hd.v;
    s_red[wave * 5 + 4] = __int_as_float(hd.i);
  }
  __syncthreads();
  if (tid == 0) {
    float a = 0.f, o = 0.f, e2 = 0.f;
    MaxIdx h{-__builtin_inff(), 0x7fffffff};
    for (int w = 0; w < GW_T / 64; ++w) {
      a += s_red[w * 5 + 0];
      o += s_red[w * 5 + 1];
      e2 += s_red[w * 5 + 2];
      h = better(h, MaxIdx{s_red[w * 5 + 3], __float_as_int(s_red[w * 5 + 4])});
    }
    float* P = part + ((size_t)b * gridDim.x + ch) * GW_PART;
    P[0] = a;
    P[1] = o;
    P[2] = e2;
    P[3] = h.v;
    P[4] = __int_as_float(h.i);
  }
}

template <int G>
__global__ __launch_bounds__(GW_T) void geo_wide_sum_kernel(geoa3_geo_args A, const float4* __restrict__ rec,
                                                            const float* __restrict__ part, int R, int NC, int narrow) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int N = A.N, k = A.k, k1 = k + 1, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Nr = A.Nr > 0 ? A.Nr : N;
  const int r0 = blockIdx.x * R, Rn = min(R, N - r0);   // this workgroup's destinations: r0 .. r0 + Rn - 1 (Rn >= 1: the launcher)
  unsigned long long* s_acc = reinterpret_cast<unsigned long long*>(sm);   // [3][R] fixed-point sums: own curvature term + pulls
  float* s_pos = reinterpret_cast<float*>(s_acc + 3 * R);                  // [N][3]
  float* s_red = s_pos + 3 * N;                                            // [GW_RED]
  GeoPool pool;                                                            // destinations with coarse-scale terms
  pool.cap = GB_POOL_CAP;
  pool.acc = reinterpret_cast<unsigned long long*>((reinterpret_cast<uintptr_t>(s_red + GW_RED) + 7) & ~(uintptr_t)7);
  pool.key = reinterpret_cast<int*>(pool.acc + GB_POOL_CAP * 3);
  unsigned* s_bad = reinterpret_cast<unsigned*>(pool.key + GB_POOL_CAP);   // [ceil(R / 32)] sticky "not representable"
  const size_t bN = (size_t)b * N, bNr = (size_t)b * Nr;
  const float* adv = A.adv + bN * 3;
  const float* ori = A.ori + bNr * 3;
  const bool do_curv = (A.w_curv != 0.f || A.dkappa != nullptr) && A.knn_adv != nullptr;
  const bool do_cd = A.dis_type == 1, do_l2 = A.dis_type == 2;
  const bool two_side = do_cd && !A.single_side && A.d_oa != nullptr;
  const bool do_hd = A.w_hd != 0.f && A.d_ao != nullptr;
  const bool want_grad = A.grad != nullptr;
  const float invN = 1.0f / (float)N;
  // ---- the loss values: the chunks' partials in chunk order (every thread forms the arg-max; one thread writes)
  MaxIdx hd{-__builtin_inff(), 0x7fffffff};
  {
    const float* P = part + (size_t)b * NC * GW_PART;
    float a = 0.f, o = 0.f, e2 = 0.f;
    for (int c = 0; c < NC; ++c) {
      a += P[c * GW_PART + 0];
      o += P[c * GW_PART + 1];
      e2 += P[c * GW_PART + 2];
      hd = better(hd, MaxIdx{P[c * GW_PART + 3], __float_as_int(P[c * GW_PART + 4])});
    }
    if (tid == 0 && blockIdx.x == 0) {
      float dis = 0.f;
      if (do_cd) dis = a * invN + (two_side ? o * (1.0f / (float)Nr) : 0.f);
      if (do_l2) dis = a;
      const float hdv = do_hd ? hd.v : 0.f;
      const float curv = do_curv ? e2 * invN : 0.f;
      float con = 0.f;
      if (A.dis_type != 0) con = A.w_dis * dis;
      if (do_hd) con = con + A.w_hd * hdv;
      if (do_curv) con = con + A.w_curv * curv;
      if (A.dis_loss) A.dis_loss[b] = dis;
      if (A.hd_loss) A.hd_loss[b] = hdv;
      if (A.curv_loss) A.curv_loss[b] = curv;
      if (A.constrain) A.constrain[b] = con;
    }
  }
  const int hd_arg = hd.i;
  if (!want_grad) return;
  for (int i = tid; i < N; i += GW_T) {
    s_pos[3 * i] = adv[i];
    s_pos[3 * i + 1] = adv[N + i];
    s_pos[3 * i + 2] = adv[2 * N + i];
  }
  for (int i = tid; i < 3 * R; i += GW_T) s_acc[i] = 0ull;
  for (int i = tid; i < GB_POOL_CAP * 3; i += GW_T) pool.acc[i] = 0ull;
  for (int i = tid; i < GB_POOL_CAP; i += GW_T) pool.key[i] = -1;
  for (int i = tid; i < (R + 31) / 32; i += GW_T) s_bad[i] = 0u;
  float xmax = 0.f;
  if (A.dkappa && do_curv) {                       // (dkappa mode only: the INSTANCE's largest |dkappa|: a maximum has no order)
    for (int i = tid; i < N; i += GW_T) xmax = fmaxf(xmax, fabsf(A.dkappa[bN + i]));
    xmax = wave_max(xmax);
    if (lane == 0) s_red[wave] = xmax;
  }
  __syncthreads();
  if (A.dkappa && do_curv) {
    xmax = 0.f;
#pragma unroll
    for (int w = 0; w < GW_T / 64; ++w) xmax = fmaxf(xmax, s_red[w]);
  }
  GeoFix FX = geo_fix_make(geo_coef_bound(A, N, Nr, xmax));
  if (narrow) {   // (header comment: more than 8192 terms per destination)
    FX.lim_f = __uint_as_float(__float_as_uint(FX.lim_f * geo_pow2(-narrow)) - 1u);
    FX.lim_c = __uint_as_float(__float_as_uint(FX.lim_c * geo_pow2(-narrow)) - 1u);
  }
  // ---- pairs: lane = (centre c, neighbour m), the whole table.  The pair's term goes to q's sums if q is ours, its
  // negative, summed over m, to c's if c is ours (geo_big_kernel's pair phase, same expressions, dk from pass A)
  if (do_curv) {
    constexpr int CPP = GW_T / G, U = 4;
    const int32_t* tab = A.knn_adv + bN * (size_t)k1;
    const int m = tid % G, cl = tid / G;
    const bool lane_on = m < k;
    for (int c0 = 0; c0 < N; c0 += CPP * U) {
      int q[U];
      float4 cv[U];
      float csx[U], csy[U], csz[U];   // the group sums of the U centres' pair terms (the same in every lane of a group)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u * CPP + cl;
        const int cc = c < N ? c : N - 1;
        q[u] = (c < N && lane_on) ? tab[(size_t)c * k1 + 1 + m] : cc;
        cv[u] = rec[bN + cc];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u * CPP + cl;
        const bool cvalid = c < N, active = cvalid && lane_on;
        const int cc = cvalid ? c : N - 1;
        const float cx = s_pos[3 * cc], cy = s_pos[3 * cc + 1], cz = s_pos[3 * cc + 2];
        bool oob;
        q[u] = geo_tab_idx(q[u], N, cc, oob);
        const float qx = oob ? __builtin_nanf("") : s_pos[3 * q[u]], qy = s_pos[3 * q[u] + 1], qz = s_pos[3 * q[u] + 2];
        const float4 nv = cv[u];
        float dvx, dvy, dvz, t2;
        geo_pair_grad(cx, cy, cz, nv.x, nv.y, nv.z, nv.w, qx, qy, qz, dvx, dvy, dvz, t2);
        const float sx = group_sum<G>(active ? dvx : 0.f), sy = group_sum<G>(active ? dvy : 0.f),
                    sz = group_sum<G>(active ? dvz : 0.f);
        const int ql = q[u] - r0;
        if (active && !oob && (unsigned)ql < (unsigned)Rn) geo_fix_add<3>(FX, s_acc, R, pool, s_bad, ql, dvx, dvy, dvz);
        csx[u] = sx;
        csy[u] = sy;
        csz[u] = sz;
      }
      // the centres' own terms: lane m < U of a group takes centre m of the U just done (as geo_big_kernel)
      if (m < U) {
        const int c = c0 + m * CPP + cl, cl2 = c - r0;
        if ((unsigned)cl2 < (unsigned)Rn) {
          float sx = csx[0], sy = csy[0], sz = csz[0];
#pragma unroll
          for (int u = 1; u < U; ++u) {
            sx = m == u ? csx[u] : sx;
            sy = m == u ? csy[u] : sy;
            sz = m == u ? csz[u] : sz;
          }
          geo_fix_add<3>(FX, s_acc, R, pool, s_bad, cl2, -sx, -sy, -sz);
        }
      }
    }
  }
  const float c_cd = A.w_dis * invN * 2.0f;
  const float cr = (Nr != N) ? A.w_dis * (1.0f / (float)Nr) * 2.0f : c_cd;
  if (two_side)          // clean point j pulls on its nearest adversarial point
    for (int j = tid; j < Nr; j += GW_T) {
      const int q = A.i_oa[bNr + j], ql = q - r0;
      if ((unsigned)ql < (unsigned)Rn)
        geo_fix_add<3>(FX, s_acc, R, pool, s_bad, ql, cr * (s_pos[3 * q] - ori[j]), cr * (s_pos[3 * q + 1] - ori[Nr + j]),
                       cr * (s_pos[3 * q + 2] - ori[2 * Nr + j]));
    }
  __syncthreads();       // every pull of this range is in the sums
  // ---- every point of the range: its Chamfer / Hausdorff / L2 terms, then its fixed-point sums (own curvature term + pulls)
  float* Gd = A.grad + bN * 3;
  for (int il = tid; il < Rn; il += GW_T) {
    const int i = r0 + il;
    const float px = s_pos[3 * i], py = s_pos[3 * i + 1], pz = s_pos[3 * i + 2];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (do_cd || do_hd) {
      bool nn_oob;
      const int nn = geo_tab_idx(A.i_ao[bN + i], Nr, 0, nn_oob);
      const float dx = px - (nn_oob ? __builtin_nanf("") : ori[nn]), dy = py - (nn_oob ? __builtin_nanf("") : ori[Nr + nn]),
                    dz = pz - (nn_oob ? __builtin_nanf("") : ori[2 * Nr + nn]);
      float c = do_cd ? c_cd : 0.f;
      if (do_hd && i == hd_arg) c += A.w_hd * 2.0f;
      gx += c * dx;
      gy += c * dy;
      gz += c * dz;
    }
    if (do_l2) {
      const float c = A.w_dis * 2.0f;
      gx += c * (px - ori[i]);
      gy += c * (py - ori[Nr + i]);
      gz += c * (pz - ori[2 * Nr + i]);
    }
    float ax = __ll2float_rn((long long)s_acc[il]) * FX.from_f, ay = __ll2float_rn((long long)s_acc[R + il]) * FX.from_f,
          az = __ll2float_rn((long long)s_acc[2 * R + il]) * FX.from_f;
    const int sl = geo_pool_find(pool, il, false);
    if (sl >= 0) {
      ax += __ll2float_rn((long long)pool.acc[sl * 3 + 0]) * FX.from_c;
      ay += __ll2float_rn((long long)pool.acc[sl * 3 + 1]) * FX.from_c;
      az += __ll2float_rn((long long)pool.acc[sl * 3 + 2]) * FX.from_c;
    }
    gx += ax;
    gy += ay;
    gz += az;
    if ((s_bad[il >> 5] >> (il & 31)) & 1u) gx = gy = gz = __builtin_nanf("");   // a term beyond the coarse limit, a NaN, or a full pool
    Gd[i] = gx;
    Gd[N + i] = gy;
    Gd[2 * N + i] = gz;
  }
}

size_t gw_sum_lds(int N, int R) {
  return (size_t)24 * R + (size_t)12 * N + GW_RED * sizeof(float) + 8 + GB_POOL_CAP * (3 * 8 + 4) + ((size_t)(R + 31) / 32) * 4;
}
constexpr size_t GW_LDS_MAX = 160 * 1024;

}  // namespace

size_t geo_wide_scratch_bytes(int B, int N) {   // the records, then the chunks' partials
  return (size_t)16 * B * N + (size_t)B * gw_chunks(N) * GW_PART * sizeof(float);
}

int geo_wide_ranges(int N) {
  for (int S = 1; S <= 16; S *= 2)
    if (gw_sum_lds(N, (N + S - 1) / S) <= GW_LDS_MAX) return S;
  return 0;
}

int geo_wide_launch(const geoa3_geo_args* a, int ranges, hipStream_t s) {
  const int N = a->N, Nr = a->Nr > 0 ? a->Nr : a->N;
  const bool do_curv = (a->w_curv != 0.f || a->dkappa) && a->knn_adv;
  if (N < 64 || N > GEO_WIDE_MAX_N || !a->scratch || (do_curv && a->k > 64) || ranges < 0 || ranges > 16) return GEOA3_ENOSUPPORT;
  const int S = ranges > 0 ? ranges : geo_wide_ranges(N);
  if (S <= 0) return GEOA3_ENOSUPPORT;
  const int R = (N + S - 1) / S;
  const size_t ldsB = gw_sum_lds(N, R), ldsA = ((size_t)3 * N + GW_RED) * sizeof(float);
  if (ldsB > GW_LDS_MAX || (size_t)(S - 1) * R >= (size_t)N) return GEOA3_ENOSUPPORT;   // (every range holds a point)
  int narrow = 0;   // header comment: the fixed-point limits beyond 4096 points
  if (N > 4096) {
    narrow = 1;
    for (int64_t cap = 16384; cap < (int64_t)N + Nr; cap *= 2) ++narrow;
  }
  const int NC = gw_chunks(N);
  float4* rec = reinterpret_cast<float4*>(a->scratch);
  float* part = reinterpret_cast<float*>(rec + (size_t)a->B * N);
  int G = 16;
  while (G < a->k && do_curv) G *= 2;
#define GEOA3_WIDE_CASE(GG)                                                                                            \
  if (G == GG) {                                                                                                       \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(geo_wide_pair_kernel<GG>),                                 \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsA);                                  \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(geo_wide_sum_kernel<GG>),                                  \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB);                                  \
    hipLaunchKernelGGL(geo_wide_pair_kernel<GG>, dim3(NC, a->B), dim3(GW_T), ldsA, s, *a, rec, part);                  \
    hipLaunchKernelGGL(geo_wide_sum_kernel<GG>, dim3(S, a->B), dim3(GW_T), ldsB, s, *a, rec, part, R, NC, narrow);     \
  }
  GEOA3_WIDE_CASE(16)
  GEOA3_WIDE_CASE(32)
  GEOA3_WIDE_CASE(64)
#undef GEOA3_WIDE_CASE
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int64_t geoa3_debug_geo_wide_scratch_bytes(int B, int N) {
  return B > 0 && N > 0 ? (int64_t)geo_wide_scratch_bytes(B, N) : 0;
}

extern "C" int geoa3_debug_geo_wide(const geoa3_geo_args* a, int ranges, void* stream) {
  // the argument checks of geoa3_geo_loss_grad
  if (!a || !a->adv || !a->ori || a->B <= 0 || a->N <= 0 || a->Nr < 0) return GEOA3_EINVAL;
  if (a->dis_type == 2 && a->Nr > 0 && a->Nr != a->N) return GEOA3_EINVAL;
  if (a->dis_type == 1 && (!a->d_ao || !a->i_ao)) return GEOA3_EINVAL;
  if (a->w_hd != 0.f && (!a->d_ao || !a->i_ao)) return GEOA3_EINVAL;
  if ((a->w_curv != 0.f || a->dkappa) && (!a->knn_adv || !a->normal_ori || !a->i_ao || a->k <= 0)) return GEOA3_EINVAL;
  if (a->w_curv != 0.f && !a->dkappa && !a->kappa_ori) return GEOA3_EINVAL;
  if (a->dis_type == 1 && !a->single_side && a->d_oa && !a->i_oa) return GEOA3_EINVAL;
  return geo_wide_launch(a, ranges, geoa3_stream(stream));
}
