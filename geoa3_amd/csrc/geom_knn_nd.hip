// K nearest neighbours in D dimensions (gfx950): knn_points for feature spaces (1 <= D <= 128), in the operator's OWN layout --
// point-major float32 q [B,Nq,D], r [B,Nr,D] -- so a dynamic-graph network searches its activations without a transpose pass.
//
// The contract extends the pinned one of geoa3_knn ("Ties"):
//   dist(q, r) = acc_D,  acc_0 = +0.0,  acc_{d+1} = fl(acc_d + fl(fl(q_d - r_d)^2))   (sequential, no fused multiply-add)
//   results ascend by (distance, index); exactly equal distances go to the lower index
// so a plain float32 loop on the CPU reproduces dists and idx bit for bit.  A distance that is NaN (a non-finite coordinate)
// is ordered AND reported as +inf: every query still receives K distinct indices in [0, Nr).
//
// Exact VALU arithmetic, all pairs: one query per thread, its coordinates in registers, padded with zeros to the bucket DB of
// the template (fl(acc + fl(fl(0 - 0)^2)) == acc for every acc, NaN included: the padding changes no bit).  The reference
// cloud passes through LDS in tiles of KND_TILE_FLOATS / DB points, padded the same way; every lane reads the same point (a
// broadcast ds_read_b128, no bank conflict).  The K best are kept as geom_nn.hip keeps its own: every point at or under the
// query's radius tau is appended to the thread's list in LDS; when a list is full the lane keeps its K best and tightens tau
// to the K-th distance.  tau starts at +inf and K <= Nr, so a list never ends with fewer than K entries.
#include "common.h"

namespace {

constexpr int KND_BLOCK = 128;          // queries per workgroup
constexpr int KND_TILE_FLOATS = 8192;   // the reference tile: 32 KB = 1024 / 256 / 128 / 64 points for DB = 8 / 32 / 64 / 128

__device__ __forceinline__ bool knd_less(float da, int ia, float db, int ib) { return (da < db) || (da == db && ia < ib); }

// the lane's K lexicographically smallest (distance, index) among its cnt >= K candidates, sorted, to the front of its
// column; returns the K-th distance
__device__ __forceinline__ float knd_compact(uint16_t* ci /*[CAP][KND_BLOCK]*/, float* cd /*[CAP][KND_BLOCK]*/, int cnt, int K,
                                             int tid) {
  float kth = __builtin_inff();
  for (int p = 0; p < K; ++p) {
    float bd = cd[p * KND_BLOCK + tid];
    int bi = ci[p * KND_BLOCK + tid];
    int bs = p;
    for (int s = p + 1; s < cnt; ++s) {
      const float d = cd[s * KND_BLOCK + tid];
      const int i = ci[s * KND_BLOCK + tid];
      if (knd_less(d, i, bd, bi)) {
        bd = d;
        bi = i;
        bs = s;
      }
    }
    if (bs != p) {
      cd[bs * KND_BLOCK + tid] = cd[p * KND_BLOCK + tid];
      ci[bs * KND_BLOCK + tid] = ci[p * KND_BLOCK + tid];
      cd[p * KND_BLOCK + tid] = bd;
      ci[p * KND_BLOCK + tid] = (uint16_t)bi;
    }
    kth = bd;
  }
  return kth;
}

template <int DB, int CAP>
__global__ __launch_bounds__(KND_BLOCK) void knn_nd_kernel(const float* __restrict__ Q, const float* __restrict__ R, int Nq,
                                                           int Nr, int D, int K, float* __restrict__ dists,
                                                           int32_t* __restrict__ idx) {
#pragma clang fp contract(off)
  constexpr int TR = KND_TILE_FLOATS / DB;
  extern __shared__ __attribute__((aligned(16))) unsigned char knd_sm[];
  float* s_ref = reinterpret_cast<float*>(knd_sm);                                 // [TR][DB]
  float* s_cd = s_ref + KND_TILE_FLOATS;                                           // [CAP][KND_BLOCK]
  uint16_t* s_ci = reinterpret_cast<uint16_t*>(s_cd + (size_t)CAP * KND_BLOCK);    // [CAP][KND_BLOCK]

  const int b = blockIdx.y, tid = threadIdx.x;
  const int q = blockIdx.x * KND_BLOCK + tid;
  const bool live = q < Nq;
  const float* Qp = Q + ((size_t)b * Nq + (live ? q : Nq - 1)) * D;
  const float* Rb = R + (size_t)b * Nr * D;
  float qv[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) qv[d] = d < D ? Qp[d] : 0.f;

  float tau = live ? __builtin_inff() : -1.f;   // (padding lanes never collect)
  int cnt = 0;
  for (int r0 = 0; r0 < Nr; r0 += TR) {
    const int tn = min(TR, Nr - r0);
    __syncthreads();
    for (int f = tid; f < tn * DB; f += KND_BLOCK) {
      const int j = f / DB, d = f - j * DB;
      s_ref[f] = d < D ? Rb[(size_t)(r0 + j) * D + d] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < tn; ++j) {
      const float4* rp = reinterpret_cast<const float4*>(s_ref + j * DB);
      float acc = 0.f;
#pragma unroll
      for (int d4 = 0; d4 < DB / 4; ++d4) {
        const float4 rv = rp[d4];
        const float t0 = qv[4 * d4] - rv.x, t1 = qv[4 * d4 + 1] - rv.y, t2 = qv[4 * d4 + 2] - rv.z, t3 = qv[4 * d4 + 3] - rv.w;
        acc = acc + t0 * t0;
        acc = acc + t1 * t1;
        acc = acc + t2 * t2;
        acc = acc + t3 * t3;
      }
      const float dk = acc == acc ? acc : __builtin_inff();
      if (dk <= tau) {   // cnt < CAP here: a full list was compacted below
        s_cd[cnt * KND_BLOCK + tid] = dk;
        s_ci[cnt * KND_BLOCK + tid] = (uint16_t)(r0 + j);
        ++cnt;
      }
      if (__builtin_expect(__any(cnt >= CAP), 0)) {
        if (cnt >= K) {
          tau = knd_compact(s_ci, s_cd, cnt, K, tid);
          cnt = K;
        }
      }
    }
  }
  if (live) {   // cnt >= K (see the head of this file)
    knd_compact(s_ci, s_cd, cnt, K, tid);
    float* od = dists + ((size_t)b * Nq + q) * K;
    int32_t* oi = idx + ((size_t)b * Nq + q) * K;
    for (int m = 0; m < K; ++m) {
      od[m] = s_cd[m * KND_BLOCK + tid];
      oi[m] = (int32_t)s_ci[m * KND_BLOCK + tid];
    }
  }
}

template <int DB, int CAP>
void knd_launch(const float* q, const float* r, int B, int Nq, int Nr, int D, int K, float* dists, int32_t* idx, hipStream_t s) {
  const size_t lds = (size_t)KND_TILE_FLOATS * 4 + (size_t)CAP * KND_BLOCK * 6;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(knn_nd_kernel<DB, CAP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL((knn_nd_kernel<DB, CAP>), dim3((Nq + KND_BLOCK - 1) / KND_BLOCK, B), dim3(KND_BLOCK), lds, s, q, r, Nq, Nr,
                     D, K, dists, idx);
}

template <int DB>
void knd_launch_k(const float* q, const float* r, int B, int Nq, int Nr, int D, int K, float* dists, int32_t* idx, hipStream_t s) {
  if (K <= 20) knd_launch<DB, 40>(q, r, B, Nq, Nr, D, K, dists, idx, s);
  else if (K <= 40) knd_launch<DB, 72>(q, r, B, Nq, Nr, D, K, dists, idx, s);
  else knd_launch<DB, 96>(q, r, B, Nq, Nr, D, K, dists, idx, s);
}

}  // namespace

extern "C" int geoa3_knn_nd(const float* q, const float* r, int B, int Nq, int Nr, int D, int K, float* dists, int32_t* idx,
                            void* stream) {
  if (!q || !r || !dists || !idx || B <= 0 || Nq <= 0 || Nr <= 0 || D < 1 || K < 1 || K > Nr) return GEOA3_EINVAL;
  if (D > GEOA3_KNN_ND_MAX_D || K > GEOA3_KNN_MAX_K || Nq > 8192 || Nr > 8192 || B > 65535) return GEOA3_ENOSUPPORT;
  hipStream_t s = geoa3_stream(stream);
  if (D <= 8) knd_launch_k<8>(q, r, B, Nq, Nr, D, K, dists, idx, s);
  else if (D <= 32) knd_launch_k<32>(q, r, B, Nq, Nr, D, K, dists, idx, s);
  else if (D <= 64) knd_launch_k<64>(q, r, B, Nq, Nr, D, K, dists, idx, s);
  else knd_launch_k<128>(q, r, B, Nq, Nr, D, K, dists, idx, s);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
