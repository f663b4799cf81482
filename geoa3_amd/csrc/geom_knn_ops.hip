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
// The scatter is the scheme of three_interpolate_grad (pointnet2_interp.hip), restated for int64 indices, any segment
// length and flat launches (no limit on B from the grid's y dimension).  The E = L K entries of an instance are sorted by
// destination -- a counting sort into the caller's scratch -- then one thread per (destination, group of components)
// walks its list:
//   scratch (int32): start [B][M+1] | cursor [B][M] | bucket [B][E] | order [B][E]
//   1. kso_count:  start[b][j] = number of entries that point at j (integer atomics: a count has no order)
//   2. kso_scan:   start <- its exclusive prefix sum (one workgroup per instance), cursor <- start
//   3. kso_place:  every entry takes the next free place of its destination's segment of `bucket` (integer atomic cursor:
//                  the ORDER inside a segment depends on timing ...)
//   4. kso_sort:   ... so every segment is sorted by e into `order` (the entries are distinct: the result is unique) by
//                  rank counting -- the rank of an entry is the number of smaller ones in its segment.  Up to 64 entries: one
//                  wavefront, lane shuffles.  Longer (a hub can receive all E entries): the whole workgroup, the segment
//                  passing through LDS in tiles of KSO_TILE entries while every thread counts for KSO_KPT entries of its
//                  own; any length, quadratic in it.
//   5. the sums (kgg_sum / kpg_g2) in list order; an empty list writes +0.0.  Every element is written.
// Two forms of the same five steps, the same bits: when an instance's tables fit the LDS of one compute unit
// (2 M + 2 E + E / 65 + 2 ints <= KSL_LDS_MAX bytes: every shape of the reference's objective, e.g. M = 1024, E = 1024 x 17)
// ONE workgroup per instance keeps them there and does all five steps in one launch (ksl_*: LDS atomics place the entries,
// `scratch` is not touched); larger instances take the five launches through `scratch` (kso_*).
// An index outside [0, M) is the caller's error: it is neither wrapped nor clamped nor dereferenced -- the gather writes NaN
// to that element, the backward passes drop the term (the entry is in no list).
// No float atomics; a NaN or inf term is added like any other value.
#include <climits>
#include "common.h"

namespace {

constexpr int KSO_TILE = 1024;   // entries of a long segment per LDS tile
constexpr int KSO_KPT = 4;       // entries a thread ranks per pass over a long segment (256 threads: 1024 per pass)
constexpr int KGG_CG = 4;        // components per thread of kgg_sum
constexpr int MAX_GRID_Y = 65535;

__device__ __forceinline__ bool kso_valid(int64_t j, int M) { return (uint64_t)j < (uint64_t)M; }

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
    out[f] = kso_valid(j, M) ? x[((size_t)b * M + (size_t)j) * U + c] : __builtin_nanf("");
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
  if (kso_valid(j, M)) {
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
// the counting sort of the entries by destination.  t: flat entry number over the batch (B E < 2^31), d: flat destination
// number (B M < 2^31).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kso_count_kernel(const int64_t* __restrict__ idx, int E, int M, int BE,
                                                        int* __restrict__ start) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= BE) return;
  const int b = t / E;
  const int64_t j = idx[t];
  if (kso_valid(j, M)) atomicAdd(start + (size_t)b * (M + 1) + (int)j, 1);
}

__global__ __launch_bounds__(256) void kso_scan_kernel(int* __restrict__ start, int* __restrict__ cursor, int M) {
  __shared__ int s_w[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* S = start + (size_t)b * (M + 1);
  int* Cu = cursor + (size_t)b * M;
  int carry = 0;
  for (int i0 = 0; i0 < M; i0 += 256) {
    const int i = i0 + tid;
    const int v = i < M ? S[i] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    int base = carry, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) base += s_w[w];
      total += s_w[w];
    }
    if (i < M) {
      S[i] = base + x - v;
      Cu[i] = base + x - v;
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) S[M] = carry;
}

__global__ __launch_bounds__(256) void kso_place_kernel(const int64_t* __restrict__ idx, int E, int M, int BE,
                                                        int* __restrict__ cursor, int* __restrict__ bucket) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= BE) return;
  const int b = t / E, e = t - b * E;
  const int64_t j = idx[t];
  if (!kso_valid(j, M)) return;
  const int pos = atomicAdd(cursor + (size_t)b * M + (int)j, 1);   // < start[j + 1] <= E: the counts were taken from the same idx
  bucket[(size_t)b * E + pos] = e;
}

// One wavefront per destination (four per workgroup); the segments of more than 64 entries are then ranked by the whole
// workgroup, one after the other.  No thread leaves before the last barrier.
__global__ __launch_bounds__(256) void kso_sort_kernel(const int* __restrict__ start, const int* __restrict__ bucket,
                                                       int* __restrict__ order, int E, int M, int BM) {
  __shared__ int s_tile[KSO_TILE];
  __shared__ int s_len[4];
  __shared__ size_t s_off[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = blockIdx.x * 4 + wave;
  int L = 0;
  size_t off = 0;
  if (d < BM) {
    const int b = d / M, i = d - b * M;
    const int* S = start + (size_t)b * (M + 1);
    const int s0 = S[i];
    L = S[i + 1] - s0;
    off = (size_t)b * E + s0;
  }
  if (L > 0 && L <= 64) {
    const int key = lane < L ? bucket[off + lane] : INT_MAX;
    int r = 0;
    for (int k = 0; k < L; ++k) r += __shfl(key, k, 64) < key ? 1 : 0;
    if (lane < L) order[off + r] = key;
  }
  if (lane == 0) {
    s_len[wave] = L > 64 ? L : 0;
    s_off[wave] = off;
  }
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    const int Lw = s_len[w];   // (the same value in every thread: the loops and barriers below are uniform)
    if (Lw == 0) continue;
    const int* in = bucket + s_off[w];
    int* out = order + s_off[w];
    for (int q0 = 0; q0 < Lw; q0 += 256 * KSO_KPT) {
      int key[KSO_KPT], r[KSO_KPT];
#pragma unroll
      for (int u = 0; u < KSO_KPT; ++u) {
        const int q = q0 + u * 256 + tid;
        key[u] = q < Lw ? in[q] : INT_MIN;   // (nothing is smaller than INT_MIN: such a slot counts nothing and writes nothing)
        r[u] = 0;
      }
      for (int t0 = 0; t0 < Lw; t0 += KSO_TILE) {
        const int tn = min(KSO_TILE, Lw - t0);
        __syncthreads();
        for (int k = tid; k < tn; k += 256) s_tile[k] = in[t0 + k];
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < tn; ++k) {
          const int v = s_tile[k];   // the same address in every lane: a broadcast read
#pragma unroll
          for (int u = 0; u < KSO_KPT; ++u) r[u] += v < key[u] ? 1 : 0;
        }
      }
#pragma unroll
      for (int u = 0; u < KSO_KPT; ++u)
        if (q0 + u * 256 + tid < Lw) out[r[u]] = key[u];   // r < Lw: a rank among Lw distinct entries
    }
  }
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
    if (!kso_valid(j, N2)) continue;
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
// The same steps with the tables of ONE instance in LDS: one workgroup of KSL_T threads per instance.
//   LDS (int32): start [M+1] | cursor [M] | bucket [E] | order [E] | long [E / 65 + 1]
// `long` lists the destinations with more than 64 entries (at most E / 65 of them; the order of the list does not matter:
// every segment's result is unique); the workgroup ranks them one after the other, KSL_KPT entries per thread and pass,
// reading the segment straight from LDS (the same address in every lane: broadcast reads).
// ------------------------------------------------------------------------------------------
constexpr int KSL_T = 1024;
constexpr int KSL_KPT = 4;
constexpr size_t KSL_LDS_MAX = 160 * 1024 - 1024;   // dynamic LDS (the static wave partials beside it)

size_t ksl_lds_bytes(int E, int M) { return sizeof(int) * ((size_t)(M + 1) + M + 2 * (size_t)E + E / 65 + 1); }

struct KslLists {
  const int* start;
  const int* order;
};

__device__ __forceinline__ KslLists ksl_build(const int64_t* __restrict__ I, int E, int M, int* sm) {
  __shared__ int s_w[KSL_T / 64];
  __shared__ int s_nlong;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* s_start = sm;
  int* s_cursor = s_start + (M + 1);
  int* s_bucket = s_cursor + M;
  int* s_order = s_bucket + E;
  int* s_long = s_order + E;
  for (int i = tid; i <= M; i += KSL_T) s_start[i] = 0;
  if (tid == 0) s_nlong = 0;
  __syncthreads();
  for (int e = tid; e < E; e += KSL_T) {
    const int64_t j = I[e];
    if (kso_valid(j, M)) atomicAdd(s_start + (int)j, 1);
  }
  __syncthreads();
  int carry = 0;
  for (int i0 = 0; i0 < M; i0 += KSL_T) {
    const int i = i0 + tid;
    const int v = i < M ? s_start[i] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    int base = carry, total = 0;
#pragma unroll
    for (int w = 0; w < KSL_T / 64; ++w) {
      if (w < wave) base += s_w[w];
      total += s_w[w];
    }
    if (i < M) {
      s_start[i] = base + x - v;
      s_cursor[i] = base + x - v;
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) s_start[M] = carry;
  __syncthreads();
  for (int e = tid; e < E; e += KSL_T) {
    const int64_t j = I[e];
    if (!kso_valid(j, M)) continue;
    const int pos = atomicAdd(s_cursor + (int)j, 1);   // < start[j + 1] <= E: the counts were taken from the same idx
    s_bucket[pos] = e;
  }
  __syncthreads();
  for (int i = wave; i < M; i += KSL_T / 64) {
    const int s0 = s_start[i], L = s_start[i + 1] - s0;
    if (L <= 0) continue;
    if (L <= 64) {
      const int key = lane < L ? s_bucket[s0 + lane] : INT_MAX;
      int r = 0;
      for (int k = 0; k < L; ++k) r += s_bucket[s0 + k] < key ? 1 : 0;
      if (lane < L) s_order[s0 + r] = key;
    } else if (lane == 0) {
      s_long[atomicAdd(&s_nlong, 1)] = i;   // at most E / 65 segments hold more than 64 of the E entries
    }
  }
  __syncthreads();
  const int nlong = s_nlong;
  for (int q = 0; q < nlong; ++q) {
    const int i = s_long[q];
    const int s0 = s_start[i], L = s_start[i + 1] - s0;
    for (int p0 = 0; p0 < L; p0 += KSL_T * KSL_KPT) {
      int key[KSL_KPT], r[KSL_KPT];
#pragma unroll
      for (int u = 0; u < KSL_KPT; ++u) {
        const int p = p0 + u * KSL_T + tid;
        key[u] = p < L ? s_bucket[s0 + p] : INT_MIN;   // (nothing is smaller than INT_MIN: counts nothing, writes nothing)
        r[u] = 0;
      }
      for (int k = 0; k < L; ++k) {
        const int v = s_bucket[s0 + k];
#pragma unroll
        for (int u = 0; u < KSL_KPT; ++u) r[u] += v < key[u] ? 1 : 0;
      }
#pragma unroll
      for (int u = 0; u < KSL_KPT; ++u)
        if (p0 + u * KSL_T + tid < L) s_order[s0 + r[u]] = key[u];   // r < L: a rank among L distinct entries
    }
  }
  __syncthreads();
  return KslLists{s_start, s_order};
}

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

// steps 1-4: `scratch` <- the lists of the B x M destinations
int kso_build(const int64_t* idx, int B, int E, int M, void* scratch, hipStream_t s, int** start_out, int** order_out) {
  const int BE = B * E, BM = B * M;
  int* start = static_cast<int*>(scratch);
  int* cursor = start + (size_t)B * (M + 1);
  int* bucket = cursor + (size_t)B * M;
  int* order = bucket + (size_t)B * E;
  if (hipMemsetAsync(start, 0, (size_t)B * (M + 1) * sizeof(int), s) != hipSuccess) return GEOA3_ELAUNCH;
  hipLaunchKernelGGL(kso_count_kernel, dim3((BE + 255) / 256), dim3(256), 0, s, idx, E, M, BE, start);
  hipLaunchKernelGGL(kso_scan_kernel, dim3(B), dim3(256), 0, s, start, cursor, M);
  hipLaunchKernelGGL(kso_place_kernel, dim3((BE + 255) / 256), dim3(256), 0, s, idx, E, M, BE, cursor, bucket);
  hipLaunchKernelGGL(kso_sort_kernel, dim3((BM + 3) / 4), dim3(256), 0, s, start, bucket, order, E, M, BM);
  *start_out = start;
  *order_out = order;
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
  return (int64_t)sizeof(int) * B * ((int64_t)(M + 1) + M + 2 * (int64_t)E);
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
  int *start = nullptr, *order = nullptr;
  const int rb = kso_build(idx, B, E, M, scratch, s, &start, &order);
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
    int *start = nullptr, *order = nullptr;
    const int rb = kso_build(idx, B, E, N2, scratch, s, &start, &order);
    if (rb != GEOA3_OK) return rb;
    const int BN2 = B * N2;
    hipLaunchKernelGGL(kpg_g2_kernel, dim3((BN2 + 255) / 256), dim3(256), 0, s, p1, p2, gd, start, order, N1, N2, K, BN2, g2);
  }
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
