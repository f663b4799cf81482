// Self K-NN with slab pruning (gfx950): the all-pairs kernel of geom_nn.hip, fed with a fraction of the pairs.
//
// A candidate p can only enter the K nearest of q if its distance is within q's radius tau (the K-th distance to last
// iteration's neighbours), and d(q,p) >= (q_a - p_a)^2 along ANY axis a.  So: per instance, bin the cloud along its
// longest bounding-box axis (counting sort into 512 bins, one workgroup, ~3 us), hand the queries out in that order
// (256 consecutive sorted positions per workgroup: a narrow slab), and let the workgroup scan only the CONTIGUOUS run
// of sorted points whose bins intersect [q_a - sqrt(tau), q_a + sqrt(tau)] for any of its queries.  The inner loop is
// the regular LDS-broadcast distance loop of the all-pairs kernel (no per-lane cell walks, no divergence), the lists,
// the compaction and the lexicographic (distance, index) selection are the same, and the bin function is monotone in
// the coordinate, so the result is BIT-IDENTICAL to the all-pairs search for any input; a query without a usable
// radius scans everything.
//
// This file holds that search (slab_bin_kernel, then ONE of knn_slab_kernel<40 / 72 / 96> -- (distance, index) lists -- or
// knn_slabp_kernel<32, false> / <56, true> -- position lists; the attack loop at 250 x 1024, K = 17 runs <32, false>) and the
// entry points of the self K-NN: knn_self_route picks between it, the cell-grid search of geom_knn_grid.hip and the
// all-pairs kernel.
#include <utility>
#include "geom_internal.h"
#include "geom_knn_self.h"
#include "profile.h"

namespace {

constexpr int SB_T = 1024;            // binning kernel: threads
constexpr int SB_NB = 512;            // bins
constexpr int SB_PPT = 8;             // up to 8192 points
constexpr int SK_BLOCK = 256;
constexpr int SK_CHUNK = 1024;

// (per-instance records and rows written by one workgroup each and read by the next kernel: a 128-byte line of their own,
//  no two workgroups -- XCDs -- write into one cache line; NOTEBOOK 5a)
struct alignas(128) SlabGeo {
  float lo, inv_w;
  int axis, pad;
};
constexpr int SB_PITCH = 544;         // ints per row of bin starts (SB_NB + 1 = 513, rounded up to whole lines)

__device__ __forceinline__ int slab_bin(float v, float lo, float inv_w) {
  const int c = (int)floorf((v - lo) * inv_w);
  return c < 0 ? 0 : (c > SB_NB - 1 ? SB_NB - 1 : c);
}

// sorted: [B][3][N] coordinates in bin order, sidx [B][N] original indices, bstart [B][SB_NB+1], geo [B]
__global__ __launch_bounds__(SB_T) void slab_bin_kernel(const float* __restrict__ pc, int N, float* __restrict__ sorted,
                                                        int32_t* __restrict__ sidx, int32_t* __restrict__ bstart,
                                                        SlabGeo* __restrict__ geo) {
  __shared__ float s_red[16][6];
  __shared__ int s_cnt[SB_NB], s_start[SB_NB + 1], s_wsum[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* P = pc + (size_t)b * 3 * N;
  float px[SB_PPT], py[SB_PPT], pz[SB_PPT];
  float lo[3] = {S_INF, S_INF, S_INF}, hi[3] = {-S_INF, -S_INF, -S_INF};
#pragma unroll
  for (int p = 0; p < SB_PPT; ++p) {
    const int i = tid + p * SB_T;
    if (i < N) {
      px[p] = P[i];
      py[p] = P[N + i];
      pz[p] = P[2 * N + i];
      lo[0] = fminf(lo[0], px[p]); hi[0] = fmaxf(hi[0], px[p]);
      lo[1] = fminf(lo[1], py[p]); hi[1] = fmaxf(hi[1], py[p]);
      lo[2] = fminf(lo[2], pz[p]); hi[2] = fmaxf(hi[2], pz[p]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = -wave_max(-lo[c]);
    hi[c] = wave_max(hi[c]);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_red[wave][c] = lo[c];
      s_red[wave][3 + c] = hi[c];
    }
  }
  if (tid < SB_NB) s_cnt[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = fminf(lo[c], s_red[w][c]);
      hi[c] = fmaxf(hi[c], s_red[w][3 + c]);
    }
  const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  const int axis = (ex >= ey && ex >= ez) ? 0 : (ey >= ez ? 1 : 2);
  const float alo = axis == 0 ? lo[0] : (axis == 1 ? lo[1] : lo[2]);
  const float ext = axis == 0 ? ex : (axis == 1 ? ey : ez);
  const float inv_w = ext > 1e-30f ? (float)SB_NB / (ext * 1.00001f) : 0.f;
  int bin[SB_PPT];
#pragma unroll
  for (int p = 0; p < SB_PPT; ++p) {
    const int i = tid + p * SB_T;
    if (i < N) {
      bin[p] = slab_bin(axis == 0 ? px[p] : (axis == 1 ? py[p] : pz[p]), alo, inv_w);
      atomicAdd(&s_cnt[bin[p]], 1);
    }
  }
  __syncthreads();
  // exclusive scan of the 512 counters by the first 512 threads (one each)
  int c = tid < SB_NB ? s_cnt[tid] : 0, incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) s_wsum[wave] = incl;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) base += (w < wave) ? s_wsum[w] : 0;
  if (tid < SB_NB) {
    s_start[tid] = base + incl - c;
    s_cnt[tid] = 0;
  }
  if (tid == SB_NB - 1) s_start[SB_NB] = base + incl;
  __syncthreads();
  float* S = sorted + (size_t)b * 3 * N;
#pragma unroll
  for (int p = 0; p < SB_PPT; ++p) {
    const int i = tid + p * SB_T;
    if (i < N) {
      const int pos = s_start[bin[p]] + atomicAdd(&s_cnt[bin[p]], 1);
      S[pos] = px[p];
      S[N + pos] = py[p];
      S[2 * N + pos] = pz[p];
      sidx[(size_t)b * N + pos] = i;
    }
  }
  for (int e = tid; e <= SB_NB; e += SB_T) bstart[(size_t)b * SB_PITCH + e] = s_start[e];
  if (tid == 0) geo[b] = SlabGeo{alo, inv_w, axis, 0};
}

typedef float slab_f2 __attribute__((ext_vector_type(2)));
// Two candidates' squared distances to the query per packed instruction.  The query arrives NEGATED (slab_negq, once per
// query): the differences are x + (-q) -- plain v_pk_add_f32 without a source modifier.  (x - q)^2 and (q - x)^2 are the same
// bits.  (Written while `neg` modifiers were suspected of the wrong values of NOTEBOOK 5a; the form that matters turned out to be
// op_sel, which these hand-built pairs never carried.  Kept: it costs nothing and the build refuses op_sel either way.)
__device__ __forceinline__ void slab_sqdist2(float nqx, float nqy, float nqz, float x0, float x1, float y0, float y1,
                                             float z0, float z1, float& d0, float& d1) {
#pragma clang fp contract(off)
  const slab_f2 dx = slab_f2{x0, x1} + slab_f2{nqx, nqx};
  const slab_f2 dy = slab_f2{y0, y1} + slab_f2{nqy, nqy};
  const slab_f2 dz = slab_f2{z0, z1} + slab_f2{nqz, nqz};
  const slab_f2 xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const slab_f2 s = xx + yy;
  const slab_f2 d = s + zz;
  d0 = d.x;
  d1 = d.y;
}
__device__ __forceinline__ void slab_negq(float qx, float qy, float qz, float& nqx, float& nqy, float& nqz) {
  nqx = -qx;
  nqy = -qy;
  nqz = -qz;
  asm volatile("" : "+v"(nqx), "+v"(nqy), "+v"(nqz));   // (opaque: not folded back into a modifier of the packed add)
}

__device__ __forceinline__ bool slab_lex_less(float da, int ia, float db, int ib) {
  return (da < db) || (da == db && ia < ib);
}

// The K smallest of a thread's cnt <= CAP candidates by (distance, index), in order, into slots 0 .. K-1; returns the
// K-th distance.  Small CAP: the whole list goes to registers as 64-bit keys (distance bits : index -- distances are
// >= +0, so the bit patterns order like the values and one integer compare is the lexicographic one), every entry's
// rank is counted over all pairs and the entry is written to the slot of its rank.  No dependent LDS round trips: the
// selection loop below waits for two of them per step (K * cnt / 2 steps: ~30 us per call for a wavefront at K = 17).
template <int CAP>
__device__ __forceinline__ float slab_compact(uint16_t* cand, float* candd, int cnt, int K, int tid) {
  float kth = S_INF;
  if constexpr (CAP <= 40) {
    unsigned long long key[CAP];
    int rank[CAP];
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
      const unsigned d = __float_as_uint(candd[s * SK_BLOCK + tid]);
      const unsigned i = cand[s * SK_BLOCK + tid];
      key[s] = s < cnt ? ((unsigned long long)d << 32) | i : ~0ull;
      rank[s] = CAP - 1 - s;      // as if every later entry were smaller; corrected pair by pair
    }
#pragma unroll
    for (int i = 0; i < CAP; ++i)
#pragma unroll
      for (int j = i + 1; j < CAP; ++j) {
        // lt = key[i] < key[j]; rank[i] -= lt; rank[j] += lt -- compare and both carries back to back (left to the
        // compiler the compares are batched and their lane masks spilled: 4000 v_readlane / v_writelane)
        unsigned long long m;
        asm volatile("v_cmp_lt_u64 %2, %3, %4\n\tv_subbrev_co_u32 %0, vcc, 0, %0, %2\n\t"
                     "v_addc_co_u32 %1, vcc, 0, %1, %2"
                     : "+v"(rank[i]), "+v"(rank[j]), "=&s"(m)
                     : "v"(key[i]), "v"(key[j])
                     : "vcc");
      }
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
      if (rank[s] < K) {
        const float d = __uint_as_float((unsigned)(key[s] >> 32));
        candd[rank[s] * SK_BLOCK + tid] = d;
        cand[rank[s] * SK_BLOCK + tid] = (uint16_t)key[s];
        if (rank[s] == K - 1) kth = d;
      }
    }
    return kth;
  }
  for (int p = 0; p < K; ++p) {
    float bd = candd[p * SK_BLOCK + tid];
    int bidx = cand[p * SK_BLOCK + tid];
    int bs = p;
    for (int s = p + 1; s < cnt; ++s) {
      const float d = candd[s * SK_BLOCK + tid];
      const int i = cand[s * SK_BLOCK + tid];
      if (slab_lex_less(d, i, bd, bidx)) {
        bd = d;
        bidx = i;
        bs = s;
      }
    }
    if (bs != p) {
      candd[bs * SK_BLOCK + tid] = candd[p * SK_BLOCK + tid];
      cand[bs * SK_BLOCK + tid] = cand[p * SK_BLOCK + tid];
      candd[p * SK_BLOCK + tid] = bd;
      cand[p * SK_BLOCK + tid] = (uint16_t)bidx;
    }
    kth = bd;
  }
  return kth;
}

// One staging chunk of the sorted cloud -- coordinates and original indices of cn <= SK_CHUNK points from c0 on -- on its way
// to LDS.  request() issues every load of the thread without a wait between them (a loop of load / wait / LDS write is one
// round trip to memory per trip: four of them per chunk, all workgroups of a launch in the same phase); commit() writes them.
// What the caller puts between the two runs under the loads' latency.  Sixteen dwords per thread (16-byte loads for the
// instances whose rows are aligned were tried: the compiler merges the two forms' registers and waits for everything in
// flight before the second); the addresses are clamped, not predicated (a branch around a load brings its wait along).
// Elements [cn, cn4) are padded with NaN coordinates: the distance is NaN and `d <= tau` is false.
struct SlabRun {
  static constexpr int T = SK_CHUNK / SK_BLOCK;
  float x[T], y[T], z[T];
  int32_t id[T];
  __device__ __forceinline__ void request(const float* __restrict__ Sb, const int32_t* __restrict__ Ib, int N, int c0, int cn,
                                          int tid) {
#pragma unroll
    for (int u = 0; u < T; ++u) {
      const int j = c0 + max(min(tid + u * SK_BLOCK, cn - 1), 0);
      x[u] = Sb[j];
      y[u] = Sb[N + j];
      z[u] = Sb[2 * N + j];
      id[u] = Ib[j];
    }
  }
  __device__ __forceinline__ void commit(float* s_ref, uint16_t* s_id, int cn, int tid) const {
    const int cn4 = (cn + 3) & ~3;
#pragma unroll
    for (int u = 0; u < T; ++u) {
      const int j = tid + u * SK_BLOCK;
      if (j < cn4) {
        const bool ok = j < cn;
        s_ref[j] = ok ? x[u] : __builtin_nanf("");
        s_ref[SK_CHUNK + j] = ok ? y[u] : __builtin_nanf("");
        s_ref[2 * SK_CHUNK + j] = ok ? z[u] : __builtin_nanf("");
        s_id[j] = ok ? (uint16_t)id[u] : (uint16_t)0;
      }
    }
  }
};

template <int CAP>
__global__ __launch_bounds__(SK_BLOCK) void knn_slab_kernel(const float* __restrict__ R, int N, int K,
                                                            const int32_t* __restrict__ prior,
                                                            const float* __restrict__ sorted,
                                                            const int32_t* __restrict__ sidx,
                                                            const int32_t* __restrict__ bstart,
                                                            const SlabGeo* __restrict__ geo, float* __restrict__ dists,
                                                            int32_t* __restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* s_ref = reinterpret_cast<float*>(smem);                                    // 3*SK_CHUNK floats
  float* s_cd = s_ref + 3 * SK_CHUNK;                                               // [CAP][SK_BLOCK]
  uint16_t* s_ci = reinterpret_cast<uint16_t*>(s_cd + (size_t)CAP * SK_BLOCK);      // [CAP][SK_BLOCK]
  uint16_t* s_id = s_ci + (size_t)CAP * SK_BLOCK;                                   // [SK_CHUNK] original indices
  __shared__ int s_lo, s_hi;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int pos = blockIdx.x * SK_BLOCK + tid;
  const bool live = pos < N;
  const float* Rb = R + (size_t)b * 3 * N;
  const float* Sb = sorted + (size_t)b * 3 * N;
  const int32_t* Ib = sidx + (size_t)b * N;
  const int32_t* bs = bstart + (size_t)b * SB_PITCH;
  const SlabGeo g = geo[b];
  const int pc = live ? pos : N - 1;
  const float qx = Sb[pc], qy = Sb[N + pc], qz = Sb[2 * N + pc];
  float nqx, nqy, nqz;
  slab_negq(qx, qy, qz, nqx, nqy, nqz);
  const int qo = Ib[pc];                                     // the query's original index
  if (tid == 0) {
    s_lo = SB_NB;
    s_hi = -1;
  }
  float tau = S_INF;
  if (prior != nullptr && live) {
    // eight neighbours at a time: their indices, then their coordinates, all in flight together (one index / one point
    // per trip of a loop with an exit is 2 K dependent round trips: 30 us of the kernel at K = 17)
    const int32_t* pr = prior + ((size_t)b * N + qo) * K;
    float t = 0.f;
    bool ok = true;
    for (int m0 = 0; m0 < K; m0 += 8) {
      int j[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) j[u] = m0 + u < K ? pr[m0 + u] : 0;
      float px[8], py[8], pz[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        ok = ok && j[u] >= 0 && j[u] < N;
        const int jc = j[u] < 0 ? 0 : (j[u] >= N ? N - 1 : j[u]);
        px[u] = Rb[jc];
        py[u] = Rb[N + jc];
        pz[u] = Rb[2 * N + jc];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (m0 + u < K) t = fmaxf(t, geoa3_sqdist(qx, qy, qz, px[u], py[u], pz[u]));
    }
    if (ok) tau = t;
  }
  if (!live) tau = -1.f;  // padding lanes never collect candidates
  __syncthreads();
  if (live) {
    int blo = 0, bhi = SB_NB - 1;
    if (tau < S_INF) {
      const float qa = g.axis == 0 ? qx : (g.axis == 1 ? qy : qz);
      const float r = sqrtf(tau) * 1.00001f + 1e-30f;
      blo = slab_bin(qa - r, g.lo, g.inv_w);
      bhi = slab_bin(qa + r, g.lo, g.inv_w);
    }
    atomicMin(&s_lo, blo);
    atomicMax(&s_hi, bhi);
  }
  __syncthreads();
  int c_lo = bs[s_lo], c_hi = bs[s_hi + 1];

  // the list's fill state as the BYTE offset of its next distance slot, cnt * (4 SK_BLOCK) + 4 tid: the slot of the index
  // list is half of it, an accepted candidate advances it by one row -- three address instructions per candidate less
  // than from a count
  static_assert(SK_BLOCK == 256, "aoff >> 10 is the count");
  unsigned char* const cdb = reinterpret_cast<unsigned char*>(s_cd);
  unsigned char* const cib = reinterpret_cast<unsigned char*>(s_ci);
  unsigned aoff = 4u * tid;
  int cnt = 0;
  for (int pass = 0; pass < 2; ++pass) {
    // pass 1 only runs if a (bad) prior left some lane with fewer than K candidates: everything, without pruning
    for (int c0 = c_lo; c0 < c_hi; c0 += SK_CHUNK) {
      const int cn = min(SK_CHUNK, c_hi - c0);
      const int cn4 = (cn + 3) & ~3;
      SlabRun run;
      run.request(Sb, Ib, N, c0, cn, tid);   // (in flight across the barrier: the last chunk's readers are what it waits for)
      __syncthreads();
      run.commit(s_ref, s_id, cn, tid);
      __syncthreads();
      // the next four candidates are requested before this step's appends (LDS stores the loads may not be moved across):
      // two waves per SIMD do not hide an LDS round trip per step (the last step's extra read stays inside the arrays)
      float4 nx = *reinterpret_cast<const float4*>(&s_ref[0]);
      float4 ny = *reinterpret_cast<const float4*>(&s_ref[SK_CHUNK]);
      float4 nz = *reinterpret_cast<const float4*>(&s_ref[2 * SK_CHUNK]);
      for (int j = 0; j < cn4; j += 4) {
        const float4 rx = nx, ry = ny, rz = nz;
        const int jn = j + 4 < SK_CHUNK ? j + 4 : j;
        nx = *reinterpret_cast<const float4*>(&s_ref[jn]);
        ny = *reinterpret_cast<const float4*>(&s_ref[SK_CHUNK + jn]);
        nz = *reinterpret_cast<const float4*>(&s_ref[2 * SK_CHUNK + jn]);
        // two candidates per instruction: v_pk_add_f32 / v_pk_mul_f32 are IEEE per component, so with contraction off
        // the distances are the bits of geoa3_sqdist (3 sub + 3 mul + 2 add = 4 packed instructions per point)
        float da[4];
        slab_sqdist2(nqx, nqy, nqz, rx.x, rx.y, ry.x, ry.y, rz.x, rz.y, da[0], da[1]);
        slab_sqdist2(nqx, nqy, nqz, rx.z, rx.w, ry.z, ry.w, rz.z, rz.w, da[2], da[3]);
        // branch-free append: the candidate is written to the list's next slot whether it qualifies or not and the
        // slot is kept only if it does (a passed-over `if` per candidate is a taken branch per candidate: with two
        // waves per SIMD the scan ran at ~140 cycles per candidate).  cnt <= CAP - 4 here (the check below)
        const uint2 ids = *reinterpret_cast<const uint2*>(&s_id[j]);
        const unsigned id4[4] = {ids.x & 0xffffu, ids.x >> 16, ids.y & 0xffffu, ids.y >> 16};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          *reinterpret_cast<float*>(cdb + aoff) = da[u];
          *reinterpret_cast<uint16_t*>(cib + (aoff >> 1)) = (uint16_t)id4[u];
          aoff += da[u] <= tau ? 4u * SK_BLOCK : 0u;
        }
        if (__builtin_expect(__any(aoff > (unsigned)(CAP - 4) * 4u * SK_BLOCK + 4u * SK_BLOCK - 1u), 0)) {   // cnt > CAP - 4
          cnt = (int)(aoff >> 10);
          if (cnt >= K) {
            tau = slab_compact<CAP>(s_ci, s_cd, cnt, K, tid);
            aoff = (unsigned)K * 4u * SK_BLOCK + 4u * tid;
          }
        }
      }
    }
    cnt = (int)(aoff >> 10);
    const bool short_list = live && cnt < K && K <= N;
    if (!__syncthreads_or(short_list) || pass == 1) break;   // (the exact pass is final: geom_nn.hip, knn_kernel)
    tau = live ? S_INF : -1.f;
    cnt = 0;
    aoff = 4u * tid;
    c_lo = 0;
    c_hi = N;
  }

  if (live) {
    const int keep = cnt < K ? cnt : K;
    slab_compact<CAP>(s_ci, s_cd, cnt, keep, tid);
    float* od = dists + ((size_t)b * N + qo) * K;
    int32_t* oi = idx + ((size_t)b * N + qo) * K;
    for (int m = 0; m < K; ++m) {
      od[m] = m < keep ? s_cd[m * SK_BLOCK + tid] : S_INF;
      oi[m] = m < keep ? (int32_t)s_ci[m * SK_BLOCK + tid] : -1;
    }
  }
}

// ------------------------------------------------------------------------------------------
// The slab kernel for a cloud that fits one staging chunk (N <= SK_CHUNK) and short lists (K <= 20): a candidate is
// remembered as its POSITION in the staged run (2 bytes) instead of (distance, index) (6 bytes); the distance is formed
// again, from the same staged coordinates with the same un-fused operations (the same bits), when the list is ranked.
// 34 KB of LDS per workgroup instead of 76: four workgroups per CU instead of two -- the scan is a dependent chain per
// wavefront (compare -> list cursor -> store address) and runs at the rate of the wavefronts that interleave on a SIMD.
// The ranking (64-bit keys in registers, every pair compared once) writes the result straight to memory.
// ------------------------------------------------------------------------------------------
// compile-time loops (indices into register arrays must be constants; a 56 x 56 nest is beyond the unroller's budget)
template <typename F, int... S>
__device__ __forceinline__ void sp_static_for_impl(F&& f, std::integer_sequence<int, S...>) {
  (f(std::integral_constant<int, S>{}), ...);
}
template <int N_, typename F>
__device__ __forceinline__ void sp_static_for(F&& f) {
  sp_static_for_impl(f, std::make_integer_sequence<int, N_>{});
}
// r += (kj < ki): compare + carry back to back (left to the compiler the compares are batched and their masks spilled)
__device__ __forceinline__ void sp_count_less(int& r, unsigned long long kj, unsigned long long ki) {
  asm volatile("v_cmp_lt_u64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(r) : "v"(kj), "v"(ki) : "vcc");
}

#ifdef GEOA3_SP_STAMPS   // probe build: s_memtime at the phase boundaries of eight workgroups of <32, false> (tools/sp_stamps.py)
__device__ unsigned long long g_sp_stamps[8 * 16];
#define SP_STAMP(i)                                                                                                    \
  do {                                                                                                                 \
    if (!MULTI && tid == 0 && blockIdx.x == 1 && (blockIdx.y & 31) == 7 && blockIdx.y < 256)                           \
      g_sp_stamps[(blockIdx.y >> 5) * 16 + (i)] = __builtin_amdgcn_s_memtime();                                        \
  } while (0)
// ... once v has arrived (a stamp behind loads that nothing has used yet would be taken while they are in flight)
#define SP_STAMP_AFTER(i, v)                                                                                           \
  do {                                                                                                                 \
    asm volatile("" ::"v"(v));                                                                                         \
    SP_STAMP(i);                                                                                                       \
  } while (0)
#else
#define SP_STAMP(i)
#define SP_STAMP_AFTER(i, v)
#endif

// Lists of 32 slots at four waves per SIMD (round 4).  With 40 slots the final ranking's keys (80 registers) spilled 35
// registers at the 128 of four waves -- 140 bytes of scratch per lane, 36 MB each way per launch at 250 instances; at three
// waves (168 VGPRs) nothing spilled but the kernel alone took 116 instead of 101 us.  32 slots: 8 bytes of scratch, the list
// is compacted when a lane passes 28 candidates instead of 36 (seeded lists hold K = 17 + the few points inside the old
// radius: p99 21), and the kernel takes 127 instead of 142 us in the bench's one-stream figure, the iteration 1.740 instead
// of 1.755 ms (three interleaved runs, profiles/round4_ab_slab_waves.txt).
// MULTI: a cloud of more than one staging chunk (N <= 65535) and / or longer lists (K <= SP_CAP - 16): the positions are
// those of the whole sorted cloud and the ranking gathers the coordinates from memory (L2) instead of the staged chunk.
template <int SP_CAP, bool MULTI>
__global__ __launch_bounds__(SK_BLOCK) __attribute__((amdgpu_waves_per_eu(MULTI ? 3 : 4, MULTI ? 3 : 4))) void knn_slabp_kernel(const float* __restrict__ R, int N, int K,
                                                             const int32_t* __restrict__ prior,
                                                             const float* __restrict__ sorted,
                                                             const int32_t* __restrict__ sidx,
                                                             const int32_t* __restrict__ bstart,
                                                             const SlabGeo* __restrict__ geo, float* __restrict__ dists,
                                                             int32_t* __restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float s_ref[3 * SK_CHUNK];
  __shared__ __attribute__((aligned(16))) uint16_t s_id[SK_CHUNK];
  // !MULTI: the lists' LDS also holds, before the scan, the cloud in ORIGINAL order and last iteration's lists (the seed
  // radius is formed from LDS, not by 4 K scattered loads per thread) and, after it, the sorted rows on their way out
  constexpr int SP_KMAX = 20;
  constexpr int SP_SEED = 3 * SK_CHUNK * 4 + SK_BLOCK * SP_KMAX * 2;
  constexpr int SP_UNION = !MULTI && SP_SEED > SP_CAP * SK_BLOCK * 2 ? SP_SEED : SP_CAP * SK_BLOCK * 2;
  __shared__ __attribute__((aligned(16))) unsigned char s_un[SP_UNION];
  uint16_t* const s_pos = reinterpret_cast<uint16_t*>(s_un);
  __shared__ int s_lo, s_hi;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int pos = blockIdx.x * SK_BLOCK + tid;
  const bool live = pos < N;
  const float* Rb = R + (size_t)b * 3 * N;
  const float* Sb = sorted + (size_t)b * 3 * N;
  const int32_t* Ib = sidx + (size_t)b * N;
  const int32_t* bs = bstart + (size_t)b * SB_PITCH;
  const SlabGeo g = geo[b];
  const int pc = live ? pos : N - 1;
  // Every load of the prologue is requested before the first wait (the launch is one round of workgroups, all in the same
  // phase: nothing else is resident to cover a round trip to memory, and the loops this replaces made 33 of them one after
  // the other).  First the query's original index -- the rows of the old table hang on it --, then its coordinates.
  const int qo = Ib[pc];
  const float qx = Sb[pc], qy = Sb[N + pc], qz = Sb[2 * N + pc];
  SP_STAMP(0);
  // !MULTI: the sorted cloud is one chunk, so what the scan reads does not depend on the windows: it is requested here and
  // lands in LDS behind the seed radius's walk (profiles/knn_slabp_phases.txt)
  constexpr bool EARLY = !MULTI;
  SlabRun run;
  if (EARLY && prior == nullptr) run.request(Sb, Ib, N, 0, N, tid);
  if (!EARLY && tid == 0) {
    s_lo = SB_NB;
    s_hi = -1;
  }
  float tau = S_INF;
  if (!MULTI && prior != nullptr) {
    // The seed radius: the largest distance to last iteration's K neighbours.  The cloud (original order) and the
    // workgroup's 256 rows of the old table are staged through LDS with coalesced loads (a wavefront fetches ITS 64 rows:
    // 64 K consecutive elements of ~4 rows per load instruction instead of 64 rows), then every thread walks its row.
    float* const s_org = reinterpret_cast<float*>(s_un);
    uint16_t* const s_pri = reinterpret_cast<uint16_t*>(s_un + 3 * SK_CHUNK * 4);
    // the cloud: 3 N <= 3 SK_CHUNK floats, twelve dwords per thread
    constexpr int CT = 3 * SK_CHUNK / SK_BLOCK;
    const int n3 = 3 * N;
    float cl[CT];
#pragma unroll
    for (int u = 0; u < CT; ++u) cl[u] = Rb[min(tid + u * SK_BLOCK, n3 - 1)];
    // the old rows: a wavefront's 64 K <= 64 SP_KMAX elements, every gather requested before the first range check (the
    // rows' original indices come from the wavefront's own lanes)
    const int w0 = tid & ~63, lane = tid & 63;
    const float inv_k = 1.0f / (float)K;
    int32_t pv[SP_KMAX];
    SP_STAMP_AFTER(1, qo);
#pragma unroll
    for (int u = 0; u < SP_KMAX; ++u) {
      const int e = min(lane + 64 * u, 64 * K - 1);
      const int row = (int)(((float)e + 0.5f) * inv_k), m = e - row * K;
      pv[u] = prior[((size_t)b * N + __shfl(qo, row, 64)) * K + m];
    }
    if constexpr (EARLY) run.request(Sb, Ib, N, 0, N, tid);   // (last: the seed radius does not wait for it)
    // (no predicate: s_org holds 3 SK_CHUNK floats whatever N is, and nothing reads beyond 3 N -- a store under `j < 3 N`
    // takes its load along into the branch, with a wait of its own)
#pragma unroll
    for (int u = 0; u < CT; ++u) s_org[tid + u * SK_BLOCK] = cl[u];
    SP_STAMP(2);
    // (opaque: a gather whose only use is the predicated store below is moved into its branch, behind a wait of its own)
#pragma unroll
    for (int u = 0; u < SP_KMAX; ++u) asm volatile("" : "+v"(pv[u]));
#pragma unroll
    for (int u = 0; u < SP_KMAX; ++u) {
      const int e = lane + 64 * u;
      if (e < 64 * K) s_pri[w0 * K + e] = (uint16_t)(pv[u] < 0 || pv[u] >= N ? 0xffff : pv[u]);
    }
    SP_STAMP(3);
    __syncthreads();
    if (live) {
      float t = 0.f;
      bool ok = true;
      for (int m = 0; m < K; ++m) {
        const unsigned j = s_pri[tid * K + m];
        ok = ok && j != 0xffffu;
        const int jc = j >= (unsigned)N ? N - 1 : (int)j;
        t = fmaxf(t, geoa3_sqdist(qx, qy, qz, s_org[jc], s_org[N + jc], s_org[2 * N + jc]));
      }
      if (ok) tau = t;
    }
  }
  if (MULTI && prior != nullptr && live) {
    const int32_t* pr = prior + ((size_t)b * N + qo) * K;
    float t = 0.f;
    bool ok = true;
    for (int m0 = 0; m0 < K; m0 += 8) {
      int j[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) j[u] = m0 + u < K ? pr[m0 + u] : 0;
      float px[8], py[8], pz[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        ok = ok && j[u] >= 0 && j[u] < N;
        const int jc = j[u] < 0 ? 0 : (j[u] >= N ? N - 1 : j[u]);
        px[u] = Rb[jc];
        py[u] = Rb[N + jc];
        pz[u] = Rb[2 * N + jc];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (m0 + u < K) t = fmaxf(t, geoa3_sqdist(qx, qy, qz, px[u], py[u], pz[u]));
    }
    if (ok) tau = t;
  }
  if (!live) tau = -1.f;  // padding lanes never collect candidates
  SP_STAMP(4);
  float nqx, nqy, nqz;
  slab_negq(qx, qy, qz, nqx, nqy, nqz);
  if (!EARLY) __syncthreads();
  int blo = SB_NB, bhi = -1;
  if (live) {
    blo = 0;
    bhi = SB_NB - 1;
    if (tau < S_INF) {
      const float qa = g.axis == 0 ? qx : (g.axis == 1 ? qy : qz);
      const float r = sqrtf(tau) * 1.00001f + 1e-30f;
      blo = slab_bin(qa - r, g.lo, g.inv_w);
      bhi = slab_bin(qa + r, g.lo, g.inv_w);
    }
    if (!EARLY) {
      atomicMin(&s_lo, blo);
      atomicMax(&s_hi, bhi);
    }
  }
  // the workgroup stages the union of its 256 windows (EARLY: the whole sorted cloud); a WAVEFRONT scans only the union of
  // its own 64 (the queries are consecutive along the slab axis: ~2/3 of the workgroup's run)
  const int w_blo = -(int)wave_max(-(float)blo), w_bhi = (int)wave_max((float)bhi);
  int wv_lo = w_blo <= w_bhi ? bs[w_blo] : 0, wv_hi = w_blo <= w_bhi ? bs[w_bhi + 1] : 0;
  // (EARLY: the window's two bin starts are on their way while the run is written; the barrier also ends the seed phase's
  // use of the lists' LDS)
  if constexpr (EARLY) run.commit(s_ref, s_id, N, tid);
  SP_STAMP(5);
  __syncthreads();
  int c_lo = 0, c_hi = N;
  if constexpr (!EARLY) {
    c_lo = bs[s_lo];
    c_hi = bs[s_hi + 1];
  }
  SP_STAMP_AFTER(6, wv_lo + wv_hi + c_lo + c_hi);

  // a thread's list: positions s_pos[slot][tid]; fill state = the BYTE offset of the next slot, cnt * 2 SK_BLOCK + 2 tid
  static_assert(SK_BLOCK == 256, "poff >> 9 is the count");
  unsigned char* const pb = reinterpret_cast<unsigned char*>(s_pos);
  unsigned poff = 2u * tid;
  // positions -> keys in registers: distance bits : original index : position (indices are distinct, so the position
  // never decides an order; it rides along for the write-back); ~0 beyond the list
  unsigned long long key[SP_CAP];
  auto load_keys = [&](auto C_, int cnt) {
    sp_static_for<decltype(C_)::value>([&](auto S_) {
      constexpr int s = decltype(S_)::value;
      unsigned p = s_pos[s * SK_BLOCK + tid];
      float d;
      unsigned id;
      if (MULTI) {
        p = p < (unsigned)N ? p : 0u;     // (slots beyond the list hold anything)
        d = geoa3_sqdist(qx, qy, qz, Sb[p], Sb[N + p], Sb[2 * N + p]);
        id = (unsigned)Ib[p];
      } else {
        p &= SK_CHUNK - 1;
        d = geoa3_sqdist(qx, qy, qz, s_ref[p], s_ref[SK_CHUNK + p], s_ref[2 * SK_CHUNK + p]);
        id = s_id[p];
      }
      key[s] = s < cnt ? ((unsigned long long)__float_as_uint(d) << 32) | (id << 16) | p : ~0ull;
      if ((s & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // eight gathers in flight, not forty (registers)
    });
  };
  // rank of entry s = the number of smaller keys; no rank array -- the caller uses the rank at once (registers)
  auto rank_of = [&](auto C_, auto S_) {
    constexpr int s = decltype(S_)::value;
    int r = 0;
    sp_static_for<decltype(C_)::value>([&](auto J_) {
      constexpr int j = decltype(J_)::value;
      if constexpr (j != s) sp_count_less(r, key[j], key[s]);
    });
    return r;
  };
  for (int pass = 0; pass < 2; ++pass) {
    // pass 1 only runs if a (bad) prior left some lane with fewer than K candidates: everything, without pruning
   for (int c0 = c_lo; c0 < c_hi; c0 += SK_CHUNK) {      // (!MULTI: N <= SK_CHUNK, the whole run at once)
    const int cn = min(SK_CHUNK, c_hi - c0);
    if constexpr (!EARLY) {   // (EARLY: staged in the prologue, and the full scan of pass 1 reads the same chunk)
      run.request(Sb, Ib, N, c0, cn, tid);
      __syncthreads();
      run.commit(s_ref, s_id, cn, tid);
      __syncthreads();
    }
    const int j_lo = min(max(wv_lo - c0, 0), SK_CHUNK - 4) & ~3, j_hi = (min(wv_hi - c0, cn) + 3) & ~3;
    float4 nx = *reinterpret_cast<const float4*>(&s_ref[j_lo]);
    float4 ny = *reinterpret_cast<const float4*>(&s_ref[SK_CHUNK + j_lo]);
    float4 nz = *reinterpret_cast<const float4*>(&s_ref[2 * SK_CHUNK + j_lo]);
    for (int j = j_lo; j < j_hi; j += 4) {
      const float4 rx = nx, ry = ny, rz = nz;
      const int jn = j + 4 < SK_CHUNK ? j + 4 : j;
      nx = *reinterpret_cast<const float4*>(&s_ref[jn]);
      ny = *reinterpret_cast<const float4*>(&s_ref[SK_CHUNK + jn]);
      nz = *reinterpret_cast<const float4*>(&s_ref[2 * SK_CHUNK + jn]);
      float da[4];
      slab_sqdist2(nqx, nqy, nqz, rx.x, rx.y, ry.x, ry.y, rz.x, rz.y, da[0], da[1]);
      slab_sqdist2(nqx, nqy, nqz, rx.z, rx.w, ry.z, ry.w, rz.z, rz.w, da[2], da[3]);
      // branch-free append: the position goes to the list's next slot whether the candidate qualifies or not, and the
      // slot is kept only if it does.  cnt <= SP_CAP - 4 here (the check below)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        *reinterpret_cast<uint16_t*>(pb + poff) = (uint16_t)((MULTI ? c0 : 0) + j + u);
        poff += da[u] <= tau ? 2u * SK_BLOCK : 0u;
      }
      if (__builtin_expect(__any(poff > (unsigned)(SP_CAP - 4) * 2u * SK_BLOCK + 2u * SK_BLOCK - 1u), 0)) {   // cnt > CAP - 4
        const int cnt = (int)(poff >> 9);
        if (cnt >= K) {   // keep the K best (in order), tighten the radius; every old slot is in a register by now
          load_keys(std::integral_constant<int, SP_CAP>{}, cnt);
          sp_static_for<SP_CAP>([&](auto S_) {
            constexpr int s = decltype(S_)::value;
            const int r = rank_of(std::integral_constant<int, SP_CAP>{}, S_);
            if (r < K) s_pos[r * SK_BLOCK + tid] = (uint16_t)key[s];
            if (r == K - 1) tau = __uint_as_float((unsigned)(key[s] >> 32));
          });
          poff = (unsigned)K * 2u * SK_BLOCK + 2u * tid;
        }
      }
    }
   }
    const int cnt = (int)(poff >> 9);
    const bool short_list = live && cnt < K && K <= N;
    if (!__syncthreads_or(short_list) || pass == 1) break;   // (the exact pass is final: geom_nn.hip, knn_kernel)
    tau = live ? S_INF : -1.f;
    poff = 2u * tid;
    c_lo = 0;
    c_hi = N;
    wv_lo = 0;
    wv_hi = N;
  }
  SP_STAMP(7);

  if constexpr (MULTI) {
    if (live) {
      const int cnt = (int)(poff >> 9);
      const int keep = cnt < K ? cnt : K;
      constexpr std::integral_constant<int, SP_CAP> C_{};
      load_keys(C_, cnt);
      float* od = dists + ((size_t)b * N + qo) * K;
      int32_t* oi = idx + ((size_t)b * N + qo) * K;
      sp_static_for<SP_CAP>([&](auto S_) {
        constexpr int s = decltype(S_)::value;
        const int r = rank_of(C_, S_);
        if (r < keep) {
          od[r] = __uint_as_float((unsigned)(key[s] >> 32));
          oi[r] = (int32_t)((key[s] >> 16) & 0xffffu);
        }
      });
      for (int m = keep; m < K; ++m) {   // fewer than K points in the cloud
        od[m] = S_INF;
        oi[m] = -1;
      }
    }
  } else {
    // The final ranking at the length the wavefront's lists actually have -- seeded, a list holds the K old neighbours
    // plus the few points that came inside their radius: 20 or 28 slots instead of SP_CAP (every pair of slots is
    // compared: 380 / 756 pairs instead of 1560); the same keys in the same order either way.  The sorted rows leave
    // through LDS: a row is K consecutive floats, so 64 consecutive elements of the workgroup's 256 K are ~4 rows per
    // store instruction instead of 64 (measured: the scattered stores were a quarter of the kernel).
    const int cnt = live ? (int)(poff >> 9) : 0;
    const int keep = cnt < K ? cnt : K;
    const int cls = !__any(cnt > 20) ? 0 : (!__any(cnt > 28) ? 1 : 2);       // uniform over the wavefront
    constexpr std::integral_constant<int, 20> C20{};
    constexpr std::integral_constant<int, 28> C28{};
    constexpr std::integral_constant<int, SP_CAP> CXX{};
    if (cls == 0) load_keys(C20, cnt);
    else if (cls == 1) load_keys(C28, cnt);
    else load_keys(CXX, cnt);
    __syncthreads();                       // every list, the staged run and its ids are in registers: the LDS is free
    float* const s_od = reinterpret_cast<float*>(s_un);          // [256][K]
    uint16_t* const s_oi = reinterpret_cast<uint16_t*>(s_ref);   // [256][K]
    s_id[tid] = (uint16_t)qo;
    for (int m = keep; m < K; ++m) {       // fewer than K points in the cloud (and the padding lanes)
      s_od[tid * K + m] = S_INF;
      s_oi[tid * K + m] = 0xffff;
    }
    auto rank_out = [&](auto C_) {
      sp_static_for<decltype(C_)::value>([&](auto S_) {
        constexpr int s = decltype(S_)::value;
        const int r = rank_of(C_, S_);
        if (r < keep) {
          s_od[tid * K + r] = __uint_as_float((unsigned)(key[s] >> 32));
          s_oi[tid * K + r] = (uint16_t)(key[s] >> 16);
        }
      });
    };
    if (cls == 0) rank_out(C20);
    else if (cls == 1) rank_out(C28);
    else rank_out(CXX);
    SP_STAMP(8);
    __syncthreads();
    const float inv_k = 1.0f / (float)K;
    const int rows = min(SK_BLOCK, N - (int)blockIdx.x * SK_BLOCK);
    for (int e = tid; e < rows * K; e += SK_BLOCK) {
      const int row = (int)(((float)e + 0.5f) * inv_k), m = e - row * K;
      const size_t o = ((size_t)b * N + s_id[row]) * K + m;
      const unsigned v = s_oi[e];
      dists[o] = s_od[e];
      idx[o] = v == 0xffffu ? -1 : (int32_t)v;
    }
    SP_STAMP(9);
  }
}

// ------------------------------------------------------------------------------------------
// Which search a call of geoa3_knn_self runs: a pure function of its sizes and flags (no GPU work), so that tests can hold
// it to a table (geoa3_debug_knn_self_route).  All routes return the same bits.
// ------------------------------------------------------------------------------------------
enum KnnRoute {
  ALLPAIRS = GEOA3_KNN_ROUTE_ALLPAIRS,
  CELLGRID = GEOA3_KNN_ROUTE_CELLGRID,
  SLAB40 = GEOA3_KNN_ROUTE_SLAB40,      // knn_slab_kernel<CAP>: (distance, index) lists of CAP slots
  SLAB72 = GEOA3_KNN_ROUTE_SLAB72,
  SLAB96 = GEOA3_KNN_ROUTE_SLAB96,
  SLABP32 = GEOA3_KNN_ROUTE_SLABP32,    // knn_slabp_kernel<32, false>: position lists, the cloud in one staging chunk
  SLABP56 = GEOA3_KNN_ROUTE_SLABP56,    // knn_slabp_kernel<56, true>: position lists, any cloud the sort holds
};
constexpr int KNN_SORT_MAX_N = SB_T * SB_PPT;   // the counting sorts hold the cloud in registers: beyond it, all pairs
constexpr int KNN_SHORT_K = 20;                 // lists the short kernels hold (SLAB40, SLABP32)
constexpr int KNN_MID_K = 40;                   // ... and the middle ones (SLAB72, SLABP56)
constexpr int KNN_GRID_MIN_N = 2048;            // method 0: the cell grid from this cloud size on (or above KNN_SHORT_K)
// positions instead of (distance, index) lists: twice the occupancy -- for launches the (distance, index) kernel cannot hold
// at once (two workgroups per CU); a small shard's launch runs beside the victim's kernels, where the denser kernel cost
// more than it saved (32 instances: 0.500 -> 0.506 ms per iteration)
constexpr size_t KNN_DENSE_MIN_WGS = 512;       // position lists for launches of MORE workgroups than this
static_assert(KNN_SORT_MAX_N <= 65535, "positions and original indices travel as 16 bits");

bool knn_self_sizes_ok(int B, int N, int K) { return B > 0 && N > 0 && K > 0 && K <= GEOA3_KNN_MAX_K; }

KnnRoute knn_self_route(int B, int N, int K, int method, bool has_prior, bool scratch_ok) {
  if (!has_prior || !scratch_ok || N > KNN_SORT_MAX_N || K > N) return ALLPAIRS;   // nothing to prune with
  // method 0: the cell grid (one wave per query) for large lists / large clouds, the slab kernel otherwise
  if (method == GEOA3_KNN_SELF_GRID || (method == GEOA3_KNN_SELF_AUTO && (K > KNN_SHORT_K || N >= KNN_GRID_MIN_N)))
    return CELLGRID;
  // (every other value: the slab kernels.)  SLAB_LISTS / SLAB_POSITIONS (tests, A/B runs): the (distance, index)-list
  // kernel / the position-list kernel whatever the launch size
  const size_t wgs = (size_t)((N + SK_BLOCK - 1) / SK_BLOCK) * B;
  const bool positions =
      method != GEOA3_KNN_SELF_SLAB_LISTS && (wgs > KNN_DENSE_MIN_WGS || method == GEOA3_KNN_SELF_SLAB_POSITIONS);
  if (K <= KNN_SHORT_K && N <= SK_CHUNK && positions) return SLABP32;
  if (K <= KNN_MID_K && positions) return SLABP56;
  return K <= KNN_SHORT_K ? SLAB40 : (K <= KNN_MID_K ? SLAB72 : SLAB96);
}

template <int CAP, class Launch>
void launch_slab(Launch&& launch) {
  const size_t lds = 3 * SK_CHUNK * 4 + (size_t)CAP * SK_BLOCK * 6 + SK_CHUNK * 2;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(knn_slab_kernel<CAP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  launch(knn_slab_kernel<CAP>, lds);
}

}  // namespace

extern "C" int64_t geoa3_knn_self_scratch_bytes(int B, int N) {
  if (B <= 0 || N <= 0) return -1;
  const size_t a = knn_self_carve(nullptr, B, N, SB_PITCH, sizeof(SlabGeo)).total, g = geoa3_knn_cellgrid_scratch_bytes(B, N);
  return (int64_t)(a > g ? a : g);
}

#ifdef GEOA3_SP_STAMPS
extern "C" int geoa3_debug_sp_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sp_stamps), sizeof(g_sp_stamps)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int geoa3_debug_knn_self_route(int B, int N, int K, int method, int has_prior, int scratch_ok) {
  if (!knn_self_sizes_ok(B, N, K)) return GEOA3_EINVAL;
  return knn_self_route(B, N, K, method, has_prior != 0, scratch_ok != 0);
}

extern "C" int geoa3_knn_self(const float* pc, int B, int N, int K, const int32_t* prior, float* dists, int32_t* idx,
                              void* scratch, int method, void* stream) {
  if (!pc || !dists || !idx || !knn_self_sizes_ok(B, N, K)) return GEOA3_EINVAL;
  hipStream_t s = geoa3_stream(stream);
  geoa3_prof_begin(GEOA3_PROF_KNN, s);
  int rc = GEOA3_OK;
  const bool scratch_ok = scratch && ((uintptr_t)scratch & 255) == 0;
  // the slab search: the sort, then one of the five scans over its output
  auto slab = [&](auto kernel, size_t lds) {
    const KnnSelfScratch sc = knn_self_carve(scratch, B, N, SB_PITCH, sizeof(SlabGeo));
    SlabGeo* const geo = static_cast<SlabGeo*>(sc.geo);
    hipLaunchKernelGGL(slab_bin_kernel, dim3(B), dim3(SB_T), 0, s, pc, N, sc.sorted, sc.sidx, sc.start, geo);
    hipLaunchKernelGGL(kernel, dim3((N + SK_BLOCK - 1) / SK_BLOCK, B), dim3(SK_BLOCK), lds, s, pc, N, K, prior, sc.sorted,
                       sc.sidx, sc.start, geo, dists, idx);
    if (hipGetLastError() != hipSuccess) rc = GEOA3_ELAUNCH;
  };
  switch (knn_self_route(B, N, K, method, prior != nullptr, scratch_ok)) {
    case ALLPAIRS: rc = geoa3_launch_knn(pc, pc, B, N, N, K, prior, dists, idx, nullptr, s); break;
    case CELLGRID: rc = geoa3_launch_knn_cellgrid(pc, B, N, K, prior, dists, idx, scratch, s); break;
    case SLAB40: launch_slab<40>(slab); break;
    case SLAB72: launch_slab<72>(slab); break;
    case SLAB96: launch_slab<96>(slab); break;
    case SLABP32: slab(knn_slabp_kernel<32, false>, 0); break;
    case SLABP56: slab(knn_slabp_kernel<56, true>, 0); break;
  }
  geoa3_prof_end(GEOA3_PROF_KNN, s);
  return rc;
}
