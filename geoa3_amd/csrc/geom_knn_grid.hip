// Self K-NN through a cell grid (gfx950): the second exact search behind geoa3_knn_self (geom_slab.hip routes here for
// K > 20 or N >= 2048, and for method 2); bit-identical to the all-pairs kernel of geom_nn.hip and to the slab search.
//
// Cell-grid search, one WAVEFRONT per query (the K = 33 / N = 4096 regime, where the per-thread lists of the slab kernel
// leave room for one wave per SIMD and a 1-D slab still holds 10-15 % of the cloud).
// The cloud is counting-sorted into a 16^3 grid over its bounding box (cell index x fastest, so the cells x0..x1 of a
// (y, z) row are ONE contiguous run of the sorted array).  A query's radius tau is the largest distance to last
// iteration's K neighbours (K distinct points: an upper bound of the true K-th distance), so every true neighbour lies in
// the box of cells that [q - sqrt(tau), q + sqrt(tau)] touches (the cell function is monotone in the coordinate).
// The wave gives every (y, z) row of that box to a lane; the lanes walk their runs in lockstep, candidates with d <= tau
// are appended to the wave's list by ballot + popcount (64 at a time), and the K smallest by (distance, index) are
// picked by rank counting over the list -- every lane ranks its own candidates against all of them.  Distances are the
// un-fused bits of geoa3_sqdist and the order is the lexicographic one of the other kernels: BIT-IDENTICAL results.
// No per-thread lists, ~2.5 KB of LDS per wave: eight waves per SIMD hide the dependent loads of the walk.
#include <utility>
#include "geom_internal.h"
#include "geom_knn_self.h"

namespace {

constexpr int KG_G = 16, KG_CELLS = KG_G * KG_G * KG_G;
constexpr int KG_T = 1024, KG_PPT = 8;       // cell sort: up to 8192 points
constexpr int KG_CAP = 256;                  // entries of a wave's candidate list
constexpr int KG_QPW = 8;                    // queries per wave (sequential)

constexpr int KG_PITCH = ((16 * 16 * 16 + 1 + 31) / 32) * 32;   // ints per row of cell starts: whole lines (NOTEBOOK 5a)
// Cells that follow the density: per axis 15 interior boundaries near the 1/16 .. 15/16 quantiles of the cloud's
// coordinates (edges of a 256-bin histogram), cell coordinate = the number of boundaries <= the coordinate.  On a cloud
// with a dense part (75 % of the points on 1/64 of the surface) a query's box of uniform cells held 656 candidates at
// N = 4096, K = 32, of quantile cells 123 (108 / 103 on an ellipsoid: tools' CPU count); any monotone cell function keeps
// the search exact.  bnd[16 axis + m]: boundary m = 1..15 (non-decreasing), entry 0 = +inf (never counted).
struct alignas(128) GridGeo {
  float bnd[48];
};

// the largest m in 0..15 with b[m] <= v (b[1..15] non-decreasing; 0 if none): the cell coordinate
__device__ __forceinline__ int kg_cell_tab(float v, const float* b) {
  int c = v >= b[8] ? 8 : 0;
  c += v >= b[c + 4] ? 4 : 0;
  c += v >= b[c + 2] ? 2 : 0;
  c += v >= b[c + 1] ? 1 : 0;
  return c;
}

// sorted [B][3][N] coordinates in cell order, sidx [B][N] original indices, cstart [B][KG_CELLS + 1], geo [B]
__global__ __launch_bounds__(KG_T) void knn_cellsort_kernel(const float* __restrict__ pc, int N, float* __restrict__ sorted,
                                                            int32_t* __restrict__ sidx, int32_t* __restrict__ cstart,
                                                            GridGeo* __restrict__ geo) {
  __shared__ float s_red[16][6];
  __shared__ int s_cnt[KG_CELLS], s_wsum[16];
  __shared__ int s_hist[3][256];
  __shared__ float s_bnd[48];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* P = pc + (size_t)b * 3 * N;
  float px[KG_PPT], py[KG_PPT], pz[KG_PPT];
  float lo[3] = {S_INF, S_INF, S_INF}, hi[3] = {-S_INF, -S_INF, -S_INF};
#pragma unroll
  for (int p = 0; p < KG_PPT; ++p) {
    const int i = tid + p * KG_T;
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
  for (int e = tid; e < KG_CELLS; e += KG_T) s_cnt[e] = 0;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = fminf(lo[c], s_red[w][c]);
      hi[c] = fmaxf(hi[c], s_red[w][3 + c]);
    }
  // ---- per-axis histograms (256 bins over the axis' own extent) -> boundaries near the 16-quantiles
  if (tid < 768) (&s_hist[0][0])[tid] = 0;
  if (tid < 48) s_bnd[tid] = S_INF;           // (a boundary no count reaches -- or entry 0 -- stays +inf)
  float wbin[3], ibin[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float e = hi[c] - lo[c];
    wbin[c] = e * (1.00001f / 256.f);
    ibin[c] = e > 1e-30f ? 256.f / (e * 1.00001f) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < KG_PPT; ++p) {
    const int i = tid + p * KG_T;
    if (i < N) {
      const float v[3] = {px[p], py[p], pz[p]};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int k = (int)floorf((v[c] - lo[c]) * ibin[c]);
        k = k < 0 ? 0 : (k > 255 ? 255 : k);       // (NaN: bin 0)
        atomicAdd(&s_hist[c][k], 1);
      }
    }
  }
  __syncthreads();
  if (wave < 3) {     // one wave per axis: four fine bins per lane
    const int c = wave;
    int h4[4], sum4 = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      h4[u] = s_hist[c][4 * lane + u];
      sum4 += h4[u];
    }
    int incl4 = sum4;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl4, o, 64);
      if (lane >= o) incl4 += v;
    }
    const int total = __builtin_amdgcn_readlane(incl4, 63);     // the points with a finite place (all of them)
    int run4 = incl4 - sum4;
    const float l0 = c == 0 ? lo[0] : (c == 1 ? lo[1] : lo[2]), w0 = c == 0 ? wbin[0] : (c == 1 ? wbin[1] : wbin[2]);
    for (int u = 0; u < 4; ++u) {
      const int before = run4, after = run4 + h4[u];
      run4 = after;
      if (after > before && total > 0) {
        // boundaries m with before < m total / 16 <= after: the upper edge of this bin
        const int m0 = (int)(((long long)before * 16) / total) + 1, m1 = (int)(((long long)after * 16) / total);
        const float edge = l0 + (float)(4 * lane + u + 1) * w0;
        for (int m = m0; m <= m1 && m <= 15; ++m) s_bnd[16 * c + m] = edge;
      }
    }
  }
  __syncthreads();
  int cell[KG_PPT];
#pragma unroll
  for (int p = 0; p < KG_PPT; ++p) {
    const int i = tid + p * KG_T;
    if (i < N) {
      cell[p] = (kg_cell_tab(pz[p], s_bnd + 32) * KG_G + kg_cell_tab(py[p], s_bnd + 16)) * KG_G + kg_cell_tab(px[p], s_bnd);
      atomicAdd(&s_cnt[cell[p]], 1);
    }
  }
  __syncthreads();
  // exclusive scan of the 4096 counters: four consecutive entries per thread
  int c4[4], sum = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    c4[u] = s_cnt[4 * tid + u];
    sum += c4[u];
  }
  int incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) s_wsum[wave] = incl;
  __syncthreads();
  int run = incl - sum;
#pragma unroll
  for (int w = 0; w < 16; ++w) run += (w < wave) ? s_wsum[w] : 0;
  int32_t* cs = cstart + (size_t)b * KG_PITCH;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    s_cnt[4 * tid + u] = run;     // from here on: the fill cursor of the cell
    cs[4 * tid + u] = run;
    run += c4[u];
  }
  if (tid == KG_T - 1) cs[KG_CELLS] = run;
  __syncthreads();
  float* S = sorted + (size_t)b * 3 * N;
#pragma unroll
  for (int p = 0; p < KG_PPT; ++p) {
    const int i = tid + p * KG_T;
    if (i < N) {
      const int pos = atomicAdd(&s_cnt[cell[p]], 1);   // the order inside a cell is free: the selection does not depend on it
      S[pos] = px[p];
      S[N + pos] = py[p];
      S[2 * N + pos] = pz[p];
      sidx[(size_t)b * N + pos] = i;
    }
  }
  if (tid < 48) geo[b].bnd[tid] = s_bnd[tid];
}

__device__ __forceinline__ unsigned long long kg_key(float d, int i) {   // d >= 0: its bits order like the value
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
}

// element idx of a UNIFORM array through a 32-bit byte offset (idx < 2^30): `global_load v, voffset, s[base]` -- no 64-bit
// address arithmetic per lane
template <class T>
__device__ __forceinline__ T kg_ld(const T* base, unsigned idx) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + idx * (unsigned)sizeof(T));
}
template <class T>
__device__ __forceinline__ void kg_st(T* base, unsigned idx, T v) {
  *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + idx * (unsigned)sizeof(T)) = v;
}

__global__ __launch_bounds__(256) void knn_grid_kernel(const float* __restrict__ R, int N, int K,
                                                       const int32_t* __restrict__ prior,
                                                       const float* __restrict__ sorted, const int32_t* __restrict__ sidx,
                                                       const int32_t* __restrict__ cstart, const GridGeo* __restrict__ geo,
                                                       float* __restrict__ dists, int32_t* __restrict__ idx) {
  __shared__ unsigned long long s_key[4][KG_CAP];
  __shared__ int s_rowp[4][64], s_rows[4][64];   // per wave: exclusive prefix of the rows' lengths, their first positions
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (uniform row bases + UNSIGNED 32-bit indices everywhere below: scalar-base addressing, no 64-bit address arithmetic per
  //  lane -- the kernel is bound by VALU issue)
  const float* Rb = R + (size_t)b * 3 * N;
  const float* Sb = sorted + (size_t)b * 3 * N;
  const float *Sy = Sb + N, *Sz = Sb + 2 * (size_t)N, *Ry = Rb + N, *Rz = Rb + 2 * (size_t)N;
  const int32_t* Ib = sidx + (size_t)b * N;
  const int32_t* cs = cstart + (size_t)b * KG_PITCH;
  // lane 16 axis + m holds boundary m of the axis: a coordinate's cell = the number of its axis' boundaries <= it
  const float bl = lane < 48 ? geo[b].bnd[lane] : S_INF;
  auto cellq = [&](float v, int axis) {      // v wave-uniform
    const unsigned long long mk = __ballot(v >= bl) & (0xfffeull << (16 * axis));
    return (int)__builtin_popcountll(mk);
  };
  unsigned long long* L = s_key[wave];
  int* P = s_rowp[wave];
  int* Sr = s_rows[wave];
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int q0 = (blockIdx.x * 4 + wave) * KG_QPW;
  // A query costs five dependent round trips (its coordinates + index, its prior neighbours, their coordinates, the cell
  // table, the candidates).  The first three are taken off the critical path: lanes 0..KG_QPW-1 load the wave's queries
  // at once, and while query qi is searched the prior indices of query qi + 2 and the neighbour coordinates of query
  // qi + 1 are already in flight (K <= 64: one neighbour per lane).
  float vqx = 0.f, vqy = 0.f, vqz = 0.f;
  int vqo = 0;
  if (lane < KG_QPW && q0 + lane < N) {
    const unsigned ql = (unsigned)(q0 + lane);
    vqx = kg_ld(Sb, ql);
    vqy = kg_ld(Sy, ql);
    vqz = kg_ld(Sz, ql);
    vqo = kg_ld(Ib, ql);
  }
  const bool pipe = K <= 64;
  auto load_prior = [&](int qi) {     // neighbour `lane` of query qi (or -1)
    if (qi >= KG_QPW || q0 + qi >= N || lane >= K) return -1;
    const int32_t* pr = prior + ((size_t)b * N + __builtin_amdgcn_readlane(vqo, qi)) * K;   // uniform
    return (int)kg_ld(pr, (unsigned)lane);
  };
  int jn = pipe ? load_prior(0) : -1;           // indices whose coordinates are requested next
  float cx = 0.f, cy = 0.f, cz = 0.f;            // coordinates of the CURRENT query's neighbour
  bool cok = true;
  auto load_coords = [&](int j) {
    cok = lane >= K || (j >= 0 && j < N);
    const unsigned jj = j >= 0 && j < N ? (unsigned)j : 0u;
    cx = kg_ld(Rb, jj);
    cy = kg_ld(Ry, jj);
    cz = kg_ld(Rz, jj);
  };
  if (pipe) {
    load_coords(jn);
    jn = load_prior(1);
  }
  for (int qi = 0; qi < KG_QPW; ++qi) {
    const int pos = q0 + qi;
    if (pos >= N) break;                       // wave-uniform
    const float qx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vqx), qi));
    const float qy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vqy), qi));
    const float qz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vqz), qi));
    const int qo = __builtin_amdgcn_readlane(vqo, qi);
    // radius: the largest distance to last iteration's K neighbours
    float t = 0.f;
    bool ok = true;
    if (pipe) {
      ok = cok;
      if (lane < K && cok) t = geoa3_sqdist(qx, qy, qz, cx, cy, cz);
      load_coords(jn);                 // query qi + 1
      jn = load_prior(qi + 2);
    } else {
      for (int m = lane; m < K; m += 64) {
        const int j = prior[((size_t)b * N + qo) * K + m];
        if (j < 0 || j >= N) ok = false;
        else t = fmaxf(t, geoa3_sqdist(qx, qy, qz, Rb[j], Rb[N + j], Rb[2 * N + j]));
      }
    }
    float tau = wave_max(t);
    if (__any(!ok)) tau = S_INF;               // no usable radius: the whole grid
    int cnt = 0;                                // wave-uniform
    // second pass only when a degenerate prior (repeated indices) left fewer than K candidates within its radius
    for (int pass = 0; pass < 2; ++pass) {
    int x0 = 0, x1 = KG_G - 1, y0 = 0, y1 = KG_G - 1, z0 = 0, z1 = KG_G - 1;
    if (tau < S_INF) {
      const float r = sqrtf(tau) * 1.00001f + 1e-30f;
      x0 = cellq(qx - r, 0); x1 = cellq(qx + r, 0);
      y0 = cellq(qy - r, 1); y1 = cellq(qy + r, 1);
      z0 = cellq(qz - r, 2); z1 = cellq(qz + r, 2);
    }
    const int ny = y1 - y0 + 1, nrows = ny * (z1 - z0 + 1);
    const float inv_ny = 1.f / (float)ny;     // row / ny below, exact for row < 256, ny <= 16 (no integer division: ~40 instructions)
    cnt = 0;
    for (int rb = 0; rb < nrows; rb += 64) {
      const int row = rb + lane;
      int s = 0, len = 0;
      if (row < nrows) {
        const int rz = (int)(((float)row + 0.5f) * inv_ny);
        const int zz = z0 + rz, yy = y0 + row - rz * ny;
        const int c0 = (zz * KG_G + yy) * KG_G;
        s = kg_ld(cs, (unsigned)(c0 + x0));
        len = kg_ld(cs, (unsigned)(c0 + x1 + 1)) - s;
      }
      // The rows' point ranges, concatenated, are walked 64 candidates at a time (lane = candidate): a lane per ROW left a
      // quarter of the lanes busy and made the loop as long as the longest row -- one L2 round trip per iteration.
      int incl = len;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      const int T = __builtin_amdgcn_readlane(incl, 63);
      P[lane] = incl - len;      // this wave's own slots: LDS operations of a wave execute in order
      Sr[lane] = s;
#ifndef GEOA3_KG_U
#define GEOA3_KG_U 3
#endif
      constexpr int KG_U = GEOA3_KG_U;   // batches of 64 candidates whose loads are in flight together (a query's ~150 candidates
                                         // used to cost one dependent L2 round trip per 64)
      for (int tb = 0; tb < T; tb += 64 * KG_U) {
      float fx[KG_U], fy[KG_U], fz[KG_U];
      int fo[KG_U];
#pragma unroll
      for (int u = 0; u < KG_U; ++u) {
        const int c = tb + 64 * u + lane;
        fx[u] = fy[u] = fz[u] = 0.f;
        fo[u] = 0;
        if (c < T) {
          int r = 0;             // the last row whose range starts at or before candidate c
#pragma unroll
          for (int st = 32; st > 0; st >>= 1)
            if (P[r + st] <= c) r += st;
          const unsigned j = (unsigned)(Sr[r] + (c - P[r]));
          fx[u] = kg_ld(Sb, j);
          fy[u] = kg_ld(Sy, j);
          fz[u] = kg_ld(Sz, j);
          fo[u] = kg_ld(Ib, j);
        }
      }
#pragma unroll
      for (int u = 0; u < KG_U; ++u) {
        const int t0 = tb + 64 * u;
        if (t0 >= T) break;      // wave-uniform
        const int c = t0 + lane;
        const float d = c < T ? geoa3_sqdist(qx, qy, qz, fx[u], fy[u], fz[u]) : S_INF;
        const int oi = fo[u];
        const bool pass = c < T && d <= tau;
        const unsigned long long mask = __ballot(pass);
        if (pass) L[cnt + __popcll(mask & lt)] = kg_key(d, oi);
        cnt += __popcll(mask);
        if (cnt > KG_CAP - 64) {                // wave-uniform, rare: keep the K best, tighten the radius
          // rank counting over the list; the K smallest move to the front (through registers: 4 entries per lane)
          unsigned long long mine[KG_CAP / 64];
          int rk[KG_CAP / 64];
#pragma unroll
          for (int u = 0; u < KG_CAP / 64; ++u) {
            const int c = lane + 64 * u;
            mine[u] = c < cnt ? L[c] : ~0ull;
            rk[u] = 0;
          }
          for (int j2 = 0; j2 < cnt; ++j2) {
            const unsigned long long kj = L[j2];
#pragma unroll
            for (int u = 0; u < KG_CAP / 64; ++u) rk[u] += kj < mine[u] ? 1 : 0;
          }
          const int keep = cnt < K ? cnt : K;
#pragma unroll
          for (int u = 0; u < KG_CAP / 64; ++u)
            if (lane + 64 * u < cnt && rk[u] < keep) L[rk[u]] = mine[u];
          cnt = keep;
          if (keep == K) tau = __uint_as_float((unsigned)(L[K - 1] >> 32));
        }
      }
      }
    }
    if (cnt >= K || K > N || !(tau < S_INF)) break;
    tau = S_INF;
    }
    // the K smallest of the list by (distance, index): every lane ranks its own entries -- ONE per lane when the list holds
    // at most 64 (the usual case: the K old neighbours + the few points that moved inside their radius), so the rank loop
    // is a broadcast read, a compare and an add per entry instead of four compares (the kernel is bound by VALU issue:
    // ~700 instructions per query, 250 of them here)
    {
      float* od = dists + ((size_t)b * N + qo) * K;
      int32_t* oi = idx + ((size_t)b * N + qo) * K;
      auto rank_emit = [&](auto ul) {
        constexpr int UL = decltype(ul)::value;
        unsigned long long mine[UL];
        int rk[UL];
#pragma unroll
        for (int u = 0; u < UL; ++u) {
          const int c = lane + 64 * u;
          mine[u] = c < cnt ? L[c] : ~0ull;
          rk[u] = 0;
        }
#pragma unroll 4
        for (int j2 = 0; j2 < cnt; ++j2) {
          const unsigned long long kj = L[j2];
#pragma unroll
          for (int u = 0; u < UL; ++u) rk[u] += kj < mine[u] ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < UL; ++u)
          if (lane + 64 * u < cnt && rk[u] < K) {
            kg_st(od, (unsigned)rk[u], __uint_as_float((unsigned)(mine[u] >> 32)));
            kg_st(oi, (unsigned)rk[u], (int32_t)(unsigned)(mine[u] & 0xffffffffull));
          }
      };
      if (cnt <= 64) rank_emit(std::integral_constant<int, 1>{});
      else if (cnt <= 128) rank_emit(std::integral_constant<int, 2>{});
      else rank_emit(std::integral_constant<int, KG_CAP / 64>{});
      for (int m = cnt + lane; m < K; m += 64) {   // fewer than K candidates (K > N): the all-pairs kernel's padding
        od[m] = S_INF;
        oi[m] = -1;
      }
    }
  }
}

}  // namespace

static_assert(GEOA3_KNN_MAX_K <= KG_CAP - 64, "a wave's list holds the K kept entries and the next 64 candidates");

size_t geoa3_knn_cellgrid_scratch_bytes(int B, int N) {
  return knn_self_carve(nullptr, B, N, KG_PITCH, sizeof(GridGeo)).total;
}

int geoa3_launch_knn_cellgrid(const float* pc, int B, int N, int K, const int32_t* prior, float* dists, int32_t* idx,
                              void* scratch, hipStream_t s) {
  const KnnSelfScratch gs = knn_self_carve(scratch, B, N, KG_PITCH, sizeof(GridGeo));
  GridGeo* const geo = static_cast<GridGeo*>(gs.geo);
  hipLaunchKernelGGL(knn_cellsort_kernel, dim3(B), dim3(KG_T), 0, s, pc, N, gs.sorted, gs.sidx, gs.start, geo);
  dim3 ggrid((N + 4 * KG_QPW - 1) / (4 * KG_QPW), B);
  hipLaunchKernelGGL(knn_grid_kernel, ggrid, dim3(256), 0, s, pc, N, K, prior, gs.sorted, gs.sidx, gs.start, geo, dists, idx);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
