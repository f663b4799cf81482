/*
 * geoa3_hip.h -- C ABI of libgeoa3_hip.so: the MI355X (gfx950) implementation of the GeoA3
 * inner attack loop (Gorilla-Lab-SCUT/GeoA3: Attacker/geoA3_attack.py + Lib/loss_utils.py +
 * Model/PointNet.py).  Plain pointers and sizes only; no torch types.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - point tensors are planar fp32 [B,3,N] (the reference's logical layout): plane c of
 *     instance b starts at base + (b*3 + c)*N, so a wavefront reads 64 consecutive floats;
 *   - indices are int32; distances are squared L2, evaluated un-fused as
 *       d = fl(fl(fl(dx*dx)+fl(dy*dy))+fl(dz*dz))   (bit-identical to the CPU oracle);
 *     exact distance ties go to the LOWER index;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every entry
 *     point only enqueues work: no allocation, no host synchronisation, no global state
 *     (the opt-in diagnostics of geoa3_hip_debug.h -- event timers, single-kernel entry points for the
 *     tools/ benchmarks -- are declared apart from this ABI and never change results);
 *   - return value: 0 on success, a negative GEOA3_E* code otherwise (geoa3_strerror()).
 *     The reference prints and exit(-1)s on a launch failure
 *     (Model/pointnet2_ops_lib/pointnet2_ops/_ext-src/include/cuda_utils.h:30-39); callers of
 *     this library are expected to raise instead.
 *
 * Each declaration cites the reference interface it replaces (file:line under the reference
 * repository).  INTEGRATION.md shows the ctypes binding a maintainer of the reference adds.
 */
#ifndef GEOA3_HIP_H
#define GEOA3_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEOA3_OK 0
#define GEOA3_EINVAL (-1)   /* bad argument (null pointer, size out of the supported range) */
#define GEOA3_ELAUNCH (-2)  /* hipLaunchKernel / hipGetLastError reported a failure */
#define GEOA3_ENOSUPPORT (-3)

/* The ABI version of this header: bumped on EVERY change of a struct layout or a signature.  geoa3_version() returns the
 * value the library was built with; a binding must refuse a library whose version differs (geoa3_amd/_lib.py does: a
 * stale or variant .so would misread the argument structs silently). */
#define GEOA3_ABI_VERSION 609
int geoa3_version(void);
const char* geoa3_strerror(int code);

/* ------------------------------------------------------------------------------------------
 * Operator level: pytorch3d.ops.knn_points as called from
 * Lib/loss_utils.py:32,33,41,48,57,70,77,92 and Attacker/geoA3_attack.py:65,80.
 * ------------------------------------------------------------------------------------------ */

/* K = 1, both directions in ONE launch ("CD kernel"): for every point of `a` its nearest
 * point of `r` (d_ar, i_ar: [B,Na]) and for every point of `r` its nearest point of `a`
 * (d_ra, i_ra: [B,Nr]).  Replaces the knn_points(K=1) pairs at Lib/loss_utils.py:32-33 (and the
 * repeated adv->ori queries at :48,:70,:92).  d_ra/i_ra may be NULL (one direction only,
 * pseudo_chamfer_loss, Lib/loss_utils.py:41).
 * Non-finite coordinates: the answer is the running minimum from (+inf, 0) over ascending indices with the strict `d < best`,
 * so a NaN distance (a NaN coordinate; +inf against +inf on one axis) and a +inf distance are never taken, and a query
 * without a finite distance answers (+inf, 0): every index lies in [0, N) of the searched cloud, a distance is never NaN.
 * The other instances of the batch keep their bits (tests/_nonfinite_ref.py, tests/test_gpu_nonfinite.py). */
int geoa3_nn1_pair(const float* a, const float* r, int B, int Na, int Nr,
                   float* d_ar, int32_t* i_ar, float* d_ra, int32_t* i_ra, void* stream);

/* geoa3_nn1_pair, pruned -- bit-identical results for any input.  Clouds of 1025..4096 points: a uniform grid over the
 * searched cloud (16^3 cells, rebuilt per call in LDS), every query scans the cells its seed's ball touches: O(N) instead
 * of O(N^2) work per instance for surface-like clouds; where the balls hold a large part of the cloud (dense clusters,
 * thin parts, iterates far from the surface), and for every other cloud size (with fewer than 32 points: all pairs), the
 * matrix core forms approximate distances of all pairs and only the pairs under the seed's radius (plus a bound on the
 * approximation's error) are evaluated exactly (csrc/geom_filter.hip).  prior_ar [B,Na] / prior_ra [B,Nr] (optional, MAY ALIAS i_ar / i_ra): an index into the
 * searched cloud per query, e.g. last iteration's answer; it only seeds the search radius (default: the point with
 * the query's own index), any value gives the exact result.
 * Non-finite coordinates: the rule of geoa3_nn1_pair, for every prior.  A searched cloud that holds a NaN / inf coordinate, or
 * whose extent is not finite, is searched without grid and without matrix core (the exact sweep, all pairs); so is a
 * workgroup of queries that holds one. */
int geoa3_grid_nn1_pair(const float* a, const float* r, int B, int Na, int Nr, const int32_t* prior_ar,
                        const int32_t* prior_ra, float* d_ar, int32_t* i_ar, float* d_ra, int32_t* i_ra, void* stream);

/* General K (1..GEOA3_KNN_MAX_K): dists/idx [B,Nq,K] ascending by (distance, index).
 * `prior` (optional, [B,Nq,K], int32, K DISTINCT valid indices per query, e.g. the previous
 * iteration's result) only seeds the pruning radius; the result is exact for any prior (an entry outside [0, Nr) is not
 * followed: the query is searched without a radius).
 * Non-finite coordinates: the candidates of a query are the points whose distance is not NaN -- a +inf distance IS one and
 * sorts behind every finite one, lowest index first; slots beyond the candidates (K > Nr, NaN distances) are (+inf, -1).  A
 * query with a NaN coordinate therefore comes out as K times (+inf, -1), and a table may hold -1: a consumer must look at an
 * index before it follows it.  (geoa3_knn_nd has the OTHER rule: a NaN distance counts as +inf and its indices stay in
 * range.)  Every other row, and every other instance of the batch, keeps its bits.
 * Replaces knn_points(K=k+1) at Lib/loss_utils.py:57,77. */
#define GEOA3_KNN_MAX_K 64
int geoa3_knn(const float* q, const float* r, int B, int Nq, int Nr, int K,
              const int32_t* prior, float* dists, int32_t* idx, void* stream);

/* Self K-NN of one cloud (q == r == pc, [B,3,N]) == geoa3_knn(pc, pc, B, N, N, K, prior, ...) bit for bit, pruned by
 * the radius `prior` gives (the K-th distance among last iteration's neighbours), with one of two searches:
 *   method 1 (slab): the cloud is counting-sorted along its longest axis and each workgroup of queries scans only the
 *            contiguous run of sorted points whose coordinate can lie within the queries' radius;
 *   method 2 (grid): the cloud is counting-sorted into a 16^3 grid and ONE WAVEFRONT per query walks the cell rows its
 *            ball touches, collects candidates by ballot and picks the K smallest by rank counting (no per-thread
 *            lists: the form for K > 20 or N >= 2048);
 *   method 0: picks by (K, N) -- and, for the slab search, by launch size between two bit-identical kernels: candidates
 *            kept as (distance, index) pairs (method 3 forces it) or as 2-byte positions (method 4; denser, the choice
 *            for launches of more than 512 workgroups).
 * Without `prior` or `scratch`, or for N > 8192, it runs the all-pairs kernel.  scratch:
 * geoa3_knn_self_scratch_bytes(B, N) bytes, 256-byte aligned, contents irrelevant.
 * Non-finite coordinates and a `prior` that holds -1 (last iteration's table of a diverged instance): geoa3_knn's rule and
 * bits on every route -- the row of a NaN point is K times (+inf, -1), and that point is in no other row.
 * Replaces knn_points(adv, adv, K=k+1) at Lib/loss_utils.py:77. */
#define GEOA3_KNN_SELF_AUTO 0            /* `method`; any other value behaves as GEOA3_KNN_SELF_SLAB */
#define GEOA3_KNN_SELF_SLAB 1
#define GEOA3_KNN_SELF_GRID 2
#define GEOA3_KNN_SELF_SLAB_LISTS 3
#define GEOA3_KNN_SELF_SLAB_POSITIONS 4
int64_t geoa3_knn_self_scratch_bytes(int B, int N);
int geoa3_knn_self(const float* pc, int B, int N, int K, const int32_t* prior, float* dists, int32_t* idx,
                   void* scratch, int method, void* stream);

/* pytorch3d.ops.knn_gather and the backward passes of knn_gather / knn_points, in the OPERATORS' layouts -- NOT the planar
 * one of the rest of this header: point-major float32 (x [B,M,U], p [B,N,3]) and int64 indices, as the operators hand them
 * over; no conversion pass.  Sizes: K >= 1, U >= 1, E = L K entries per instance with B E < 2^31 and B (M + 1) < 2^31
 * (GEOA3_EINVAL / GEOA3_ENOSUPPORT otherwise).  Every output element is written.  An index outside [0, M) is the caller's
 * error: it is never dereferenced -- the gather writes NaN to that element, the backward passes drop the term.
 * Where pytorch3d (and torch.scatter_add) sum with float atomics, every sum here is SEQUENTIAL in float32, starts from
 * +0.0f and runs in ascending entry number e = l K + k: a function of the call's arguments only (not of the run, of the
 * other instances of the batch or of workgroup ids), which a float32 loop on the CPU reproduces bit for bit.
 *
 * knn_gather (Lib/loss_utils.py:58,71,78, Attacker/geoA3_attack.py:66,81, Lib/utility.py:46,97,121):
 *   out[b,l,k,:] = x[b, idx[b,l,k], :];  x [B,M,U], idx [B,L,K], out [B,L,K,U]. */
int geoa3_knn_gather(const float* x, const int64_t* idx, int B, int M, int L, int K, int U, float* out, void* stream);
/* scratch of the two backward passes (the counting sort of an instance's E entries by destination): bytes, < 0 when the
 * sizes are out of range; contents irrelevant, 4-byte aligned. */
int64_t geoa3_knn_scatter_scratch_bytes(int B, int E, int M);
/* the backward of the gather at the same call sites: gx[b,j,c] = sum of g[b,l,k,c] over the entries with idx[b,l,k] == j
 * (+0.0 where nobody points);  g [B,L,K,U], gx [B,M,U], scratch: geoa3_knn_scatter_scratch_bytes(B, L K, M). */
int geoa3_knn_gather_grad(const float* g, const int64_t* idx, int B, int M, int L, int K, int U, float* gx, void* scratch,
                          void* stream);
/* the backward of knn_points through `dists` (pytorch3d's knn backward; the searches of Lib/loss_utils.py:57,70,77 and
 * Attacker/geoA3_attack.py:65,80 whose distances are differentiated):
 *   t(i,k,c) = fl( fl(2 gd[i,k]) * fl(p1[i,c] - p2[idx[i,k],c]) )        (no fused multiply-add)
 *   g1[i,c]  = sum over ascending k of t(i,k,c)
 *   g2[j,c]  = sum of -t(i,k,c) over the entries with idx[i,k] == j, in ascending e = i K + k
 * p1 [B,N1,3], p2 [B,N2,3], idx / gd [B,N1,K]; g1 [B,N1,3] or NULL, g2 [B,N2,3] or NULL (not both);
 * scratch: geoa3_knn_scatter_scratch_bytes(B, N1 K, N2), may be NULL when g2 is. */
int geoa3_knn_points_grad(const float* p1, const float* p2, const int64_t* idx, const float* gd, int B, int N1, int N2, int K,
                          float* g1, float* g2, void* scratch, void* stream);

/* knn_points in D dimensions (a dynamic-graph network's search in feature space), point-major like the operator:
 * q [B,Nq,D], r [B,Nr,D] -> dists / idx [B,Nq,K] ascending by (distance, index), exactly equal distances to the lower
 * index.  The squared distance is the SEQUENTIAL float32 sum acc = fl(acc + fl(fl(q_d - r_d)^2)) over d = 0 .. D-1 from
 * +0.0, no fused multiply-add: a float32 loop on the CPU reproduces both outputs bit for bit.  A NaN distance (a
 * non-finite coordinate) is ordered and reported as +inf, so every index lies in [0, Nr).  Exact, all pairs.
 * Supported: 1 <= D <= GEOA3_KNN_ND_MAX_D, 1 <= K <= min(Nr, GEOA3_KNN_MAX_K), Nq, Nr <= 8192, B <= 65535; anything else
 * returns GEOA3_EINVAL / GEOA3_ENOSUPPORT and writes nothing. */
#define GEOA3_KNN_ND_MAX_D 128
int geoa3_knn_nd(const float* q, const float* r, int B, int Nq, int Nr, int D, int K, float* dists, int32_t* idx,
                 void* stream);

/* The neighbour half of an eval-mode EdgeConv layer, max_k LeakyReLU_0.2(BN(W [x_j - x_i ; x_i])), with the BatchNorm
 * folded: the pre-activation of edge (i, j) is U[j] + V[i] + t, U = (s W_a) x, V = (s (W_b - W_a)) x (the caller's GEMMs).
 * U, V [B,N,C] point-major, t [C], idx int64 [B,N,K] ->
 *   arg[b,i,c] (int32 [B,N,C]) = the first slot s that maximises U[b, idx[b,i,s], c] (a NaN, once met, stays);
 *   y[b,c,i]   ([B,C,N])       = lrelu(fl(fl(U[b,idx[b,i,arg],c] + V[b,i,c]) + t[c])),  lrelu(a) = a > 0 ? a : fl(0.2f a).
 * An index outside [0,N) is never dereferenced: the point's y is NaN, arg its first such slot.  Sizes: N K < 2^31 - 256,
 * B <= 65535 (GEOA3_EINVAL / GEOA3_ENOSUPPORT otherwise, nothing written). */
int geoa3_edge_max(const float* U, const float* V, const float* t, const int64_t* idx, int B, int N, int C, int K, float* y,
                   int32_t* arg, void* stream);
/* scratch of geoa3_edge_max_grad (the destination lists of idx): bytes, < 0 when the sizes are out of range. */
int64_t geoa3_edge_max_scratch_bytes(int B, int N, int K);
/* its backward: g, y [B,C,N], arg, idx as above -> dV[b,i,c] = g'[b,i,c] = y > 0 ? g : fl(0.2f g), and dU[b,j,c] = the
 * sequential float32 sum, from +0.0, of the g'[b,i,c] with idx[b,i,arg[b,i,c]] == j in ascending (i, slot) order (an index
 * outside [0,N) gives no term).  No float atomics.  dU, dV [B,N,C]. */
int geoa3_edge_max_grad(const float* g, const float* y, const int32_t* arg, const int64_t* idx, int B, int N, int C, int K,
                        float* dU, float* dV, void* scratch, void* stream);


/* _get_kappa_ori (Lib/loss_utils.py:52-62) given the self K-NN table knn_idx [B,N,k+1]
 * (column 0, the nearest hit, is dropped exactly as the reference's [:, :, :, 1:] slice):
 *   kappa[b,i] = mean_m | < normalize(p[knn_idx[b,i,m]] - p_i), n_i > |,  m = 1..k.
 * nn_idx (optional, [B,N]): normals are taken from normal[:, nn_idx[b,i]] -- the
 * _get_kappa_adv form (Lib/loss_utils.py:64-82); NULL = normal[:, i].  normal is [B,3,Nn] (Nn = 0 means N;
 * Nn != N only with nn_idx: the dense-cloud path, where pc is an npoint-sample of a cloud of Nn points). */
int geoa3_kappa(const float* pc, const float* normal, const int32_t* knn_idx, const int32_t* nn_idx,
                int B, int N, int Nn, int k, float* kappa, void* stream);

/* ------------------------------------------------------------------------------------------
 * Objective level: the geometric part of _forward_step (Attacker/geoA3_attack.py:131-166) and its
 * gradient, fused.  Consumes the tables produced by geoa3_nn1_pair / geoa3_knn.
 * ------------------------------------------------------------------------------------------ */
typedef struct geoa3_geo_args {
  /* inputs */
  const float* adv;        /* [B,3,N] current iterate                                  */
  const float* ori;        /* [B,3,Nr] clean cloud                                     */
  const float* normal_ori; /* [B,3,Nr]         (may be NULL when w_curv == 0)          */
  const float* kappa_ori;  /* [B,Nr]           (may be NULL when w_curv == 0)          */
  const float* d_ao;       /* [B,N] adv->ori squared distance                          */
  const int32_t* i_ao;     /* [B,N] adv->ori index                                     */
  const float* d_oa;       /* [B,Nr] ori->adv      (NULL when single_side or dis_type != CD) */
  const int32_t* i_oa;     /* [B,Nr]                                                   */
  const int32_t* knn_adv;  /* [B,N,k+1] self K-NN of adv (NULL when w_curv == 0)       */
  const float* dkappa;     /* [B,N] optional upstream d L / d kappa_adv: when given, the curvature part of
                              `grad` is the vector-Jacobian product of _get_kappa_adv with it (operator-level
                              autograd) instead of the curvature_loss gradient                */
  int32_t B, N, k;
  int32_t Nr;              /* points of ori / normal_ori / kappa_ori / d_oa / i_oa; 0 = N.  Nr > N is the dense-cloud
                              path (--is_subsample_opt, geoA3_attack.py:283-284): adv is the npoint-sample */
  int32_t dis_type;        /* 0 = none, 1 = CD (chamfer_loss / pseudo_chamfer_loss), 2 = L2 (norm_l2_loss) */
  int32_t single_side;     /* --is_cd_single_side                                      */
  float w_dis, w_hd, w_curv; /* dis_loss_weight, hd_loss_weight, curv_loss_weight     */
  /* outputs (each may be NULL) */
  float* dis_loss;         /* [B] chamfer_loss / pseudo_chamfer_loss / norm_l2_loss, Lib/loss_utils.py:25-43 */
  float* hd_loss;          /* [B] hausdorff_loss, Lib/loss_utils.py:45-50              */
  float* curv_loss;        /* [B] curvature_loss, Lib/loss_utils.py:84-97              */
  float* constrain;        /* [B] w_dis*dis + w_hd*hd + w_curv*curv (geoA3_attack.py:137,153,162) */
  float* kappa_adv;        /* [B,N] _get_kappa_adv, Lib/loss_utils.py:64-82            */
  float* grad;             /* [B,3,N] d constrain[b] / d adv[b]                        */
  /* deterministic != 0: every point's gradient is summed by its owner in a fixed order (own terms, then the pulls it
   * receives sorted by source) instead of with LDS float atomics: bit-for-bit reproducible and independent of the rest
   * of the batch (what the reference's scatter-adds -- knn_gather / index backward -- do not promise either).
   * Clouds of at most 1024 points take the pair-parallel kernel (a lane per (centre, neighbour) pair, reverse lists as
   * fixed-capacity rows in LDS, rows sorted in registers; a row beyond its ~50 slots -- a dense cluster, a hub of the
   * K-NN graph -- through 64-bit fixed-point sums in a small pool, order-free); 1025..4096 points with `scratch`: the
   * pair-parallel kernel with fixed-point sums; otherwise up to ~4800 points the one-workgroup kernel with LDS reverse lists; beyond (up to 5839)
   * the sums fall back to LDS float atomics (free order) whatever this flag says.  5840..8192 points need `scratch` and take
   * the two-pass kernels with fixed-point sums, order-free whatever this flag says; without `scratch`, or beyond 8192
   * points, the call returns GEOA3_ENOSUPPORT. */
  int32_t deterministic;
  /* optional workspace of geoa3_geo_scratch_bytes(B, N, k) bytes: 16 * B * N (one float4 record per point) up to 4096 points,
   * the records plus the partial loss sums of every 1024 points beyond.  Given, clouds of 1025..4096 points (and smaller
   * ones with k > 32) with the curvature term take the pair-parallel kernel with 64-bit fixed-point gradient sums (geo_big_kernel: order-free and
   * therefore reproducible; the neighbour table is read once); NULL = the one-workgroup kernel.  Same values to rounding.
   * The fixed-point sums take two power-of-two scales per instance from its largest coefficient X (2 w_curv / (N k) or
   * max |dkappa| / k, and the Chamfer coefficients): terms up to 2^10 X at 2^-40 X per unit, terms up to 2^34 X (pairs down
   * to ~1e-10 apart) at 2^-16 X through a pool of 256 destinations.  A term beyond that, a NaN, or a full pool writes NaN
   * into the gradient of the destination point -- there is no silent saturation.
   * Clouds of 5840..8192 points (what no single workgroup's LDS holds; required there, with or without the curvature term):
   * pass A, a workgroup per 1024 centres, writes kappa_adv, the records (normal, pair coefficient) and partial loss sums;
   * pass B, a workgroup per owner range of ceil(N / S) points (S = the fewest ranges that fit LDS: 2 up to ~7400 points, 4
   * beyond), streams table and records once and keeps the 64-bit sums of its own range.  Same two scales, with both limits
   * halved (2^9 X and 2^33 X; once more per doubling of N + Nr beyond 16384) so that N + Nr terms cannot wrap a sum.  The
   * gradient depends on neither S nor the batch; the loss values are summed per 1024 points, then in that order.
   * Clouds of 4097..5839 points take the one-workgroup kernel whether `scratch` is given or not. */
  void* scratch;
} geoa3_geo_args;
/* The tables and what is not an index.  Every kernel compares every entry it reads from a table with its range before it
 * forms an address from it: knn_adv and i_oa against [0, N), i_ao against [0, Nr).  (geoa3_knn / geoa3_knn_self write -1
 * into the row of a point with a NaN coordinate, and for K > N.)  An entry outside is not followed and its term counts as
 * NaN: for knn_adv the pair's -- kappa_adv and the curvature loss of the instance, the gradient of the row's own point and,
 * through its coefficient, of the neighbours it does name; for i_ao the point's distance and curvature terms -- its
 * gradient and kappa_adv; for i_oa the clean point's -- dis_loss and constrain of the instance (no point is pulled).  The
 * other instances keep their bits (csrc/geom_loss_fix.h, geo_tab_idx; tests/test_gpu_nonfinite.py runs every route on such
 * tables).  geoa3_kappa treats knn_idx and nn_idx the same way: the point's kappa is NaN.
 * The Hausdorff point of an instance whose d_ao holds +inf is the LOWEST index among the +inf entries (larger value, then
 * lower index; a NaN never wins), on every route. */
int geoa3_geo_loss_grad(const geoa3_geo_args* args, void* stream);
/* bytes of geoa3_geo_args.scratch for B clouds of N points (k: the neighbours per point; 0 = none) */
int64_t geoa3_geo_scratch_bytes(int B, int N, int k);

/* ------------------------------------------------------------------------------------------
 * Victim model: PointNet eval forward and input-gradient (Model/PointNet.py:56-160).
 * Weights: BatchNorm folded and repacked by the host (geoa3_amd/pointnet.py) into the arrays
 * below; all fp32, row-major [C_out, K] with K contiguous unless noted.
 * ------------------------------------------------------------------------------------------ */
typedef struct geoa3_tnet_weights {   /* transform_net, Model/PointNet.py:56-94 */
  int32_t K;                /* 3 or 64 */
  const float *w1, *b1;     /* conv1+bn1 folded  [64,K]           */
  const float *w2, *b2;     /* conv2+bn2         [128,64]         */
  const float *w3, *b3;     /* conv3+bn3         [1024,128]       */
  const float *w3p;         /* w3 in MFMA A-fragment order (see w5p) */
  const float *w2t;         /* [64,128] = w2^T (input-gradient; conv3's is sparse and reads w3) */
  const float *f1, *fb1;    /* fc1+bn4 [512,1024] */
  const float *f2, *fb2;    /* fc2+bn5 [256,512]  */
  const float *f3, *fb3;    /* fc3     [K*K,256]  */
  const float *f1t, *f2t, *f3t; /* transposes: [1024,512], [512,256], [256,K*K] */
  const void *w3h;          /* optional (NULL = fp32 MFMA; see w5h): v = w3 * 2^e as split-fp16 pieces in MFMA 32x32x16
                               fragment order [T = co/32][s = k/16][piece hi,lo][lane 0..63][j 0..7] = piece(w3[32T +
                               (lane&31)][16s + 8(lane>>5) + j]) (csrc/pointnet_wide_split.hip) */
  float w3h_unscale;        /* 2^-e */
  const void *w2th;         /* optional, with w3h: w2t [64,128] as split-fp16 fragments (the packing of w3h, T = row/32, K = 128):
                               the A operands of the backward's fused kernel (sparse gradient of conv3 + conv2's backward in
                               one launch).  NULL: the two run as separate kernels (same bits, slower) */
  float w2th_unscale;
} geoa3_tnet_weights;

#define GEOA3_PN_NO_FUSE_BWD 1 /* sparse backward and the 128 -> 64 layer behind it as two kernels (same bits) */
#define GEOA3_PN_NO_CHAIN 2    /* the 64-input layers one kernel each instead of chains (same bits) */
#define GEOA3_PN_NO_PRE_LISTS 8 /* the sparse backward builds its hit lists per workgroup instead of reading the forward's (same bits) */
#define GEOA3_PN_KEYS_CLEAN 4  /* geoa3_pointnet_forward: the caller vouches that the LAST call that used `workspace` was a
                                  geoa3_pointnet_forward with the same (B, N) (backward calls in between are fine) -- the
                                  arg-max keys in it are then zero already (every layer's finalize leaves them so) and the
                                  forward does not clear them again: one launch less per iteration of a loop */
typedef struct geoa3_pointnet_weights {  /* PointNet, Model/PointNet.py:96-160 */
  int32_t classes;
  geoa3_tnet_weights t3, t64;
  const float *w1, *b1;     /* conv1+bn1 [64,3]    */
  const float *w2, *b2;     /* conv2+bn2 [64,64]   */
  const float *w3, *b3;     /* conv3+bn3 [64,64]   */
  const float *w4, *b4;     /* conv4+bn4 [128,64]  */
  const float *w5, *b5;     /* conv5+bn5 [1024, 3*128]: k = tap*128 + ci (kernel 3, pad 1, PointNet.py:110) */
  const float *w5p;         /* w5 in MFMA A-fragment order: [(T*3+tap)*16+j][lane 0..63][i 0..3] =
                               w5[32T + (lane&31)][tap*128 + 8j + 4(lane>>5) + i] -- one coalesced 16-byte load per lane */
  const float *w4t, *w3t, *w2t;  /* [64,128] [64,64] [64,64] (transposes for the input-gradient) */
  const float *f1, *fb1;    /* fc1+bn6 [512,1024] */
  const float *f2, *fb2;    /* fc2+bn7 [256,512]  */
  const float *f3, *fb3;    /* fc3     [classes,256] */
  const float *f1t, *f2t, *f3t; /* [1024,512] [512,256] [256,classes] */
  const void *w5h;          /* optional (NULL = the 1024-wide layers run on the fp32 MFMA): v = w5 * 2^e as TWO fp16 values
                               per weight, hi = rn16(v), lo = rn16(v - hi), in MFMA 16x16x32 fragment order
                               [T = co/16][s = k/32][piece hi,lo][lane 0..63][j 0..7] = piece(w5[16T + (lane&15)][32s +
                               8(lane>>4) + j]); the layer then evaluates a*w = a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on the
                               f16 matrix pipe with fp32 accumulation (csrc/pointnet_wide16.hip).  Both or neither
                               of the T-Nets' w3h must be given with it.  Given, the 64/128-wide convolutions and the
                               Gram product of the backward use the same arithmetic (they split their fp32 weights
                               themselves: csrc/pointnet_conv_split.hip, pointnet_gram.hip); NULL = fp32 MFMA throughout. */
  float w5h_unscale;        /* 2^-e */
  const void *w4th;         /* optional, with w5h: w4t [64,128] as split-fp16 fragments (see t3.w2th) */
  float w4th_unscale;
  int32_t flags;            /* GEOA3_PN_* bits; 0 = the default kernels */
} geoa3_pointnet_weights;

/* bytes of scratch the forward+backward pair needs for a batch of B clouds of N points */
int64_t geoa3_pointnet_workspace_bytes(int B, int N, int classes);

/* logits[B,classes] = net(x[B,3,N]); keeps the activations backward needs in `workspace`.
 * Replaces `net(input_curr_iter)` at Attacker/geoA3_attack.py:103 (and the b batch-1 calls at :297).
 * Non-finite points (the rule of geoa3_pn2ssg_forward, and the reference's own outcome: relu(NaN) = NaN, the max keeps it):
 * a cloud with a NaN or infinite coordinate gets NaN in all of its logits, and geoa3_pointnet_backward gives NaN in all of
 * its dx under finite dlogits; the other clouds of the batch keep every bit of the result they have without it.  The
 * cloud's flag is its T3 [9] in the workspace (NaN), raised through the arg-max keys by the first kernel that reads the
 * cloud: no extra launch, the same under graph replay and with GEOA3_PN_KEYS_CLEAN. */
int geoa3_pointnet_forward(const geoa3_pointnet_weights* w, const float* x, int B, int N,
                           float* logits, void* workspace, void* stream);

/* dx[B,3,N] = d( sum_b <dlogits[b], logits[b]> ) / d x, for the forward that last filled
 * `workspace`.  Replaces the autograd walk of loss.backward() through the network
 * (Attacker/geoA3_attack.py:326); weight gradients are never formed.
 * Both directions refuse the same arguments with GEOA3_EINVAL, before any GPU work: a NULL pointer, B or N not positive,
 * t3.K != 3, t64.K != 64, classes <= 0, a workspace that is not 256-byte aligned (until ABI 609 the backward checked
 * only the pointers and the sizes). */
int geoa3_pointnet_backward(const geoa3_pointnet_weights* w, const float* x, const float* dlogits,
                            int B, int N, float* dx, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Driver level: device-resident state of attack() (Attacker/geoA3_attack.py:182-386).
 * ------------------------------------------------------------------------------------------ */
typedef struct geoa3_attack_state {
  int32_t B, N, classes;
  int32_t targeted;          /* cfg.attack_label != 'Untarget' (geoA3_attack.py:189-192) */
  int32_t cls_loss_type;     /* 0 = None, 1 = CE, 2 = Margin (geoA3_attack.py:105-127)   */
  float confidence;          /* cfg.confidence                                          */
  float inv_global_batch;    /* 1 / b of `loss_n.mean()` (geoA3_attack.py:178); the GLOBAL b when sharded */
  const int32_t* gt;         /* [B] ground-truth labels                                 */
  const int32_t* target;     /* [B] attack targets (== gt when untargeted, geoA3_attack.py:211-214) */
  float* scale_const;        /* [B] */
  float* lower_bound;        /* [B] */
  float* upper_bound;        /* [B] */
  float* best_loss;          /* [B] init 1e10 */
  float* best_attack;        /* [B,3,N] init 1.0 (geoA3_attack.py:226) */
  int32_t* best_step;        /* [B] init -1 */
  int32_t* best_bs;          /* [B] init -1 */
  float* iter_best_loss;     /* [B] reset to 1e10 per binary step */
  int32_t* iter_best_score;  /* [B] reset to -1 per binary step   */
  float* prev_constrain;     /* [B] reset to 1e10 per binary step (geoA3_attack.py:233,301) */
  int32_t* label;            /* [B] arg-max label of the current iterate */
  float* cls_loss;           /* [B] */
  float* loss_n;             /* [B] */
  float* loss_hist;          /* [iter_max_steps, B] (all_loss_list, geoA3_attack.py:229,321) or NULL */
  int32_t* last_label;       /* [1] label of the LAST instance at the LAST step (the `output_label`
                                reused for every k at geoA3_attack.py:375) */
} geoa3_attack_state;

/* Per step, after the forward: classification loss + d loss/d logits, arg-max label, the success
 * bookkeeping of geoA3_attack.py:288-310 for the CURRENT iterate x with the PREVIOUS step's
 * constrain loss, loss_n = cls + scale_const*constrain, and prev_constrain <- constrain.
 * dlogits[B,classes] already carries inv_global_batch. */
int geoa3_attack_head(const geoa3_attack_state* st, const float* logits, const float* constrain,
                      const float* x, int step, int search_step, float* dlogits, void* stream);
/* The dense-cloud form (--is_subsample_opt with more points than cfg.npoint, geoA3_attack.py:283-296): `logits` are
 * those of the npoint-sample the objective is evaluated on (classification loss, dlogits); success and
 * output_label come from vote_logits [B, eval_num, classes], the victim's answers on eval_num independent
 * farthest-point resamplings of the full iterate: success = more than half of them satisfy _compare, label = their
 * mode (smallest on ties, as torch.mode).  eval_num <= 64.  x / best_attack stay the FULL cloud (st->N points). */
int geoa3_attack_head_vote(const geoa3_attack_state* st, const float* logits, const float* vote_logits, int eval_num,
                           const float* constrain, const float* x, int step, int search_step, float* dlogits,
                           void* stream);
/* The same step in two launches, for callers that overlap the geometry kernels with the victim's backward:
 * _classify = the part that needs only the logits (cls_loss, label, last_label, d loss / d logits, the success flag of
 * geoA3_attack.py:297-300 -> ok [B] int32); _finish = loss_n / loss history and the best-so-far bookkeeping of
 * :301-310 once the constrain loss is known.  _classify + _finish == geoa3_attack_head_vote bit for bit. */
int geoa3_attack_head_classify(const geoa3_attack_state* st, const float* logits, const float* vote_logits, int eval_num,
                               float* dlogits, int32_t* ok, void* stream);
int geoa3_attack_head_finish(const geoa3_attack_state* st, const int32_t* ok, const float* constrain, const float* x,
                             int step, int search_step, void* stream);

/* Per step, after both backward passes: g = g_cls + scale_const[b]*inv_global_batch*g_geo, then the
 * optimiser update of `offset` (torch.optim.Adam defaults or plain SGD, geoA3_attack.py:269-272,
 * 323-331), optional lp_clip (geoA3_attack.py:88-98,349-352), and x = ori + offset for the next step.
 * step_size = lr/(1-beta1^t) and sqrt_bc2 = sqrt(1-beta2^t) are formed on the host in double
 * exactly as torch.optim.Adam does.  optim: 0 = adam, 1 = sgd (step_size = lr). */
int geoa3_attack_update(const geoa3_attack_state* st, const float* g_cls, const float* g_geo,
                        const float* ori, float* offset, float* adam_m, float* adam_v, float* x,
                        int optim, float step_size, float sqrt_bc2, float cc_linf, void* stream);

/* --is_partial_var (geoA3_attack.py:239-262,278-281, Lib/utility.py:211-216): the optimised variable is `part`
 * [B,3,kr] on the kr points pidx [B,kr] of every instance, x = periodical + pad(part).  optim -1: only writes
 * x[:, :, pidx] = periodical + part (after a re-draw); 0: Adam step (scalars as geoa3_attack_update); 1: SGD with
 * `momentum` (first != 0: the momentum buffer pm is initialised with the gradient, torch.optim.SGD). */
int geoa3_attack_partial_step(const geoa3_attack_state* st, const float* g_cls, const float* g_geo, const int32_t* pidx,
                              int kr, const float* periodical, float* part, float* pm, float* pv, float* x, int optim,
                              float step_size, float sqrt_bc2, float momentum, int first, void* stream);

/* The flag-gated projections that follow the optimiser step (--is_pro_grad / --is_real_offset,
 * geoA3_attack.py:59-85,341-347), one point per thread.
 *   mode 0 (find_offset, :79-85):  offset = x - ori[:, nn[b,i]]            (nn = nearest original of x)
 *   mode 1 (offset_proj, :59-77):  n = normal_ori[:, nn[b,i]] with nn = nearest original point OF THE OFFSET
 *          VECTOR (the reference queries knn_points with `offset` as the cloud, :65);
 *          offset = <offset, n/(|n|+1e-6)> n/(|n|+1e-6); then lp_clip (cc_linf != 0, :88-98,349-352) and
 *          x = ori + offset. */
int geoa3_attack_project(int mode, const float* ori, const float* normal_ori, const int32_t* nn, float* offset,
                         float* x, int B, int N, float cc_linf, void* stream);

/* End of a binary step: the scale_const / bound update of geoA3_attack.py:374-384, bug-compatible
 * (uses *last_label for every instance).  It touches scale_const and the two bounds only: the per-binary-step state
 * (iter_best_*, prev_constrain) is re-armed by geoa3_attack_begin_search_step, as the reference resets it at the top of
 * its loop (:231-233). */
int geoa3_attack_binary_update(const geoa3_attack_state* st, void* stream);

/* Start of a binary step: offset <- init_offset, adam state <- 0, x = ori + offset, per-step state reset. */
int geoa3_attack_begin_search_step(const geoa3_attack_state* st, const float* ori, const float* init_offset,
                                   float* offset, float* adam_m, float* adam_v, float* x, void* stream);

/* ------------------------------------------------------------------------------------------
 * PointNet++ operators: the nine functions of the reference's vendored CUDA extension `pointnet2_ops._ext`
 * (Model/pointnet2_ops_lib/pointnet2_ops/_ext-src/src/bindings.cpp:6-19): the six the SSG classifier uses, and
 * three_nn / three_interpolate / three_interpolate_grad of the feature-propagation (FP) module.
 * Layouts as in the extension: xyz [B,N,3] point-major, features [B,C,N], indices int32.
 * ------------------------------------------------------------------------------------------ */
/* sampling.cpp:66-87 / sampling_gpu.cu:69-229.  temp: optional [B,N] scratch that receives the final running
 * distances (the extension's `tmp` tensor); idx [B,m]. */
int geoa3_pn2_furthest_point_sampling(const float* xyz, int B, int N, int m, float* temp, int32_t* idx, void* stream);
/* sampling.cpp:25-43 / sampling_gpu.cu:8-30: out[b,c,j] = points[b,c,idx[b,j]] */
int geoa3_pn2_gather_points(const float* points, const int32_t* idx, int B, int C, int N, int M, float* out,
                            void* stream);
/* sampling.cpp:45-64 / sampling_gpu.cu:34-57: scatter-add into grad_points [B,C,N] (zeroed here) */
int geoa3_pn2_gather_points_grad(const float* grad_out, const int32_t* idx, int B, int C, int N, int M,
                                 float* grad_points, void* stream);
/* ball_query.cpp:10-32 / ball_query_gpu.cu:9-54: idx [B,M,nsample] (zeroed here) */
int geoa3_pn2_ball_query(const float* new_xyz, const float* xyz, int B, int N, int M, float radius, int nsample,
                         int32_t* idx, void* stream);
/* The same two with `flags`.  GEOA3_PN2_CONTRACT: the squared distances (and the sampler's |p|^2 <= 1e-3 skip test) as
 * fmaf(dz, dz, fmaf(dy, dy, dx * dx)) -- what nvcc's default -fmad=true makes of sampling_gpu.cu:100,103-104 and
 * ball_query_gpu.cu:31-32 (setup.py:32 builds with -O3 and no -fmad flag) -- instead of the un-fused default.  For
 * comparing indices with a CUDA run of the reference; the two forms differ only at near-ties. */
#define GEOA3_PN2_CONTRACT 1
int geoa3_pn2_furthest_point_sampling_ex(const float* xyz, int B, int N, int m, float* temp, int32_t* idx, int flags,
                                         void* stream);
int geoa3_pn2_ball_query_ex(const float* new_xyz, const float* xyz, int B, int N, int M, float radius, int nsample,
                            int32_t* idx, int flags, void* stream);
/* group_points.cpp:13-34 / group_points_gpu.cu:8-39: out[b,c,j,k] = points[b,c,idx[b,j,k]] */
int geoa3_pn2_group_points(const float* points, const int32_t* idx, int B, int C, int N, int M, int nsample,
                           float* out, void* stream);
/* group_points.cpp:36-58 / group_points_gpu.cu:43-75: scatter-add into grad_points [B,C,N] (zeroed here) */
int geoa3_pn2_group_points_grad(const float* grad_out, const int32_t* idx, int B, int C, int N, int M, int nsample,
                                float* grad_points, void* stream);
/* interpolate.cpp:14-40 / interpolate_gpu.cu:9-68: for every point of unknown [B,n,3] the three nearest of known [B,m,3],
 * dist2 [B,n,3] (SQUARED distances, ascending) and idx [B,n,3].  The reference's scan exactly: k = 0 .. m-1 in order, the
 * strict `<` cascade (equal distances stay in ascending index), NaN / +inf distances never selected, unfilled slots
 * (m < 3) = (+inf, 0).  Any n, m >= 1.  _ex: `flags` as above (GEOA3_PN2_CONTRACT: the distance of :33 contracted). */
int geoa3_pn2_three_nn(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                       void* stream);
int geoa3_pn2_three_nn_ex(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                          int flags, void* stream);
/* the kernel's tile sizes (known points per LDS tile, unknown points per workgroup): for tests that straddle them */
int geoa3_pn2_three_nn_tile(int* known_tile, int* unknown_tile);
/* interpolate.cpp:42-70 / interpolate_gpu.cu:72-111: out[b,c,j] = (p[i1] * w1 + p[i2] * w2) + p[i3] * w3 with
 * p = points[b,c,:] ([B,C,m]), (i1,i2,i3) = idx[b,j,:], (w1,w2,w3) = weight[b,j,:]; out [B,C,n].  Un-fused; _ex with
 * GEOA3_PN2_CONTRACT: fmaf(p3, w3, fmaf(p2, w2, p1 * w1)).  An index outside [0,m) is the caller's error: it is not
 * wrapped, the element comes out as NaN. */
int geoa3_pn2_three_interpolate(const float* points, const int32_t* idx, const float* weight, int B, int C, int m, int n,
                                float* out, void* stream);
int geoa3_pn2_three_interpolate_ex(const float* points, const int32_t* idx, const float* weight, int B, int C, int m,
                                   int n, float* out, int flags, void* stream);
/* interpolate.cpp:71-99 / interpolate_gpu.cu:116-154: grad_points[b,c,i] = sum over (j,slot) with idx[b,j,slot] == i of
 * grad_out[b,c,j] * weight[b,j,slot]; grad_points [B,C,m] is written in full (0 where nobody points).  Instead of the
 * reference's float atomics every destination sums its contributions in ascending (j, slot) order: bit-reproducible,
 * and row b does not depend on the rest of the batch.  scratch: geoa3_pn2_three_interpolate_scratch_bytes(B, n, m)
 * bytes (< 0: sizes out of range) for the per-instance counting sort of the 3n entries by destination. */
int64_t geoa3_pn2_three_interpolate_scratch_bytes(int B, int n, int m);
int geoa3_pn2_three_interpolate_grad(const float* grad_out, const int32_t* idx, const float* weight, int B, int C, int n,
                                     int m, float* grad_points, void* scratch, void* stream);

/* Tails of the shared MLPs (pointnet2_modules.py:9-19: Conv2d 1x1 + BatchNorm2d + ReLU; :62-70: max over nsample)
 * around the channel GEMMs, eval mode, BatchNorm scale already folded into the GEMM weights:
 *   bias_relu:           z [B,C,L] <- relu(z + shift[c])                         (in place)
 *   relu_grad:           dz = (y > 0) ? g : 0                                     (dz may alias g)
 *   bias_relu_max:       out [B,C,M] = relu(max_s z[B,C,M,S] + shift[c]), arg = first maximising s (F.max_pool2d)
 *   bias_relu_max_grad:  dz [B,C,M,S] = (s == arg && out > 0) ? g : 0 */
int geoa3_pn2_bias_relu(float* z, const float* shift, int B, int C, long L, void* stream);
/* The first layer of a set-abstraction MLP is linear in the gathered inputs, W [xyz_j - c_m ; f_j] = (W_x xyz + W_f f)_j
 * - (W_x c)_m: it is applied to the npoint UN-grouped columns once and the result gathered (geoa3_pn2_group_points);
 * what remains per grouped element is a shift per (instance, channel, centre) and the relu:
 *   shift_relu:       z[row][s] <- relu(z[row][s] + shift[row]),  row = (b, c, m), s < S   (in place)
 *   shift_relu_grad:  dz = y > 0 ? g : 0,  dshift[row] = sum_s dz[row][s]
 * (replaces the grouping of xyz, the cat and the K = C + 3 GEMM over npoint * nsample columns of
 * pointnet2_utils.py:318-331 + pointnet2_modules.py:57-64). */
int geoa3_pn2_shift_relu(float* z, const float* shift, long rows, int S, void* stream);
/* gather + shift + relu in one pass: out[b][c][m][s] = relu(points[b][c][idx[b][m][s]] + shift[b][c][m]);
 * shift_relu_grad with y == NULL: g is already gated, only dshift[row] = sum_s g[row][s] is formed */
/* group_points_grad + rowsum[b][c][m] = sum_s grad_out[b][c][m][s] in the same pass (nsample == 64; GEOA3_ENOSUPPORT
 * otherwise: use geoa3_pn2_shift_relu_grad with y == NULL) */
int geoa3_pn2_group_points_grad_sums(const float* grad_out, const int32_t* idx, int B, int C, int N, int M, int nsample,
                                     float* grad_points, float* rowsum, void* stream);
int geoa3_pn2_group_shift_relu(const float* points, const int32_t* idx, const float* shift, int B, int C, int N, int M,
                               int nsample, float* out, void* stream);
int geoa3_pn2_shift_relu_grad(const float* y, const float* g, float* dz, float* dshift, long rows, int S, void* stream);
int geoa3_pn2_relu_grad(const float* y, const float* g, float* dz, long total, void* stream);
int geoa3_pn2_bias_relu_max(const float* z, const float* shift, int B, int C, long M, int S, float* out, int32_t* arg,
                            void* stream);
int geoa3_pn2_bias_relu_max_grad(const float* g, const float* out, const int32_t* arg, int B, int C, long M, int S,
                                 float* dz, void* stream);

/* Channel-major 1x1 convolution with fused epilogue, the shared-MLP layer of pointnet2_modules.py:57-64 (Conv2d 1x1 +
 * eval BatchNorm2d folded into W / bias + ReLU) on [B,K,N] -> [B,Co,N] (N = npoint * nsample, contiguous):
 *   Y[b][co][n] = epi( sum_k W[co][k] X[b][k][n] ),  epi = (+ bias[co] if bias) (relu if relu) (0 where Z[b][co][n] <= 0 if Z)
 * K in {64, 128, 256}, Co a multiple of 64; fp32 in and out, split-fp16 operands on the f16 matrix pipe inside
 * (csrc/pointnet_conv_split.hip).  The input-gradient of such a layer is the same call with W^T and Z = the layer's
 * input activation. */
int geoa3_conv1x1(const float* X, const float* W, const float* bias, const float* Z, float* Y, int B, long N, int K,
                  int Co, int relu, void* stream);

/* The last layer of a set-abstraction MLP with F.max_pool2d over the 64 samples of a centre in its epilogue (the
 * [B,Co,npoint,64] activation is never written): out[b][co][m] = relu(max_s (W x)[co][64 m + s] + bias[co]), arg = the
 * first maximal sample (pointnet2_modules.py:57-70).  K = 128, Co a multiple of 64, N = 64 * npoint. */
int geoa3_conv1x1_max64(const float* X, const float* W, const float* bias, float* out, int32_t* arg, int B, long N, int K,
                        int Co, void* stream);
/* ... and its input gradient: the pooled layer's sparse gradient ((arg == s) ? g : 0; g and arg CENTRE-major
 * [B][npoint][K]; g must carry the pooled output's relu gate) is formed in registers, multiplied by W ([Co][K] = the transposed layer weight, K = 256) and gated by the
 * relu of the layer below (keep where Z > 0). */
int geoa3_conv1x1_onehot64(const float* g, const int32_t* arg, const float* W, const float* Z, float* Y, int B, long N,
                           int K, int Co, void* stream);

/* First set-abstraction level of the SSG classifier, fused (PointNetPP_ssg.py:58-66: npoint 512, radius 0.2, nsample 64,
 * mlp [3, 64, 64, 128]; pointnet2_modules.py:29-74, pointnet2_utils.py:296-333): grouped xyz (xyz[idx] - new_xyz) ->
 * three Conv2d 1x1 + eval BatchNorm2d (folded into w / shift b by the host) + ReLU -> max over the 64 samples.
 * xyz [B,N,3], new_xyz [B,M,3] point-major as in the reference; idx [B,M,64] from geoa3_pn2_ball_query;
 * out [B,M,128] CENTROID-major (one contiguous 512-byte row per centroid; the caller transposes to the reference's
 * [B,128,M]); arg [B,M,128] (u8: the arg-max sample, first on ties like F.max_pool2d) is what backward needs. */
typedef struct geoa3_sa1_weights {
  const float *w1, *b1;   /* [64,3],   [64]  */
  const float *w2, *b2;   /* [64,64],  [64]  */
  const float *w3, *b3;   /* [128,64], [128] */
} geoa3_sa1_weights;
int geoa3_pn2_sa1_forward(const float* xyz, const float* new_xyz, const int32_t* idx, const geoa3_sa1_weights* w, int B,
                          int N, int M, float* out, uint8_t* arg, void* stream);
/* grad_xyz [B,N,3] (the scatter-add over idx) and grad_new_xyz [B,M,3] (= minus the per-centroid sum) from
 * grad_out [B,M,128] (same layout as out); the hidden activations are recomputed, not stored.
 * scratch: geoa3_pn2_sa1_scratch_bytes(B, M) bytes -> the scatter-add as order-free 64-bit fixed-point sums at the
 * instance's own scale (deterministic, batch-independent; a NaN / infinite contribution gives NaN, not a clamp);
 * NULL -> global float atomics as the reference (group_points_gpu.cu:60). */
int64_t geoa3_pn2_sa1_scratch_bytes(int B, int M);
int geoa3_pn2_sa1_backward(const float* xyz, const float* new_xyz, const int32_t* idx, const geoa3_sa1_weights* w, int B,
                           int N, int M, const float* out, const uint8_t* arg, const float* grad_out, float* grad_xyz,
                           float* grad_new_xyz, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * The whole PointNet++ SSG classifier (eval mode) as a native victim: forward and input gradient, the counterpart of
 * geoa3_pointnet_forward / _backward for BASELINE configs[3].  Replaces `PointNet2ClassificationSSG.forward`
 * (Model/PointNetPP_ssg.py:106-124: SA(512, r 0.2, 64 samples, [3,64,64,128]) -> SA(128, r 0.4, 64, [131,128,128,256])
 * -> SA(GroupAll, [259,256,512,1024]) -> Linear/BN/ReLU 1024-512-256 -> Linear classes; modules
 * pointnet2_modules.py:29-74, groupers pointnet2_utils.py:296-379) and torch autograd's backward through it.
 * Every Conv2d 1x1 / Linear (no bias) + eval BatchNorm is passed FOLDED: W' = diag(bn.weight / sqrt(var + eps)) W,
 * shift = bn.bias - mean * scale.  The first layer of levels 2 and 3 is split into its xyz columns (w?_wx [Co,3], the
 * first three input channels: QueryAndGroup / GroupAll cat xyz first) and its feature columns (w?_wf); *t = the
 * transposed matrix ([K,Co] row-major) used by the input gradient.
 * x, dx: planar [B,3,N] (the attack's layout), 32 <= N <= 8192 (a cloud of fewer than 512 points has its points repeated
 * by the sampler, as in the reference); workspace: geoa3_pn2ssg_workspace_bytes(B, N) bytes, 256-byte
 * aligned, the SAME buffer for forward and the backward that follows it (backward reads the forward's activations).
 * ------------------------------------------------------------------------------------------ */
typedef struct geoa3_pn2ssg_weights {
  int classes;
  geoa3_sa1_weights sa1;
  const float *sa2_wx, *sa2_wf, *sa2_b0, *sa2_wft;   /* [128,3], [128,128], [128], [128,128] */
  const float *sa2_w1, *sa2_b1, *sa2_w1t;            /* [128,128], [128], [128,128] */
  const float *sa2_w2, *sa2_b2, *sa2_w2t;            /* [256,128], [256], [128,256] */
  const float *sa3_wx, *sa3_wf, *sa3_b0, *sa3_wft;   /* [256,3], [256,256], [256], [256,256] */
  const float *sa3_w1, *sa3_b1, *sa3_w1t;            /* [512,256], [512], [256,512] */
  const float *sa3_w2, *sa3_b2, *sa3_w2t;            /* [1024,512], [1024], [512,1024] */
  const float *f1, *fb1, *f1t;                       /* [512,1024], [512], [1024,512] */
  const float *f2, *fb2, *f2t;                       /* [256,512], [256], [512,256] */
  const float *f3, *fb3, *f3t;                       /* [classes,256], [classes], [256,classes] */
  const void* images;   /* geoa3_pn2ssg_pack_images of THESE weights, or NULL (the forward then rebuilds them per call) */
  void* side;           /* geoa3_side_queue_create(), or NULL: one stream.  With it the forward is pipelined: the sampler's rounds
                           of level 1 in four launches, each followed by the gather + ball query of its 128 centroids, and then
                           level 2's sampling, ball query and shift (functions of the level-1 centroids only) on the queue's
                           stream, beside level 1's MLP on `stream`; joined in front of level 2's MLP.  Same bits; the call is
                           still ordered on `stream` as a whole.  One queue per concurrent caller (the events are re-recorded by
                           every call). */
  int32_t flags;        /* GEOA3_PN2_CONTRACT: the sampler's and the ball queries' distances contracted (see above); 0 = default */
} geoa3_pn2ssg_weights;
/* A HIP stream + five events owned by the caller's module object (the library keeps no global state).  Destroy after the
 * last call that used it has been enqueued (destroy synchronises the side stream). */
void* geoa3_side_queue_create(void);
void geoa3_side_queue_destroy(void* side);
/* The level-2 / level-3 matrices as split-fp16 fragment images (the order the matrix-core loops read them; one
 * power-of-two scale per matrix): built once per set of weights into `images` (geoa3_pn2ssg_images_bytes() bytes,
 * 256-byte aligned; the `images` member of *w is not read). */
int64_t geoa3_pn2ssg_images_bytes(void);
int geoa3_pn2ssg_pack_images(const geoa3_pn2ssg_weights* w, void* images, void* stream);
int64_t geoa3_pn2ssg_workspace_bytes(int B, int N);
int geoa3_pn2ssg_forward(const geoa3_pn2ssg_weights* w, const float* x, int B, int N, float* logits, void* workspace,
                         void* stream);
int geoa3_pn2ssg_backward(const geoa3_pn2ssg_weights* w, const float* x, const float* dlogits, int B, int N, float* dx,
                          void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense-cloud attack path, point-removal defence and smoothness measurement.
 * Two rules hold for every entry of this section ("NaN rule"):
 *   - a NaN input is a NaN in every output it feeds (the clamp of geoa3_perp_jitter and the maximum of
 *     geoa3_smoothness keep it; geoa3_sor_statistic gives NaN for a point with a non-finite coordinate and leaves
 *     that point out of every other point's neighbours; geoa3_sor_select mode 0 ranks -inf < finite < +inf < NaN,
 *     equal values by index, and keeps exactly N - drop_num);
 *   - a K-NN table entry outside [0,N) -- geoa3_knn pads with -1 when K > Nr -- is never dereferenced: a row that
 *     holds one, in any column, gives NaN in geoa3_local_frames (evals and evecs), geoa3_estimate_normal,
 *     geoa3_smoothness (per_point, and so out) and geoa3_knn_normal; every other row keeps its bits.
 * ------------------------------------------------------------------------------------------ */
/* farthest_points_sample, Lib/utility.py:175-187: m-1 rounds of dists = min(dists, |p - p_last|), next = first
 * arg-max.  start [B]: the index the reference draws with torch.randint (:179).  idx [B,m]; pts [B,3,m] (optional)
 * = pc gathered at idx.  N <= 16384. */
int geoa3_fps_sample(const float* pc, int B, int N, int m, const int32_t* start, int32_t* idx, float* pts,
                     void* stream);
/* estimate_normal_via_ori_normal, Lib/utility.py:91-108, from (knn_d, knn_i) = geoa3_knn(adv, ori, K) [B,Nq,K]:
 * out [B,3,Nq] = normal of the nearest original point when knn_d[..,0] < 1e-6, else the normalised mean of the K
 * gathered normals (evaluated per instance, as main_attack.py:244-246 calls it). */
int geoa3_knn_normal(const float* knn_d, const int32_t* knn_i, const float* normal_ori, int B, int Nq, int Nr, int K,
                     float* out, void* stream);
/* Local frames: eigen-decomposition of the covariance (factor 1/(k-1)) of the k = K1-1 nearest neighbours listed in
 * knn_idx [B,N,K1] (column 0, the point itself, dropped) -- Lib/utility.py:122-133,
 * Measurement/compute_data_smoothness.py:52-61.  evals [B,3,N] ascending; evecs [B,3(e),3(xyz),N], unit length,
 * largest-magnitude component positive. */
int geoa3_local_frames(const float* pc, const int32_t* knn_idx, int B, int N, int K1, float* evals, float* evecs,
                       void* stream);
/* estimate_normal, Lib/utility.py:40-89: normal_out [B,3,N] = the unit eigenvector of the smallest eigenvalue of the
 * covariance geoa3_local_frames forms from knn_idx [B,N,K1] (K1 >= 3, column 0 dropped) -- the same device code, the
 * same bits as its evecs[:,0].  orient 0: largest-magnitude component positive.  orient 1 ("outward"): the sign makes
 * n.(p_i - c) >= 0, c = the centroid of the cloud summed in a fixed order (no atomics); a dot product of exactly 0 keeps
 * the orient-0 sign.  The reference's own rule (:62-64, the sign of n.(sum of the mean-centred neighbours), a sum that is
 * zero up to rounding) is NOT mirrored.  A row that lists a point with a non-finite coordinate gives a NaN normal; under
 * orient 1 a non-finite coordinate anywhere in a cloud makes all of that cloud's normals NaN. */
int geoa3_estimate_normal(const float* pc, const int32_t* knn_idx, int B, int N, int K1, int orient, float* normal_out,
                          void* stream);
/* The tail of __farthest_points_normalized, Provider/modelnet10_instance250.py:120-124 (and of
 * Provider/gen_data_mat_sample_from10000.py:18-22): out [B,3,M] = (pts - mean over the M points) / largest point norm.
 * out may be pts (in place).  centroid_out [B,3] / scale_out [B] (optional): the mean subtracted and the norm divided
 * by.  One workgroup per cloud, fixed reduction order.  A cloud whose largest norm is 0 or not finite comes out NaN. */
int geoa3_normalize_cloud(const float* pts, float* out, int B, int M, float* centroid_out, float* scale_out,
                          void* stream);
/* estimate_perpendicular's tail, Lib/utility.py:146-149: out [B,3,N] = clamp(v_max*aux1, +-clip) +
 * clamp(v_mid*aux2, +-clip); aux1/aux2 [B,N] = sigma * N(0,1) drawn by the caller. */
int geoa3_perp_jitter(const float* evecs, const float* aux1, const float* aux2, int B, int N, float clip, float* out,
                      void* stream);
/* compute_data_smoothness.py:63-67: out[b] = max_i mean_{m=1..K1-1} |<p[knn_idx[b,i,m]] - p_i, n_i>| with n_i the
 * smallest-eigenvalue eigenvector from geoa3_local_frames; per_point [B,N] optional. */
int geoa3_smoothness(const float* pc, const int32_t* knn_idx, const float* evecs, int B, int N, int K1,
                     float* per_point, float* out, void* stream);
/* defense.py:27-28: dis [B,N] = mean distance to the K nearest neighbours, distances evaluated as
 * sqrt(sum_c (p_j - p_i + 1e-10)^2) like the reference. */
int geoa3_sor_statistic(const float* pc, int B, int N, int K, float* dis, void* stream);
/* defense.py:31-45: the kept indices of every cloud, ascending, idx [B,N] padded with -1, count [B].
 * mode 0 = outliers_fixNum (keep the N-drop_num smallest dis), 1 = outliers_variance (dis < mean + alpha*std);
 * stats [B,2] (optional) = (mean, std). */
int geoa3_sor_select(const float* dis, int B, int N, int mode, int drop_num, float alpha, int32_t* idx,
                     int32_t* count, float* stats, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh inputs: area-weighted surface sampling of a ragged batch of triangle meshes (Provider/gen_data_mat.py:88-119,
 * sample_points, which the reference defines and never calls).  Batch layout: verts f32 [total_verts,3]; faces i32
 * [total_faces,3], indices LOCAL to their mesh; vert_off / face_off i64 [B+1] on the device (mesh b owns
 * verts[vert_off[b] .. vert_off[b+1]) and faces[face_off[b] .. face_off[b+1])).  The sizes are stated again on the host:
 * total_verts, total_faces and max_faces = the largest face count of one mesh; the kernels clamp every offset to them.
 * Limits: max_faces <= 2^22, total_faces < 2^31 (GEOA3_ENOSUPPORT otherwise, nothing launched).
 * Rules: a face with an index outside [0,V_b) or a non-finite area is never dereferenced, weighs 0, is never selected and
 * is counted in bad_faces; a mesh of total weight 0 gives NaN points and normals and face_idx -1; so does a sample with a
 * NaN draw, alone.  Deterministic: integer sums only, repeated calls are bit-identical.
 * ------------------------------------------------------------------------------------------ */
/* Bytes of the table of geoa3_mesh_area_table (the prefix_sum of gen_data_mat.py:88-119): 8 * total_faces (GEOA3_ENOSUPPORT from 2^31 faces on). */
int64_t geoa3_mesh_table_bytes(int64_t total_faces);
/* gen_data_mat.py:88-119, its lines :92-95 (areas, np.cumsum) in exact integers: table u64 [total_faces] = per mesh the inclusive prefix
 * sum of w_f = rint(A_f / unit), restarting at every mesh; A_f = 0.5 |(b-a) x (c-a)| in double from the float32 vertices,
 * unit = 2^(e-40) with (m, e) = frexp(the mesh's largest A_f), so w_f <= 2^40 and a mesh's total stays below 2^62.
 * bad_faces i32 [B].  One workgroup per mesh, no atomics. */
int geoa3_mesh_area_table(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* face_off,
                          int B, int64_t total_verts, int64_t total_faces, int64_t max_faces, uint64_t* table,
                          int32_t* bad_faces, void* stream);
/* gen_data_mat.py:88-119, its loop :97-115 for S samples of every mesh, from the draws u f32 [B,S,3] in [0,1) the caller makes (:99,
 * :107-108): with T_b the mesh's last table entry, t = min(T_b - 1, (uint64)((double)u0 * (double)T_b)) and the face is
 * the first f with table[f] > t (bisect_right, :103); in float32 r1 = u1, r2 = u2, both replaced by 1 - r when
 * r1 + r2 >= 1, r3 = (1 - r1) - r2, p = (r1 a + r2 b) + r3 c, no contraction (:106-113); the normal is the unit vector of
 * (b-a) x (c-a) formed in double and rounded once, its sign the winding's.  pts, normals f32 [B,3,S] planar; face_idx
 * i32 [B,S], local to the mesh.  u0 carries 24 bits: a face below 2^-24 of its mesh's area is hit with a quantised
 * probability.  B <= 65535. */
int geoa3_mesh_sample(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* face_off,
                      const uint64_t* table, const float* u, int B, int S, int64_t total_verts, int64_t total_faces,
                      int64_t max_faces, float* pts, float* normals, int32_t* face_idx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh attack (main_attack.py:27-28, 283-293: --attack GeoA3_mesh, which the reference parses and never published; its
 * two weights name pytorch3d's mesh_laplacian_smoothing and mesh_edge_loss).  The vertices are held as the attack loop
 * holds every cloud: verts f32 [B,3,Vp] planar and padded, nv i32 [B] (V_b = nv[b] <= Vp; columns >= V_b are padding:
 * never read, their gradient written as 0).  Faces as above: faces i32 [total_faces,3] local, face_off i64 [B+1].
 * Topology: one CSR over the B Vp rows of the batch (row b Vp + v; padding rows empty): row_off i32 [B Vp + 1], col i32
 * [nnz] = the neighbours N(i) of the row's vertex, local and ASCENDING (every sum runs in that order), ne i32 [B] = the
 * number of undirected edges E_b.  Every device-side size is clamped to what the host states; an index outside its range
 * is not followed.  Limits: B <= 65535, B (Vp + 1) and 3 S below 2^31 - 256, total_faces < 2^31 (GEOA3_ENOSUPPORT,
 * nothing launched).  No float atomics: repeated calls are bit identical.  A NaN / inf vertex makes its own mesh's terms
 * and the points on its faces NaN and moves nothing else.
 * ------------------------------------------------------------------------------------------ */
/* pytorch3d.ops.sample_points_from_meshes at a FIXED draw (face_idx i32 [B,S], u f32 [B,S,3]: what geoa3_mesh_sample
 * returned and was given): pts f32 [B,3,S], p = (r1 a + r2 b) + r3 c with the weights of gen_data_mat.py:88-119 as
 * geoa3_mesh_sample forms them, float32, no contraction -- at the vertices the draw was made on, geoa3_mesh_sample's point
 * bit for bit.  face_idx outside [0,F_b) (-1: the sampler's "no face"), or a corner outside [0,V_b): a NaN point. */
int geoa3_mesh_points(const float* verts, const int32_t* nv, const int32_t* faces, const int64_t* face_off,
                      const int32_t* face_idx, const float* u, int B, int Vp, int S, int64_t total_faces, float* pts,
                      void* stream);
/* The pullback of geoa3_mesh_points (the backward of pytorch3d.ops.sample_points_from_meshes w.r.t. the vertices), three steps:
 * corner i32 [B,3S]: entry 3 s + k = the vertex of corner k of sample s, -1 for a sample without a point;
 * geoa3_mesh_points_lists sorts the entries by vertex into `scratch` (geoa3_mesh_points_scratch_bytes(B, Vp, S) bytes),
 * ONCE per draw; geoa3_mesh_points_grad: g_verts [B,3,Vp] = for every vertex the sum of w_k(s) g_pts[b,:,s] over its
 * entries in ascending (s, k), float32 products added sequentially from +0.0 (an empty list, the padding: +0.0). */
int geoa3_mesh_corner_index(const int32_t* nv, const int32_t* faces, const int64_t* face_off, const int32_t* face_idx,
                            int B, int Vp, int S, int64_t total_faces, int32_t* corner, void* stream);
int64_t geoa3_mesh_points_scratch_bytes(int B, int Vp, int S);
int geoa3_mesh_points_lists(const int32_t* corner, int B, int Vp, int S, void* scratch, void* stream);
int geoa3_mesh_points_grad(const float* g_pts, const float* u, const void* scratch, int B, int Vp, int S,
                           float* g_verts, void* stream);
/* pytorch3d.loss.mesh_laplacian_smoothing(method="uniform") and pytorch3d.loss.mesh_edge_loss, per mesh, one pass:
 *   delta_i = (sum_{j in N(i)} v_j) / deg_i - v_i (0 when deg_i = 0),  lap[b] = (1/V_b) sum_i |delta_i|  (0 when V_b = 0);
 *   edge[b] = (1/E_b) sum_{i<j} (l_ij - t_ij)^2  (0 when E_b = 0),  l_ij = |v_i - v_j| formed in double and rounded to
 *   float32 once, t_ij = target[q] of the CSR entry (target f32 [nnz]) or target_scalar when target is NULL.
 * unit f32 [B,4,Vp] <- (delta_i / |delta_i|, taken as 0 when |delta_i| = 0; |delta_i|): what geoa3_mesh_reg_grad reads.
 * Per-vertex terms in double, per-mesh sums reduced in double in a fixed order, rounded to float32 once.
 * constrain [B] (optional) = ((constrain_add ? constrain : 0) + w_lap lap) + w_edge edge; a term whose weight is 0 is left out. */
int geoa3_mesh_reg(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col, const int32_t* ne,
                   const float* target, float target_scalar, int B, int Vp, int nnz, float w_lap, float w_edge,
                   float* unit, float* lap, float* edge, float* constrain, int constrain_add, void* stream);
/* The gradients of pytorch3d.loss.mesh_laplacian_smoothing / mesh_edge_loss, one gather over N(i) (the adjacency is symmetric):
 *   g = w_lap g_lap[b] / V_b (-u_i [deg_i > 0] + sum_j u_j / deg_j) + w_edge g_edge[b] 2 / E_b sum_j (l_ij - t_ij)(v_i - v_j) / l_ij
 * (summand 0 when l_ij = 0; g_lap, g_edge f32 [B], NULL means ones; a term whose weight is 0 is skipped, not multiplied);
 * g_verts [B,3,Vp] = add ? g_verts + g : g, g rounded to float32 once; padding columns get g = 0. */
int geoa3_mesh_reg_grad(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col,
                        const int32_t* ne, const float* target, float target_scalar, const float* unit, const float* g_lap,
                        const float* g_edge, float w_lap, float w_edge, int B, int Vp, int nnz, float* g_verts, int add,
                        void* stream);
/* len f32 [nnz] = l_ij of every CSR entry as geoa3_mesh_reg forms it: the target_length of pytorch3d.loss.mesh_edge_loss
 * that makes the term and its gradient exactly 0 at the vertices it was taken on. */
int geoa3_mesh_edge_lengths(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col, int B,
                            int Vp, int nnz, float* len, void* stream);

/* ------------------------------------------------------------------------------------------
 * Uniformity term (Lib/loss_utils.py:151-189, uniform_loss; Attacker/geoA3_attack.py:168-174, --uniform_loss_weight).
 * ------------------------------------------------------------------------------------------ */
/* loss [1] = U, ONE scalar for the batch: for every p of percentages[num_percentages] (p <- 4p, nsample = int(N p),
 * r = sqrt(p radius), expect_len = float32(sqrt(float32(pi radius^2 p / nsample))), scale = (100 p)^2), the mean over all
 * B * npoint * nsample rows of (u - expect_len)^2 / (expect_len + 1e-12), u = the mean of sqrt(|d| + 1e-12) over the k
 * nearest other slots of the row's group (knn_points(g, g, k + 1), dists[:, :, 1:]), times scale; the sum over p divided
 * by num_percentages.  Groups: ball_query(r, nsample) around the npoint = int(N * 0.05) centres of
 * furthest_point_sample(pc, npoint) -- the bits of geoa3_pn2_furthest_point_sampling_ex / geoa3_pn2_ball_query_ex with
 * the same `flags` (GEOA3_PN2_CONTRACT).  pc [B,3,N] planar; grad [B,3,N] = dU / d pc (required).  fps_idx [B,npoint] and
 * group_idx (the ball-query rows of every p, one [B,npoint,nsample_p] block after the other) are optional outputs.
 * Supported: 1 <= num_percentages <= 8, 1 <= k <= 8, every nsample in k+1 .. 512, N <= 8192 (GEOA3_ENOSUPPORT
 * otherwise).  A non-finite coordinate makes U and its instance's gradient NaN.  Deterministic: repeated calls are bit
 * identical.  workspace: geoa3_uniform_loss_workspace_bytes(B, N) bytes. */
int64_t geoa3_uniform_loss_workspace_bytes(int B, int N);
int geoa3_uniform_loss(const float* pc, int B, int N, const double* percentages, int num_percentages, double radius,
                       int k, int flags, float* loss, float* grad, int32_t* fps_idx, int32_t* group_idx,
                       void* workspace, void* stream);
/* geoA3_attack.py:171,176-178 with constrain_loss += w * U: constrain [B] (optional) = (constrain_add ? constrain : 0)
 * + w * loss[0]; g [B,3,N] (optional) = (g_add ? g : 0) + w * (sum_b scale_const[b] / B) * grad -- the gradient of
 * mean_b(scale_const[b] * w * U), which couples the rows of the batch. */
int geoa3_uniform_fold(const float* loss, const float* grad, const float* scale_const, float w, int B, int N,
                       float* constrain, int constrain_add, float* g, int g_add, void* stream);

/* ------------------------------------------------------------------------------------------
 * Neighbour-based regularisers of Lib/loss_utils.py: functions of a self K-NN table, per row of the batch.
 * The table: (knn_d, knn_i) [B,N,knn_ld] as geoa3_knn_self(cloud, K >= k + 1) writes it (knn_ld = its K; 0 means k + 1;
 * the first k + 1 columns are used, column 0 is dropped as the reference's [:, :, 1:]), both given or both NULL.
 * NULL: the entry point runs geoa3_knn_self(cloud, k + 1) itself into `workspace` (geoa3_reg_workspace_bytes(B, N, k)
 * bytes, 256-byte aligned; also required for clouds of more than ~4200 points, whose gradient sums do not fit in LDS).
 * Every *_grad entry point writes grad [B,3,N] = d (sum g . out) / d cloud; g = NULL means ones.  Gradient sums are
 * order-free 64-bit fixed point at the instance's own scale: repeated calls are bit identical, and a row does not depend
 * on the rest of the batch.  Supported: 2 <= k + 1 <= GEOA3_KNN_MAX_K, k + 1 <= N <= 8192 (GEOA3_EINVAL /
 * GEOA3_ENOSUPPORT otherwise).  A non-finite coordinate makes every output of its instance NaN.
 * ------------------------------------------------------------------------------------------ */
int64_t geoa3_reg_workspace_bytes(int B, int N, int k);
/* kNN_smoothing_loss, Lib/loss_utils.py:135-149 (the outlier term of the kNN-attack baseline; both arguments of its
 * knn_points are adv_pc): s_i = mean_m d[i,m], thr = mean_i s + coef * std_i s (unbiased), cond[b,i] = s_i > thr
 * ([B,N] bytes, optional), loss[b] = (1/N) sum_i s_i cond_i.  Gradient (g [B]): cond carries none; every kept pair
 * (i, j) adds g_b / (N k) * 2 (x_i - x_j) to point i and subtracts it from point j. */
int geoa3_knn_smoothing_loss(const float* pc, int B, int N, int k, float coef, const float* knn_d, const int32_t* knn_i,
                             int knn_ld, float* loss, uint8_t* cond, void* workspace, void* stream);
int geoa3_knn_smoothing_loss_grad(const float* pc, int B, int N, int k, float coef, const float* knn_d,
                                  const int32_t* knn_i, int knn_ld, const float* g, float* grad, void* workspace,
                                  void* stream);
/* repulsion_loss, Lib/loss_utils.py:119-123: out[b,i] = -mean_m d exp(-d^2 / h^2), d the SQUARED distance, squared again
 * inside the exponent as the reference writes it.  Gradient (g [B,N]): pair coefficient
 * -(1/k) exp(-d^2/h^2) (1 - 2 d^2/h^2) g_i on 2 (x_i - x_j), d formed again in double from the cloud (the table gives the
 * neighbours; its float32 distances are the forward's). */
int geoa3_repulsion_loss(const float* pc, int B, int N, int k, float h, const float* knn_d, const int32_t* knn_i,
                         int knn_ld, float* out, void* workspace, void* stream);
int geoa3_repulsion_loss_grad(const float* pc, int B, int N, int k, float h, const float* knn_d, const int32_t* knn_i,
                              int knn_ld, const float* g, float* grad, void* workspace, void* stream);
/* displacement_loss, Lib/loss_utils.py:99-107: the table is taken on ORI and carries no gradient; theta_i =
 * |adv_i - ori_i|^2, out[b,i] = mean_m (theta_j - theta_i)^2.  Gradient (g [B,N]) w.r.t. adv only, through theta. */
int geoa3_displacement_loss(const float* adv, const float* ori, int B, int N, int k, const float* knn_d,
                            const int32_t* knn_i, int knn_ld, float* out, void* workspace, void* stream);
int geoa3_displacement_loss_grad(const float* adv, const float* ori, int B, int N, int k, const float* knn_d,
                                 const int32_t* knn_i, int knn_ld, const float* g, float* grad, void* workspace,
                                 void* stream);
/* corresponding_normal_loss, Lib/loss_utils.py:109-117: the forward is geoa3_knn_self + geoa3_kappa with nn_idx = NULL.
 * Gradient (g [B,N]; normal [B,3,N], read by index: point i, normal i) with the conventions of the *_grad entry points
 * above: pair (i, j) adds -g_i / k * sign(t) (n_i - t v^) / |v| to point i and subtracts it from point j, v = x_j - x_i,
 * v^ = v / max(|v|, 1e-12), t = <v^, n_i>, sign(0) = 0, every pair term formed in double.  (The dkappa path of
 * geoa3_geo_loss_grad with the identity as i_ao gives the same gradient from float32 pair terms.) */
int geoa3_corr_normal_loss_grad(const float* pc, const float* normal, int B, int N, int k, const float* knn_d,
                                const int32_t* knn_i, int knn_ld, const float* g, float* grad, void* workspace,
                                void* stream);
/* A per-row term S [B] with gradient dS [B,3,N] joins the attack's constrain loss (--is_use_knn_smoothing_loss):
 * constrain [B] (optional) = (constrain_add ? constrain : 0) + w * loss;  g [B,3,N] (optional) = (g_add ? g : 0) + w * grad. */
int geoa3_reg_fold(const float* loss, const float* grad, float w, int B, int N, float* constrain, int constrain_add,
                   float* g, int g_add, void* stream);
/* A per-point term out [B,N] joins the constrain loss through its row mean (Lib/loss_utils.py:95):
 *   term[b]      (optional) = mean_i out[b,i], accumulated in double in an order that depends on N only;
 *   constrain[b] (optional) = (constrain_add ? constrain[b] : 0) + w * term[b];
 *   g [B,3,N]    (optional) = (g_add ? g : 0) + (w / N) * grad,
 *                grad = d(sum_i out[b,i]) / d cloud, what the *_grad entry points write with g = NULL.
 * One launch, one workgroup per row: a row reads nothing outside itself, repeated calls are bit identical.  Sums and
 * products are formed in double and rounded to float once.  A row whose mean is NaN gets NaN in all of its g, whatever
 * grad holds.  out may be NULL when only g is wanted, grad when g is not (GEOA3_EINVAL when nothing is asked for). */
int geoa3_reg_fold_points(const float* out, const float* grad, float w, int B, int N, float* term, float* constrain,
                          int constrain_add, float* g, int g_add, void* stream);

/* ------------------------------------------------------------------------------------------
 * A 1024-wide PointNet layer in TRAINING mode: conv(128 -> 1024, taps 1 | 3, zero padding taps / 2) -> BatchNorm1d with
 * batch statistics -> [relu] -> max over points, without writing the [B,1024,N] activation.  Replaces
 * Model/PointNet.py:81-82 (transform_net: `F.relu(self.bn3(self.conv3(x)))`, `torch.max(x, 2, keepdim=True)[0]`) and
 * Model/PointNet.py:146-147 (`F.relu(self.bn5(self.conv5(x)))`, `torch.max(x, 2, keepdim=True)[0]`) under net.train().
 * X [B,128,N]; W [1024, taps*128] with k = tap*128 + ci; U[b,:,p] is the unfolded input column (zeros past the ends).
 * The conv bias is not an argument: BatchNorm removes it from the output and from every gradient (its gradient is zero).
 * Limits: B <= 65535, 2 <= B*N < 2^24 (GEOA3_EINVAL otherwise: B*N < 2 has no batch variance, as torch refuses it).
 * Sums are taken in an order that depends on (B, N) only: repeated calls give the same bits.
 * ------------------------------------------------------------------------------------------ */
int64_t geoa3_wide_train_workspace_bytes(int B, int N, int taps);
/* Forward.  shift [1024]: the caller's estimate of the mean of W U per channel (W mean(U) is exact up to rounding); the
 * variance is accumulated about it.  Writes, with a[b,c] the first maximum of y = W U over the points where gamma[c] > 0,
 * the first minimum where gamma[c] < 0, point 0 where gamma[c] == 0:
 *   arg [B,1024] = a,  xhat [B,1024] = (y[a] - mean) / sqrt(var + eps),  out = gamma xhat + beta, relu'd when `relu`,
 *   mean [1024] = mean of W U over all B*N positions (add the conv bias for BatchNorm's running_mean), var [1024] = the
 *   biased variance.  A non-finite activation makes mean, var and every out[:, c] / xhat[:, c] it enters NaN.
 * workspace: geoa3_wide_train_workspace_bytes(B, N, taps) bytes, 256-byte aligned. */
int geoa3_wide_train_forward(const float* X, const float* W, const float* shift, const float* gamma, const float* beta,
                             float eps, int relu, int B, int N, int taps, float* out, int32_t* arg, float* xhat,
                             float* mean, float* var, void* workspace, void* stream);
/* Backward of Model/PointNet.py:81-82 / :146-147, the term through the selected points:
 * dW [1024, taps*128] = sum_b coef[b,c] U[b,:,arg[b,c]], b ascending (coef [B,1024] = gated upstream gradient * gamma / sigma). */
int geoa3_wide_train_gather(const float* X, const float* coef, const int32_t* arg, int B, int N, int taps, float* dW,
                            void* stream);
/* ... and its input gradient: dX [B,128,N] (every element written) = sum over (c, tap) with arg[b,c] + tap - taps/2 == q
 * of coef[b,c] W[c, tap*128 + ci], in ascending (c, tap) order. */
int geoa3_wide_train_scatter(const float* W, const float* coef, const int32_t* arg, int B, int N, int taps, float* dX,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * The neighbour half of an EdgeConv layer (DGCNN) in TRAINING mode: max_k LeakyReLU_0.2(BatchNorm2d(W [x_j - x_i ; x_i])) with
 * batch statistics, without the [B,2C,N,K] edge tensor or any [B,C,N,K] tensor, forward or backward.  With W = [W_a | W_b]
 * the caller forms U0 = h W_a^T and V0 = h (W_b - W_a)^T ([B,N,C] point-major, unscaled); edge (i, s), j = idx[b,i,s], has the
 * pre-BatchNorm value z = U0[j] + V0[i], and M = B N K.
 * Limits: N K < 2^31 - 256, B <= 65535 (GEOA3_ENOSUPPORT otherwise); B N K >= 2 (GEOA3_EINVAL otherwise: one value has no
 * batch variance, as torch refuses it).  Nothing is written when an entry refuses.  No floating-point atomics: sums are
 * taken in an order that depends on the sizes and on idx only, repeated calls give the same bits.
 * ------------------------------------------------------------------------------------------ */
/* bytes of `workspace` below (the per-tile partial sums and the destination lists of idx), 256-byte aligned; < 0 when the
 * sizes are out of range */
int64_t geoa3_edge_train_workspace_bytes(int B, int N, int C, int K);
/* Forward.  gamma, beta [C], idx int64 [B,N,K] ->
 *   arg[b,i,c] (int32 [B,N,C]) = the first maximum of U0[b, idx[b,i,.], c] where gamma[c] > 0, the first minimum where
 *                gamma[c] < 0, slot 0 where gamma[c] == 0 (the float32 values are compared: ties go to the lower slot);
 *   S1[b,i,c]  ([B,N,C])       = sum_s U0[b, idx[b,i,s], c], the sequential float32 sum from +0.0;
 *   mean, var [C]              = the mean and the BIASED variance of z over the M edges, accumulated in double from the exact
 *                value of u + v in a fixed order, rounded once;  stats (double [3][C]) = mean | var | 1 / sqrt(var + eps),
 *                unrounded: what geoa3_edge_train_grad takes;
 *   y[b,c,i]   ([B,C,N])       = lrelu(gamma r (U0[b,idx[b,i,arg],c] + V0[b,i,c] - mean) + beta), lrelu(a) = a > 0 ? a : 0.2 a,
 *                formed in double, rounded once.
 * An index outside [0,N) is never dereferenced; it makes EVERY y, mean, var of the call NaN (arg: its first such slot).
 * A non-finite U0 / V0 value makes mean, var and y of its channel NaN. */
int geoa3_edge_train_forward(const float* U0, const float* V0, const int64_t* idx, const float* gamma, const float* beta,
                             float eps, int B, int N, int C, int K, float* y, int32_t* arg, float* S1, float* mean,
                             float* var, double* stats, void* workspace, void* stream);
/* Backward.  g, y [B,C,N]; U0, V0, arg, S1, idx, gamma, stats as above.  With g' = y > 0 ? g : fl(0.2f g) and
 * zhat = (z - mean) r:
 *   dbeta [C]  = sum_{b,i} g',   dgamma [C] = sum_{b,i} g' zhat_sel     (double partial sums in a fixed order, rounded once)
 *   dV0[b,i,c] = gamma r ( g' - K dbeta / M - (dgamma / M) r ( S1 + K V0 - K mean ) )
 *   dU0[b,j,c] = gamma r ( sum_{(i,s)->j, s == arg[i]} g'[i] - indeg(j) dbeta / M
 *                          - (dgamma / M) r ( indeg(j) (U0[j] - mean) + sum_{(i,s)->j} V0[i] ) )
 * where (i,s)->j runs over the entries of idx[b] equal to j, with multiplicity, in ascending (i, s) order; both sums are
 * sequential float32 sums from +0.0, the rest is formed in double and rounded once.  An index outside [0,N) gives no term.
 * dU0, dV0 [B,N,C], every element written. */
int geoa3_edge_train_grad(const float* g, const float* y, const float* U0, const float* V0, const int32_t* arg,
                          const float* S1, const int64_t* idx, const float* gamma, const double* stats, int B, int N, int C,
                          int K, float* dU0, float* dV0, float* dgamma, float* dbeta, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEOA3_HIP_H */
