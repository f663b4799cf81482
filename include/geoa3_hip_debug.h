/*
 * geoa3_hip_debug.h -- diagnostics of libgeoa3_hip.so, declared APART from the product ABI (geoa3_hip.h):
 * event timers around selected kernels (bench.py's `roofline` figures) and single-kernel entry points for the
 * tools/ micro-benchmarks and unit tests.  Nothing here is needed to run the attack loop, and nothing here
 * changes a result.  The event timer is the one piece of process-global state in the library (a table of
 * hipEvent_t, empty unless geoa3_profile_enable() is called); no entry point of geoa3_hip.h reads or writes any
 * other global.
 */
#ifndef GEOA3_HIP_DEBUG_H
#define GEOA3_HIP_DEBUG_H

#include <stdint.h>
#include "geoa3_hip.h" /* geoa3_geo_args */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Event timers (bench.py): per-launch durations of selected kernels, taken with HIP events recorded on the
 * launch stream.  Off by default; never changes results.
 * tag: 0 = conv5+max (wide_max_kernel<3>), 1 = geoa3_nn1_pair ("CD kernel"), 2 = geoa3_knn,
 *      3 = T-Net conv3+max (wide_max_kernel<1>), 4 / 5 = PointNet++ level 1 backward / forward (sa1_*_kernel),
 *      6 = the fully connected chains, 7 = geo_loss_grad_kernel, 8 / 9 = PointNet++ level 2 forward / backward
 *      (sa2_fwd8_kernel, sa2b_bwd_kernel), 10 = the backward's preparation pass (sa2b_prep_kernel).
 * ------------------------------------------------------------------------------------------ */
int geoa3_profile_enable(int capacity);                 /* events for `capacity` launches per tag; 0 = off */
int geoa3_profile_select(unsigned mask);                /* bit t set = tag t is recorded (default: all); an event
                                                           pair costs ~6 us of stream time around the kernel */
int geoa3_profile_read(int tag, float* ms_host, int cap); /* waits for the recorded launches; returns count */

/* ------------------------------------------------------------------------------------------
 * Single kernels of the PointNet path in isolation (tools/bench_*.py, tests/test_gpu_pointnet.py).
 * ------------------------------------------------------------------------------------------ */
/* The sparse arg-max backward of a 1024-wide layer (tools/bench_widebwd.py): g [B,1024], arg [B,1024],
 * W [1024, taps*128], Z / dX [B,128,N]. */
int geoa3_debug_wide_bwd(const float* g, const int32_t* arg, const float* W, const float* Z, float* dX, int B, int N,
                         int taps, void* stream);
/* One 1024-wide layer + max (tools/bench_wide.py): Wp = fp32 MFMA fragments; Wh = split-fp16 fragments in the layout the
 * library uses for this tap count (taps 1: pack_wide_split, taps 3: pack_wide_split16) or NULL. */
int geoa3_debug_wide_fwd(const float* X, const float* Wp, const void* Wh, float unscale, const float* bias, float* out,
                         int32_t* arg, void* keys, int B, int N, int taps, void* stamps, void* stream);
/* One fully connected layer Y[M,Nout] = relu?(X[M,K] W[Nout,K]^T + bias) (tools/bench_fc.py). */
int geoa3_debug_fc(const float* X, const float* W, const float* bias, float* Y, int M, int Nout, int K, int relu,
                   int ksplit, void* stream);
/* One channel-major 1x1 convolution Y[B,Co,N] = act(W[Co,K] X[B,K,N] + bias) (gated by Z > 0 when given) of the
 * PointNet trunk (K, Co in {64, 128}), for tools/bench_conv.py. */
int geoa3_debug_conv_cm(const float* X, const float* W, const float* bias, const float* Z, float* Y, int B, int N, int K,
                        int Co, int relu, int split /* 1: split-fp16 operands */, void* stream);

/* ------------------------------------------------------------------------------------------
 * The trunk kernels of geoa3_pointnet_forward one at a time (tests/test_gpu_pointnet_fwd.py).  Each entry fills the launch
 * arguments the way the forward does and starts the kernel.  A layer is Y [B,Co,N] = relu(W[b] h + bias), W [Co][K] with k
 * contiguous and sWb floats between the instances' matrices (0 = shared); its input h is X [B,K,N] or -- cloud form, K = 64,
 * x3 given and X NULL -- the folded first layer relu(w1 (T3^T x3) + b1) with x3 [B,3,N], T3 [B,9] (NULL = identity), w1
 * [64,3], b1 [64].  Ymask: the layer's gate bits (Y > 0), [B][ceil(N/64)][Co] 64-bit words as below; exactly these words are
 * written, and the bits of columns >= N in an instance's last word are unspecified.  The tests hold every stored value to
 * |got - ref| <= 4 sqrt(n) 2^-24 mag + 2^-22 |ref| of a float64 evaluation (n = the terms of the longest sum, mag = the sum
 * of the absolute products, the input's own bound carried through |W|), every gate bit to the float64 gate wherever the
 * pre-activation is farther from zero than that bound, and the bits of a stored activation to Y > 0 exactly.
 * ------------------------------------------------------------------------------------------ */
/* One launch of conv_chain_kernel (pointnet_conv_chain.hip): ns stages of 64 inputs, the last with 128 outputs, the others 64.
 * The forward's three forms are the ones that exist: cloud form with ns = 1 or 3, X form with ns = 2 (GEOA3_ENOSUPPORT
 * otherwise).  W, sWb, bias, Y, Ymask: host arrays of ns entries; Y[i] NULL = stage i leaves gate bits only.  With shared
 * weights every stage gives the bits of the geoa3_debug_conv_cm_ex launches (split = 1) it replaces. */
int geoa3_debug_conv_chain(const float* X, const float* x3, const float* T3, const float* w1, const float* b1, int ns,
                           const float* const* W, const int64_t* sWb, const float* const* bias, float* const* Y,
                           void* const* Ymask, int B, int N, void* stream);
/* geoa3_debug_conv_cm with the fields of the forward's launches: the cloud form (produce_first), per-instance weights, the
 * gate words (NULL = none).  K, Co in {64, 128}; split: 1 = split-fp16 operands (conv_cm64s_kernel), 0 = fp32 (conv_cm64_kernel). */
int geoa3_debug_conv_cm_ex(const float* X, const float* x3, const float* T3, const float* w1, const float* b1, int K, int Co,
                           const float* W, int64_t sWb, const float* bias, int relu, float* Y, void* Ymask, int split, int B,
                           int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * The kernels of geoa3_pointnet_backward one at a time (tests/test_gpu_pointnet_bwd.py).  Each entry fills the launch
 * arguments the way the backward does and starts the kernel(s); gate bit masks are [B][ceil(N/64)][C] 64-bit words, bit j
 * of word (w, row) = column 64 w + j (bits of columns >= N are ignored).
 *
 * Hit lists (hits [B][1024 taps], hoff [B][N + 1]; written by the forward's finalize pass into the workspace buffers
 * hl3 / ho3, hlq / hoq, hl5 / ho5).  An entry is (co * taps + tap) | (m << 16), filed under the column m = arg[co] + tap
 * - taps / 2 the tap's gradient lands on; a tap with m outside [0, N) has no entry.  Entries are sorted by column and,
 * inside a column, by (co / 64, tap, co); hoff[m] is the index of column m's first entry, hoff[N] the instance's entry
 * count (slots behind it are not written).  A channel whose pooled output is not positive (relu-dead: its upstream
 * gradient is zero) has no entries; a NaN output counts as live.  The backward expects g == 0 on every channel that is
 * not listed; a listed channel with g == 0 adds zeros but moves the waves' share boundaries, so the sums may be added
 * in another order than without the lists.
 * ------------------------------------------------------------------------------------------ */
/* The sparse arg-max backward of a 1024-wide layer and the gated 128 -> 64 layer behind it in one kernel
 * (pointnet_wide_bwdconv.hip): g [B,1024], arg [B,1024], W [1024, taps*128], Zmask = gate bits of the 128-channel
 * activation, W2t [64,128] with W2th = pack_wide_split(W2t) and w2th_unscale.  Either Zmask2 (gate bits of the 64-channel
 * activation) and dY [B,64,N] (written), or -- first-layer form, taps = 1 -- x3 [B,3,N], w1 [64,3], b1 [64] and dx3 [B,3,N]
 * (added into; Zmask2 / dY unused).  hits / hoff: both or neither (NULL: every workgroup builds its tile's lists from g /
 * arg). */
int geoa3_debug_wide_bwd_conv(const float* g, const int32_t* arg, const float* W, const void* Zmask, const float* W2t,
                              const void* W2th, float w2th_unscale, const void* Zmask2, float* dY, const float* x3,
                              const float* w1, const float* b1, float* dx3, const int32_t* hits, const int32_t* hoff, int B,
                              int N, int taps, void* stream);
/* P[b][i][o] = sum_n A[b][i][n] G[b][o][n], A and G [B,64,N], P [B,64,64] (pointnet_gram.hip).  scratch: B * parts * 4096
 * floats, parts = 8 / 4 / 1 from 8 / 4 / fewer 128-column chunks on; NULL = one part. */
int geoa3_debug_gram64(const float* A, const float* G, int B, int N, float* P, float* scratch, void* stream);
/* The backward of the trunk's front (conv_bwd_chain_kernel, then the fixed-order sum of its partial dT):
 * dh2 = gate(Wa[b]^T Xa + Wb^T Xb) with Xa, Xb [B,64,N], Wa [B][64 o][64 i] (sWa floats between instances; 0 = shared),
 * Wb [64 o][64 i], Zmask the gate bits of the 64 rows; g1 = gate_first(W2t dh2), W2t [64,64]; q = w1^T g1; dx [B,3,N] = T3 q
 * (T3 [B,9] or NULL = identity); dT [B,9]: dT[d][c] = sum_n x3[d][n] q[c][n].  gate_first = (w1 (T3^T x3) + b1 > 0).
 * dTpart: B * ceil(N/256) * 32 floats of scratch. */
int geoa3_debug_conv_bwd_chain(const float* Xa, const float* Wa, int64_t sWa, const float* Xb, const float* Wb,
                               const void* Zmask, const float* W2t, const float* x3, const float* T3, const float* w1,
                               const float* b1, float* dx, float* dTpart, float* dT, int B, int N, void* stream);
/* geoa3_debug_fc with every field of the launch: row pitches, the batch (instance strides sXb / sWb / sYb in floats; batch
 * 0 / 1 = none), Z [M, ldZ] (keep where Z > 0) and kscratch (ceil(Nout/16) * ceil(M/16) * 4096 floats: K >= 2048 on 16 x 16
 * tiles is split over four workgroups per tile).  ksplit as geoa3_debug_fc: (tile << 8) | waves. */
int geoa3_debug_fc_ex(const float* X, int ldX, int64_t sXb, const float* W, int ldW, int64_t sWb, const float* bias,
                      const float* Z, int ldZ, float* Y, int ldY, int64_t sYb, int M, int Nout, int K, int batch, int relu,
                      int ksplit, float* kscratch, void* stream);

/* geoa3_grid_nn1_pair (geoa3_hip.h) with its search policy given: brute_frac = the fraction of the searched cloud inside
 * the queries' boxes beyond which a workgroup searches all pairs (0 = always), filter = through the matrix-core filter
 * kernel (1) or the in-kernel sweep (0); negative values = the shipped choice.  Every policy returns the same bits. */
int geoa3_debug_grid_nn1_pair(const float* a, const float* r, int B, int Na, int Nr, const int32_t* prior_ar,
                              const int32_t* prior_ra, float* d_ar, int32_t* i_ar, float* d_ra, int32_t* i_ra,
                              float brute_frac, int filter, void* stream);

/* The search geoa3_knn_self (geoa3_hip.h) would run for these sizes, `method`, with / without a prior and a usable (non-NULL,
 * 256-byte aligned) scratch buffer: one of GEOA3_KNN_ROUTE_*, or GEOA3_EINVAL where geoa3_knn_self refuses the sizes.  No
 * GPU work.  Every route returns the same bits, so this is the one place the choice can be observed
 * (tests/test_knn_self_route.py). */
#define GEOA3_KNN_ROUTE_ALLPAIRS 0   /* geoa3_knn's kernel: nothing to prune with, N > 8192 or K > N */
#define GEOA3_KNN_ROUTE_CELLGRID 1   /* knn_cellsort_kernel + knn_grid_kernel */
#define GEOA3_KNN_ROUTE_SLAB40 2     /* slab_bin_kernel + knn_slab_kernel<40 / 72 / 96>: (distance, index) lists */
#define GEOA3_KNN_ROUTE_SLAB72 3
#define GEOA3_KNN_ROUTE_SLAB96 4
#define GEOA3_KNN_ROUTE_SLABP32 5    /* slab_bin_kernel + knn_slabp_kernel<32, false> / <56, true>: position lists */
#define GEOA3_KNN_ROUTE_SLABP56 6
int geoa3_debug_knn_self_route(int B, int N, int K, int method, int has_prior, int scratch_ok);

/* The kernel geoa3_geo_loss_grad (geoa3_hip.h) would run for these arguments: one of GEOA3_GEO_ROUTE_*, or GEOA3_EINVAL where
 * the call is refused as malformed.  Only the sizes, the flags and WHICH pointers are given are looked at: no GPU work, no
 * pointer is followed (tests/test_geo_route.py). */
#define GEOA3_GEO_ROUTE_FUSED 0     /* geo_fused_kernel: N <= 1024, reverse-list rows in LDS */
#define GEOA3_GEO_ROUTE_BIG 1       /* geo_big_kernel: N <= 4096 with scratch, fixed-point sums */
#define GEOA3_GEO_ROUTE_LISTS 2     /* geo_loss_grad_kernel<true>: one workgroup, chunked reverse lists */
#define GEOA3_GEO_ROUTE_ATOMICS 3   /* geo_loss_grad_kernel<false>: one workgroup, LDS float atomics */
#define GEOA3_GEO_ROUTE_WIDE 4      /* geo_wide_pair_kernel + geo_wide_sum_kernel: 5840 <= N <= 8192 with scratch */
#define GEOA3_GEO_ROUTE_REFUSED 5   /* geoa3_geo_loss_grad returns GEOA3_ENOSUPPORT */
int geoa3_debug_geo_route(const geoa3_geo_args* args);

/* Where reg_bwd_kernel (the gradients of geom_reg.hip) keeps the per-point fixed-point sums of a cloud of N points with k
 * neighbours: in LDS beside the cloud, or in the workspace (geoa3_reg_workspace_bytes then includes them).  mode: 0 =
 * kNN_smoothing_loss, 1 = repulsion_loss, 2 = displacement_loss, 3 = corresponding_normal_loss.  REFUSED where the entry
 * points refuse the sizes (or the mode is none of the four).  Both forms return the same bits.  No GPU work
 * (tests/test_reg_route.py). */
#define GEOA3_REG_ROUTE_LDS 0         /* reg_bwd_kernel<mode, true> */
#define GEOA3_REG_ROUTE_WORKSPACE 1   /* reg_bwd_kernel<mode, false> */
#define GEOA3_REG_ROUTE_REFUSED 2
int geoa3_debug_reg_route(int mode, int N, int k);

/* The same for uniform_main_kernel (geoa3_uniform_loss, geom_uniform.hip): LDS or WORKSPACE
 * (geoa3_uniform_loss_workspace_bytes then includes the sums), or the error code (negative) geoa3_uniform_loss returns for
 * these sizes.  percentages: P doubles on the host.  No GPU work. */
#define GEOA3_UNIFORM_ROUTE_LDS 0         /* uniform_main_kernel<*, *, true> */
#define GEOA3_UNIFORM_ROUTE_WORKSPACE 1   /* uniform_main_kernel<*, *, false> */
int geoa3_debug_uniform_route(int B, int N, const double* percentages, int P, double radius, int k);

/* The two-pass kernels behind GEOA3_GEO_ROUTE_WIDE on a cloud of any size from 64 to 8192 points (tests hold them to
 * geo_big_kernel bit for bit where both run).  ranges: owner ranges per instance, 1..16; 0 = the dispatcher's choice (the
 * fewest that fit LDS).  The gradient does not depend on it.  GEOA3_ENOSUPPORT when that many ranges do not fit LDS.
 * args->scratch: geoa3_debug_geo_wide_scratch_bytes(B, N) bytes (== geoa3_geo_scratch_bytes beyond 4096 points). */
int64_t geoa3_debug_geo_wide_scratch_bytes(int B, int N);
int geoa3_debug_geo_wide(const geoa3_geo_args* args, int ranges, void* stream);

/* Names and byte offsets (address order) of the buffers geoa3_pointnet_forward / _backward keep in their workspace:
 * tools/iteration_replay_soak.py attributes a run-to-run difference to the kernel that wrote it.  Returns the number
 * of buffers (names[i] are static strings). */
int geoa3_debug_pointnet_workspace_layout(int B, int N, int classes, const char** names, int64_t* offsets, int cap);

/* The launch sequence geoa3_pointnet_forward / _backward (geoa3_hip.h) would run for these weights and sizes, as a mask of
 * GEOA3_PN_ROUTE_* bits: the plan both entry points compute once per call and every stage reads.  Or GEOA3_EINVAL where both
 * refuse the arguments (w NULL, B or N not positive, t3.K != 3, t64.K != 64, classes <= 0).  Only the sizes, w->flags and WHICH
 * of w5h, w4th, t3.w2th, t64.w2th are given are looked at: no GPU work, no pointer is followed
 * (tests/test_pointnet_route.py).  Every route returns the same bits as the default one, except SPLIT against fp32. */
#define GEOA3_PN_ROUTE_SPLIT 1        /* w5h given: split-fp16 operands in every convolution; without it only bits 64 and 256 can be set */
#define GEOA3_PN_ROUTE_CHAIN 2        /* the trunk's 64-input layers as chain kernels (not GEOA3_PN_NO_CHAIN) */
#define GEOA3_PN_ROUTE_FUSE_TRUNK 4   /* sparse backward of conv5 + conv4's in one kernel (not GEOA3_PN_NO_FUSE_BWD; w4th given) */
#define GEOA3_PN_ROUTE_FUSE_T64 8     /* the same for the feature transform's conv3 + conv2 (t64.w2th given) */
#define GEOA3_PN_ROUTE_FUSE_T3 16     /* ... and the input transform's, with its first layer's backward (t3.w2th given) */
#define GEOA3_PN_ROUTE_PRE_LISTS 32   /* the forward builds the sparse backward's hit lists: fused backward allowed, N <= 4096,
                                         not GEOA3_PN_NO_PRE_LISTS */
#define GEOA3_PN_ROUTE_FC_KSPLIT 64   /* the T-Nets' backward lends G128 to the FC k-split: ceil(B/16)*16*4096 <= B*128*N */
#define GEOA3_PN_ROUTE_GRAM_F16 128   /* the backward's Gram product on the f16 matrix pipe (with SPLIT) */
#define GEOA3_PN_ROUTE_CLEAR_KEYS 256 /* the forward zeroes the arg-max keys (not GEOA3_PN_KEYS_CLEAN) */
int geoa3_debug_pointnet_route(const geoa3_pointnet_weights* w, int B, int N);

/* ------------------------------------------------------------------------------------------
 * The kernels of PointNet++ SSG's second level one at a time (tests/test_gpu_pn2_kernels.py).  Each entry fills the launch
 * arguments the way geoa3_pn2ssg_forward does and starts the kernel; GEOA3_EINVAL for a null pointer or a size outside the
 * kernel's contract.  No entry can look at device data: every index of gidx must lie in [0, N1).
 *
 * Fragment image of W [R][K] (R % 32 == 0, K % 16 == 0): un[0] = 2^(E - 140) with E = the biased exponent of max|W| clamped
 * to [14, 254] (the maximum times 1 / un lies in [2^13, 2^14)); img holds 2 R K fp16, the pieces hi = fp16(W / un) and
 * lo = fp16(W / un - hi) at [row >> 5][k >> 4][piece][32 ((k >> 3) & 1) + (row & 31)][k & 7].
 * ------------------------------------------------------------------------------------------ */
int geoa3_debug_pn2_frag_image(const float* W, int R, int K, void* img, float* un, void* stream);
/* Y [P][128] = X W_f^T (+ xyz W_x^T when xyz is given): X [P][128] point-major, or [P / Np][128][Np] when x_channel_major;
 * xyz [P][3], W_x [128][3]; wf_img / wf_un = the fragment image of W_f [128][128].  P (and Np) multiples of 32. */
int geoa3_debug_pn2_sa2_pre(const float* X, int x_channel_major, int Np, const float* xyz, const void* wf_img,
                            const float* wf_un, const float* Wx, float* Y, int64_t P, void* stream);
/* out [B][256][M] = relu(max_s W2 relu(W1 relu(rT[gidx] + shift) + b1) + b2), arg = the first maximal sample: rT [B][N1][128],
 * gidx [B][M][64], shift [B][128][M], the images of W1 [128][128] and W2 [256][128]; m0 / m1 [B * M][64][4] 32-bit words:
 * bit c of word w of a row (centre, sample) = channel 32 w + c of a0 / a1 is positive.  M a multiple of 8. */
int geoa3_debug_pn2_sa2_fwd(const float* rT, const int32_t* gidx, const float* shift, const void* w1_img, const float* w1_un,
                            const float* b1, const void* w2_img, const float* w2_un, const float* b2, float* out, int32_t* arg,
                            void* m0, void* m1, int B, int N1, int M, void* stream);
/* The level's backward in the order of geoa3_pn2ssg_backward: sa2b_prep_kernel, sa2b_bwd_kernel, affine3_grad_pm_kernel
 * (dnx1 = W_x^T dr), sa2b_centre_kernel (dnx2 -= the centres' share: dnx2 holds the caller's values on entry).  The sizes are
 * the classifier's: 128 centres, 64 samples, 512 points.  dout / out / arg [B][256][128], gidx [B][128][64] (indices in [0, 512);
 * arg in [0, 64) and below the ball's count of distinct points), m1 / m0 the forward's gate words, W2 [256][128], w1t_img /
 * w1t_un the fragment image of W1^T, Wx [128][3]; dr [B][512][128], dnx1 [B][512][3], dnx2 [B][128][3].
 * scratch: geoa3_debug_pn2_sa2b_scratch_bytes(B) bytes, 256-byte aligned; it stays readable afterwards.  Per cloud
 * (geoa3_debug_pn2_sa2b_scratch_bytes(1) bytes each), in this order, R = the cloud's hit rows (a row = (centre, sample) some
 * live pooled channel points at; live: out > 0 and dout != 0), in (destination point, centre) order:
 *   int32 [8192]   row keys: dest | sample << 9 | centre << 15 | last-of-dest << 31                        (R written)
 *   int32 [32768]  entries, row by row, ascending channel: channel | column << 16 | last-of-row << 31, column = the row's
 *                  position in its part, mod 64                                                            (the live channels)
 *   float [32768]  the entries' gradients
 *   int4  [132]    tiles of up to 64 rows: row0, rows, entry0, entries | (entries of rows 0-31) << 16
 *   int32 [8]      tile prefix of the 4 parts ([0..4] written); parts are cut where a destination starts: part q begins at
 *                  the first destination whose first row is at or behind floor(R q / 4)
 *   u64   [128]    bit s of word m = (centre m, sample s) is a hit row
 *   float [128][64][3]  W_x^T d a0 of each hit row, at [centre][sample]
 * rounded up to a multiple of 256 bytes. */
int64_t geoa3_debug_pn2_sa2b_scratch_bytes(int B);
int geoa3_debug_pn2_sa2b(const float* dout, const float* out, const int32_t* arg, const int32_t* gidx, const void* m1,
                         const void* m0, const float* W2, const void* w1t_img, const float* w1t_un, const float* Wx,
                         void* scratch, float* dr, float* dnx1, float* dnx2, int B, void* stream);
/* Level 1's backward needs no entry of its own: geoa3_pn2_sa1_backward (geoa3_hip.h) already takes out, arg and grad_out, and
 * with a scratch buffer (deterministic mode: N small enough for one instance's sums in LDS) it leaves dp [B][M][64][3] readable
 * in scratch afterwards -- the gradient of every (centroid, sample) difference, a ball's padded samples (repeats of its first
 * index) merged into sample 0 and zero themselves.  This entry is the second kernel of that mode alone (sa1_scatter_kernel):
 * dxyz [B][N][3] = the sum of dp over the (centroid, sample) whose idx [B][M][64] names the point, padded samples skipped, as
 * an order-free 64-bit fixed-point sum at 2^(Ex - 40), 2^Ex the power of two above the instance's largest finite |dp|
 * (Ex clamped to [-80, 80]); a NaN / infinite entry makes its destination NaN, an infinite maximum the whole instance.
 * Every index must lie in [0, N).  GEOA3_ENOSUPPORT when N is beyond what geoa3_pn2_sa1_backward takes in that mode. */
int geoa3_debug_pn2_sa1_scatter(const float* dp, const int32_t* idx, int B, int N, int M, float* dxyz, void* stream);
/* Names and byte offsets (address order) of the buffers geoa3_pn2ssg_forward / _backward keep in their workspace, one per
 * field of the workspace, then "end" = geoa3_pn2ssg_workspace_bytes(B, N).  Returns the number of names, -1 for sizes the
 * native path refuses.  Some buffers serve twice: the forward keeps rT (the pre-transformed rows) in `df1` and, with a side
 * queue, the sampler's running distances in `d1`; the backward writes dr over `r` and, with a side queue, the scattered
 * centroid gradient gx2 over `f1`. */
int geoa3_debug_pn2ssg_workspace_layout(int B, int N, const char** names, int64_t* offsets, int cap);

#ifdef __cplusplus
}
#endif
#endif /* GEOA3_HIP_DEBUG_H */
