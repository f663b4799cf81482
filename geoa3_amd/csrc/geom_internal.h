// Internal launchers of the exact searches, shared between geom_nn.hip (all pairs), geom_grid.hip and geom_filter.hip (1-NN),
// geom_slab.hip (self K-NN: slab search and routing) and geom_knn_grid.hip (self K-NN: cell grid).
#pragma once
#include "common.h"
// `only`: optional per-query byte flags ([ndir][B][max(Na,Nr)] for nn1, [B][Nq] for knn): search ONLY those queries
// (the fallback form for a pruned search; the shipped callers pass nullptr).
int geoa3_launch_nn1(const float* a, const float* r, int B, int Na, int Nr, float* d_ar, int32_t* i_ar, float* d_ra,
                     int32_t* i_ra, const uint8_t* only, hipStream_t s);
int geoa3_launch_knn(const float* q, const float* r, int B, int Nq, int Nr, int K, const int32_t* prior, float* dists,
                     int32_t* idx, const uint8_t* only, hipStream_t s);
// The cell-grid self K-NN (geom_knn_grid.hip; chosen by geoa3_knn_self, geom_slab.hip): N <= 8192, K <= min(N, GEOA3_KNN_MAX_K),
// prior [B,N,K] given, scratch 256-byte aligned and of geoa3_knn_cellgrid_scratch_bytes(B, N) bytes.
size_t geoa3_knn_cellgrid_scratch_bytes(int B, int N);
int geoa3_launch_knn_cellgrid(const float* pc, int B, int N, int K, const int32_t* prior, float* dists, int32_t* idx,
                              void* scratch, hipStream_t s);
// Grid-accelerated exact K=1 search (geom_grid.hip); GEOA3_ENOSUPPORT when a cloud exceeds 4096 points.
int geoa3_launch_grid_nn1(const float* a, const float* r, int B, int Na, int Nr, const int32_t* prior_ar,
                          const int32_t* prior_ra, float* d_ar, int32_t* i_ar, float* d_ra, int32_t* i_ra, hipStream_t s);
// The matrix-core filter + exact refinement as a kernel of its own (geom_filter.hip; the search itself: geom_filter.h):
// every query of every instance, clouds of any size.
int geoa3_launch_nn1_filter(const float* a, const float* r, int B, int Na, int Nr, const int32_t* prior_ar,
                            const int32_t* prior_ra, float* d_ar, int32_t* i_ar, float* d_ra, int32_t* i_ra, hipStream_t s);
// The geometric objective for clouds too large for one workgroup's LDS (geom_loss_wide.hip; chosen by geoa3_geo_loss_grad,
// geom_loss.hip): 64 <= N <= GEO_WIDE_MAX_N, scratch of geo_wide_scratch_bytes(B, N) bytes.  `ranges`: owner ranges per
// instance (geo_wide_ranges(N): the fewest that fit LDS, 0 = none does); GEOA3_ENOSUPPORT when that many do not fit.
constexpr int GEO_WIDE_MAX_N = 8192;
size_t geo_wide_scratch_bytes(int B, int N);
int geo_wide_ranges(int N);
int geo_wide_launch(const geoa3_geo_args* a, int ranges, hipStream_t s);
