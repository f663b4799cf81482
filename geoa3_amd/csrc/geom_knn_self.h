// What the two pruned self K-NN searches (geom_slab.hip: slab, geom_knn_grid.hip: cell grid) share: both counting-sort the
// cloud first and keep the sorted cloud in the caller's scratch buffer.
#pragma once
#include "common.h"

constexpr float S_INF = __builtin_inff();

// The scratch buffer of either search: the sorted coordinates [B][3][N], the points' original indices [B][N], a table of
// run starts (`pitch` ints per instance: bins or cells) and a record per instance (geo_bytes each) the sort kernel
// leaves for the search kernel.  Every part starts on a 256-byte boundary.  base == nullptr: the size only.
struct KnnSelfScratch {
  float* sorted;
  int32_t* sidx;
  int32_t* start;
  void* geo;
  size_t total;
};
inline KnnSelfScratch knn_self_carve(void* base, int B, int N, int pitch, size_t geo_bytes) {
  KnnSelfScratch s{};
  size_t off = 0;
  char* p = static_cast<char*>(base);
  auto take = [&](size_t bytes) {
    void* r = p ? p + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return r;
  };
  s.sorted = (float*)take((size_t)B * 3 * N * 4);
  s.sidx = (int32_t*)take((size_t)B * N * 4);
  s.start = (int32_t*)take((size_t)B * pitch * 4);
  s.geo = take((size_t)B * geo_bytes);
  s.total = off;
  return s;
}
