// Area-weighted surface sampling of triangle meshes (gfx950): the join of Provider/gen_data_mat.py:88-119
// (sample_points -- an area-weighted triangle pick, a uniform barycentric point and the face's normal, one Python loop
// round per sample) with the mesh readers of Lib/utility.py:229-452, for a RAGGED batch of meshes in two kernels.
//
// Batch layout: verts f32 [sumV,3], faces i32 [sumF,3] with indices LOCAL to their mesh, vert_off / face_off i64 [B+1].
//
// The file's rules:
//   * exact integer sums.  A face's weight is its area in units of 2^(e-40), (m, e) = frexp(the mesh's largest area),
//     rounded to the nearest integer: w <= 2^40, and with at most 2^22 faces per mesh every prefix stays below 2^62.
//     Integer sums have no order, so the table is the same bits on every run whatever the shape of the scan;
//   * a face with an index outside [0,V_b), or whose area is not finite (a NaN / inf vertex), is never dereferenced
//     beyond its three indices, weighs 0, can never be selected and is counted in bad_faces[b]; a face of area 0 weighs
//     0 too and is not counted;
//   * a mesh whose total weight is 0 (no faces, or only degenerate / bad ones) gives NaN points, NaN normals and
//     face_idx = -1; a NaN anywhere in a sample's three draws gives the same for that sample alone.  Every other mesh
//     and sample keeps its bits;
//   * the offsets are device data: every range is clamped to the sizes the caller states on the host, so that a wrong
//     offset reads nothing outside the arrays.
// The file is compiled without contraction (-ffp-contract=off, build.py): the float32 point and the float64 area and
// normal are the chains of single operations the numpy restatement (tests/_mesh_ref.py) evaluates.
//
// The pick draws from u0, a float32 with 24 bits: a face smaller than 2^-24 of its mesh's area is hit with a quantised
// probability (some such faces never).  At the 1e4 samples per mesh this feeds that is far below the sampling noise.
#include "common.h"

namespace {

constexpr int MT_T = 1024;                 // table: threads per mesh = faces per scan chunk
constexpr int MT_W = MT_T / GEOA3_WAVE;
constexpr int MS_T = 256;                  // sampler: samples per workgroup
constexpr int64_t MESH_MAX_FACES = (int64_t)1 << 22;
constexpr int64_t MESH_MAX_TOTAL = (int64_t)1 << 31;

__device__ __forceinline__ float mesh_nan() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ bool mesh_is_nan(float x) { return (geoa3_opaque_bits(x) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool mesh_finite(double x) {
  return ((unsigned long long)__double_as_longlong(x) & 0x7fffffffffffffffull) < 0x7ff0000000000000ull;
}
__device__ __forceinline__ int64_t mesh_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The mesh's slice of the two arrays, clamped to what the caller says they hold.
struct MeshRange {
  int64_t v0, nv, f0, nf;
};
__device__ __forceinline__ MeshRange mesh_range(const int64_t* vert_off, const int64_t* face_off, int b,
                                                int64_t total_verts, int64_t total_faces) {
  MeshRange r;
  r.v0 = mesh_clamp(vert_off[b], 0, total_verts);
  r.nv = mesh_clamp(vert_off[b + 1], r.v0, total_verts) - r.v0;
  r.f0 = mesh_clamp(face_off[b], 0, total_faces);
  r.nf = mesh_clamp(face_off[b + 1], r.f0, total_faces) - r.f0;
  return r;
}

// (b-a) x (c-a) in double from the float32 vertices of face f; false when an index lies outside [0,nv) (nothing read).
__device__ __forceinline__ bool face_cross(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t f,
                                           int64_t v0, int64_t nv, double n[3], float a[3], float b[3], float c[3]) {
  const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  if ((uint64_t)(int64_t)ia >= (uint64_t)nv || (uint64_t)(int64_t)ib >= (uint64_t)nv || (uint64_t)(int64_t)ic >= (uint64_t)nv)
    return false;
  const float* pa = verts + 3 * (v0 + ia);
  const float* pb = verts + 3 * (v0 + ib);
  const float* pc = verts + 3 * (v0 + ic);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = pa[k];
    b[k] = pb[k];
    c[k] = pc[k];
  }
  const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
  const double vx = (double)c[0] - (double)a[0], vy = (double)c[1] - (double)a[1], vz = (double)c[2] - (double)a[2];
  n[0] = uy * vz - uz * vy;
  n[1] = uz * vx - ux * vz;
  n[2] = ux * vy - uy * vx;
  return true;
}
__device__ __forceinline__ double cross_norm(const double n[3]) { return sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]); }

// Area of face f, 0 for a bad face (bad raised).
__device__ __forceinline__ double face_area(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t f,
                                            int64_t v0, int64_t nv, bool& bad) {
  double n[3];
  float a[3], b[3], c[3];
  if (!face_cross(verts, faces, f, v0, nv, n, a, b, c)) {
    bad = true;
    return 0.0;
  }
  const double area = 0.5 * cross_norm(n);
  if (!mesh_finite(area)) {
    bad = true;
    return 0.0;
  }
  return area;
}

// ------------------------------------------------------------------------------------------
// The area table: one workgroup per mesh.  Pass 1: the largest area (areas are >= 0, so their bit patterns order like
// integers) and the number of bad faces.  Pass 2: the faces in chunks of MT_T, weight = rint(area * 2^(40-e)), an
// inclusive scan per wavefront, the wavefront totals through LDS, and the prefix carried from chunk to chunk.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_T) void mesh_area_table_kernel(const float* __restrict__ verts,
                                                               const int32_t* __restrict__ faces,
                                                               const int64_t* __restrict__ vert_off,
                                                               const int64_t* __restrict__ face_off, int64_t total_verts,
                                                               int64_t total_faces, uint64_t* __restrict__ table,
                                                               int32_t* __restrict__ bad_faces) {
  __shared__ unsigned long long s_max[MT_W], s_tot[MT_W];
  __shared__ int s_bad[MT_W];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const MeshRange r = mesh_range(vert_off, face_off, b, total_verts, total_faces);

  unsigned long long amax = 0;
  int nbad = 0;
  for (int64_t i = tid; i < r.nf; i += MT_T) {
    bool bad = false;
    const double area = face_area(verts, faces, r.f0 + i, r.v0, r.nv, bad);
    const unsigned long long bits = (unsigned long long)__double_as_longlong(area);
    amax = bits > amax ? bits : amax;
    nbad += bad ? 1 : 0;
  }
  amax = wave_max_u64(amax);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off);
  if (lane == 0) {
    s_max[wave] = amax;
    s_bad[wave] = nbad;
  }
  __syncthreads();
  amax = 0;
  nbad = 0;
#pragma unroll
  for (int w = 0; w < MT_W; ++w) {
    amax = s_max[w] > amax ? s_max[w] : amax;
    nbad += s_bad[w];
  }
  if (tid == 0) bad_faces[b] = nbad;
  int e = 0;
  (void)frexp(__longlong_as_double((long long)amax), &e);
  const int shift = 40 - e;   // 1 / unit = 2^shift

  unsigned long long carry = 0;
  for (int64_t base = 0; base < r.nf; base += MT_T) {
    const int64_t i = base + tid;
    unsigned long long w = 0;
    if (i < r.nf) {
      bool bad = false;
      const double area = face_area(verts, faces, r.f0 + i, r.v0, r.nv, bad);
      w = (unsigned long long)rint(ldexp(area, shift));
    }
#pragma unroll
    for (int off = 1; off < GEOA3_WAVE; off <<= 1) {
      const unsigned long long o = __shfl_up(w, off);
      if (lane >= off) w += o;
    }
    if (lane == GEOA3_WAVE - 1) s_tot[wave] = w;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < MT_W; ++k) {
      const unsigned long long t = s_tot[k];
      before += k < wave ? t : 0ull;
      all += t;
    }
    if (i < r.nf) table[r.f0 + i] = carry + before + w;
    carry += all;
    __syncthreads();   // s_tot is rewritten by the next chunk
  }
}

// ------------------------------------------------------------------------------------------
// The sampler: one thread per sample.  t = min(T-1, (uint64)(u0 * T)) in double, the face is the first one whose prefix
// exceeds t (bisect_right, gen_data_mat.py:103; a face of weight 0 repeats its predecessor's prefix and is never the
// first), the point is the reference's barycentric form in float32 (:106-113), the normal the unit cross product in
// double rounded once.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_T) void mesh_sample_kernel(const float* __restrict__ verts,
                                                           const int32_t* __restrict__ faces,
                                                           const int64_t* __restrict__ vert_off,
                                                           const int64_t* __restrict__ face_off,
                                                           const uint64_t* __restrict__ table,
                                                           const float* __restrict__ u, int S, int64_t total_verts,
                                                           int64_t total_faces, float* __restrict__ pts,
                                                           float* __restrict__ normals, int32_t* __restrict__ face_idx) {
  const int b = blockIdx.y;
  const int s = blockIdx.x * MS_T + threadIdx.x;
  if (s >= S) return;
  const MeshRange r = mesh_range(vert_off, face_off, b, total_verts, total_faces);
  const uint64_t T = r.nf > 0 ? table[r.f0 + r.nf - 1] : 0;
  const float* us = u + ((size_t)b * S + s) * 3;
  const float u0 = us[0], u1 = us[1], u2 = us[2];

  float p[3] = {mesh_nan(), mesh_nan(), mesh_nan()}, nf[3] = {mesh_nan(), mesh_nan(), mesh_nan()};
  int32_t fi = -1;
  if (T != 0 && !mesh_is_nan(u0) && !mesh_is_nan(u1) && !mesh_is_nan(u2)) {
    const double x = (double)u0 * (double)T;
    uint64_t t = x >= 18446744073709551616.0 ? T - 1 : (x > 0.0 ? (uint64_t)x : 0);
    t = t < T - 1 ? t : T - 1;
    int64_t lo = 0, hi = r.nf - 1;   // table[f0 + hi] = T > t: the answer lies in [lo, hi]
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (table[r.f0 + mid] > t) hi = mid; else lo = mid + 1;
    }
    double n[3];
    float a[3], bb[3], c[3];
    // (a table that is not this mesh's own may point at a bad face: it is not dereferenced either)
    if (face_cross(verts, faces, r.f0 + lo, r.v0, r.nv, n, a, bb, c)) {
      fi = (int32_t)lo;
      float r1 = u1, r2 = u2;
      if (r1 + r2 >= 1.0f) {
        r1 = 1.0f - r1;
        r2 = 1.0f - r2;
      }
      const float r3 = (1.0f - r1) - r2;
      const double len = cross_norm(n);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        p[k] = (r1 * a[k] + r2 * bb[k]) + r3 * c[k];
        nf[k] = (float)(n[k] / len);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pts[((size_t)b * 3 + k) * S + s] = p[k];
    normals[((size_t)b * 3 + k) * S + s] = nf[k];
  }
  face_idx[(size_t)b * S + s] = fi;
}

int mesh_check_sizes(int B, int64_t total_verts, int64_t total_faces, int64_t max_faces) {
  if (B < 1 || total_verts < 0 || total_faces < 0 || max_faces < 0 || max_faces > total_faces) return GEOA3_EINVAL;
  if (max_faces > MESH_MAX_FACES || total_faces >= MESH_MAX_TOTAL) return GEOA3_ENOSUPPORT;
  return GEOA3_OK;
}

}  // namespace

extern "C" int64_t geoa3_mesh_table_bytes(int64_t total_faces) {
  if (total_faces < 0) return GEOA3_EINVAL;
  if (total_faces >= MESH_MAX_TOTAL) return GEOA3_ENOSUPPORT;
  return total_faces * (int64_t)sizeof(uint64_t);
}

extern "C" int geoa3_mesh_area_table(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                     const int64_t* face_off, int B, int64_t total_verts, int64_t total_faces,
                                     int64_t max_faces, uint64_t* table, int32_t* bad_faces, void* stream) {
  const int rc = mesh_check_sizes(B, total_verts, total_faces, max_faces);
  if (rc != GEOA3_OK) return rc;
  if (!vert_off || !face_off || !bad_faces) return GEOA3_EINVAL;
  if (total_faces > 0 && (!verts || !faces || !table)) return GEOA3_EINVAL;
  hipLaunchKernelGGL(mesh_area_table_kernel, dim3(B), dim3(MT_T), 0, geoa3_stream(stream), verts, faces, vert_off,
                     face_off, total_verts, total_faces, table, bad_faces);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_mesh_sample(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                 const int64_t* face_off, const uint64_t* table, const float* u, int B, int S,
                                 int64_t total_verts, int64_t total_faces, int64_t max_faces, float* pts, float* normals,
                                 int32_t* face_idx, void* stream) {
  const int rc = mesh_check_sizes(B, total_verts, total_faces, max_faces);
  if (rc != GEOA3_OK) return rc;
  if (S < 1) return GEOA3_EINVAL;
  if (B > 65535) return GEOA3_ENOSUPPORT;
  if (!vert_off || !face_off || !u || !pts || !normals || !face_idx) return GEOA3_EINVAL;
  if (total_faces > 0 && (!verts || !faces || !table)) return GEOA3_EINVAL;
  hipLaunchKernelGGL(mesh_sample_kernel, dim3((S + MS_T - 1) / MS_T, B), dim3(MS_T), 0, geoa3_stream(stream), verts,
                     faces, vert_off, face_off, table, u, S, total_verts, total_faces, pts, normals, face_idx);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
