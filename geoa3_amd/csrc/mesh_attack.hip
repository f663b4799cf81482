// The mesh attack's own kernels (gfx950): the map from the vertices of a batch of triangle meshes to points on their surfaces
// with its pullback, and the two mesh regularisers with their gradients.  They stand in for what the reference announces
// and never published (main_attack.py:27-28, 85-88, 283-293: --attack GeoA3_mesh, --laplacian_loss_weight,
// --edge_loss_weight): pytorch3d's sample_points_from_meshes at a FIXED draw, mesh_laplacian_smoothing(method="uniform")
// and mesh_edge_loss.
//
// Batch layout: the vertices as the attack loop holds every cloud, planar and padded, verts f32 [B,3,Vp] with nv i32 [B]
// (V_b = nv[b] <= Vp; columns >= V_b are padding: never read through a face or an edge, their gradient is written as 0);
// the faces as PackedMeshes holds them, faces i32 [total_faces,3] local to their mesh and face_off i64 [B+1].
// The topology is one CSR over the B Vp rows of the batch (row b Vp + v, padding rows empty): row_off i32 [B Vp + 1],
// col i32 [nnz] = the neighbours of the row's vertex, local, ASCENDING, and ne i32 [B] = the number of undirected edges.
//
// The file's rules:
//   * the point is the sampler's (mesh_sample.hip:208-217): the same float32 operations in the same grouping, no
//     contraction (-ffp-contract=off, build.py), so at the clean vertices it equals geoa3_mesh_sample's point bit for bit;
//   * the pullback adds float32 products sequentially, from +0.0, in ascending (sample, corner) order through the
//     destination lists of dest_lists.h: no float atomics, a float32 loop on the CPU gives the same bits;
//   * the regularisers form every per-vertex quantity in DOUBLE from the float32 vertices, summing over N(i) in the CSR's
//     order; a length l_ij is rounded to float32 once, so that a target taken from geoa3_mesh_edge_lengths at the clean
//     vertices cancels exactly and the edge term and its gradient are 0 at offset 0.  The per-mesh sums are reduced in
//     double in a FIXED order (one workgroup per mesh, every thread its vertices ascending, then a fixed tree over the
//     256 partials): the same bits on every run, and an error of (V/256 + 8) 2^-53 of the sum of magnitudes, nothing
//     beside the one float32 rounding of the result;
//   * every device-side size is clamped to what the host states (nv to Vp, face_off to total_faces, row_off to nnz); an
//     index outside its range -- a face index outside [0,F_b), a corner or a neighbour outside [0,V_b) -- is not followed:
//     the sample is NaN and in no list, the CSR entry adds nothing;
//   * no index is derived from a coordinate: a NaN / inf vertex makes its own mesh's terms NaN (a sum that is not finite
//     is written as NaN) and the points on its faces NaN, and moves nothing else.
#include "dest_lists.h"

namespace {

constexpr int MA_T = 256;   // threads per workgroup of the per-sample and per-vertex kernels
constexpr int MR_T = 256;   // mesh_reg: threads of the one workgroup per mesh
constexpr int MA_MAX_GRID_Y = 65535;
constexpr int64_t MA_MAX_TOTAL_FACES = (int64_t)1 << 31;

__device__ __forceinline__ float ma_nan() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ bool ma_finite(double x) {
  return ((unsigned long long)__double_as_longlong(x) & 0x7fffffffffffffffull) < 0x7ff0000000000000ull;
}
__device__ __forceinline__ int64_t ma_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ int ma_nv(const int32_t* __restrict__ nv, int b, int Vp) { return (int)ma_clamp(nv[b], 0, Vp); }

// The face of sample (b, s): its three corners, ok only when the face index lies in [0,F_b) and every corner in [0,V_b).
struct MaFace {
  bool ok;
  int32_t i[3];
};
__device__ __forceinline__ MaFace ma_face(const int32_t* __restrict__ nv, const int32_t* __restrict__ faces,
                                          const int64_t* __restrict__ face_off, const int32_t* __restrict__ face_idx, int b,
                                          int s, int Vp, int S, int64_t total_faces) {
  MaFace f;
  const int64_t f0 = ma_clamp(face_off[b], 0, total_faces);
  const int64_t nf = ma_clamp(face_off[b + 1], f0, total_faces) - f0;
  const unsigned nvb = (unsigned)ma_nv(nv, b, Vp);
  const int32_t fi = face_idx[(size_t)b * S + s];
  f.ok = (uint64_t)(int64_t)fi < (uint64_t)nf;
  f.i[0] = f.i[1] = f.i[2] = -1;
  if (f.ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      f.i[k] = faces[3 * (f0 + fi) + k];
      f.ok = f.ok && (unsigned)f.i[k] < nvb;
    }
  }
  return f;
}

// mesh_sample.hip:208-213: the barycentric weights of a draw (u1, u2), float32.
__device__ __forceinline__ void ma_weights(float u1, float u2, float w[3]) {
  float r1 = u1, r2 = u2;
  if (r1 + r2 >= 1.0f) {
    r1 = 1.0f - r1;
    r2 = 1.0f - r2;
  }
  w[0] = r1;
  w[1] = r2;
  w[2] = (1.0f - r1) - r2;
}

// ------------------------------------------------------------------------------------------
// mesh_points: one thread per sample, planar coalesced stores.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MA_T) void mesh_points_kernel(const float* __restrict__ verts, const int32_t* __restrict__ nv,
                                                           const int32_t* __restrict__ faces,
                                                           const int64_t* __restrict__ face_off,
                                                           const int32_t* __restrict__ face_idx, const float* __restrict__ u,
                                                           int Vp, int S, int64_t total_faces, float* __restrict__ pts) {
  const int b = blockIdx.y;
  const int s = blockIdx.x * MA_T + threadIdx.x;
  if (s >= S) return;
  const MaFace f = ma_face(nv, faces, face_off, face_idx, b, s, Vp, S, total_faces);
  float p[3] = {ma_nan(), ma_nan(), ma_nan()};
  if (f.ok) {
    const float* us = u + ((size_t)b * S + s) * 3;
    float w[3];
    ma_weights(us[1], us[2], w);
    const float* V = verts + (size_t)b * 3 * Vp;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float a = V[(size_t)k * Vp + f.i[0]], bb = V[(size_t)k * Vp + f.i[1]], c = V[(size_t)k * Vp + f.i[2]];
      p[k] = (w[0] * a + w[1] * bb) + w[2] * c;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) pts[((size_t)b * 3 + k) * S + s] = p[k];
}

// mesh_corner_index: corner [B][3S], entry 3 s + k = the vertex of corner k of sample s, -1 for a sample that has no face.
__global__ __launch_bounds__(MA_T) void mesh_corner_index_kernel(const int32_t* __restrict__ nv,
                                                                 const int32_t* __restrict__ faces,
                                                                 const int64_t* __restrict__ face_off,
                                                                 const int32_t* __restrict__ face_idx, int Vp, int S,
                                                                 int64_t total_faces, int32_t* __restrict__ corner) {
  const int b = blockIdx.y;
  const int s = blockIdx.x * MA_T + threadIdx.x;
  if (s >= S) return;
  const MaFace f = ma_face(nv, faces, face_off, face_idx, b, s, Vp, S, total_faces);
  int32_t* C = corner + ((size_t)b * S + s) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) C[k] = f.ok ? f.i[k] : -1;
}

// mesh_points_grad: one thread per vertex walks its list (ascending entry e = 3 s + k): acc = acc + w_k(s) * g[:, s].
__global__ __launch_bounds__(MA_T) void mesh_points_grad_kernel(const float* __restrict__ g_pts, const float* __restrict__ u,
                                                                const int* __restrict__ start, const int* __restrict__ order,
                                                                int Vp, int S, int BV, float* __restrict__ g_verts) {
  const int d = blockIdx.x * MA_T + threadIdx.x;
  if (d >= BV) return;
  const int b = d / Vp, v = d - b * Vp;
  const int* St = start + (size_t)b * (Vp + 1);
  const int s0 = St[v], s1 = St[v + 1];
  const int* O = order + (size_t)b * 3 * S;
  const float* G = g_pts + (size_t)b * 3 * S;
  const float* U = u + (size_t)b * S * 3;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int q = s0; q < s1; ++q) {
    const int e = O[q];
    const int s = e / 3, k = e - 3 * s;
    float w[3];
    ma_weights(U[(size_t)s * 3 + 1], U[(size_t)s * 3 + 2], w);
    const float wk = k == 0 ? w[0] : (k == 1 ? w[1] : w[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + wk * G[(size_t)c * S + s];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) g_verts[((size_t)b * 3 + c) * Vp + v] = acc[c];
}

// ------------------------------------------------------------------------------------------
// The regularisers.  A row of the CSR, clamped; a length, formed in double and rounded to float32 once.
// ------------------------------------------------------------------------------------------
struct MaRow {
  int q0, q1;
};
__device__ __forceinline__ MaRow ma_row(const int32_t* __restrict__ row_off, size_t row, int nnz) {
  MaRow r;
  r.q0 = (int)ma_clamp(row_off[row], 0, nnz);
  r.q1 = (int)ma_clamp(row_off[row + 1], r.q0, nnz);
  return r;
}
__device__ __forceinline__ double ma_len(const double xi[3], const double xj[3]) {
  const double dx = xi[0] - xj[0], dy = xi[1] - xj[1], dz = xi[2] - xj[2];
  return (double)(float)sqrt((dx * dx + dy * dy) + dz * dz);
}
__device__ __forceinline__ void ma_vertex(const float* __restrict__ V, int Vp, int v, double x[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = (double)V[(size_t)c * Vp + v];
}

// mesh_reg: one workgroup per mesh.  unit [B,4,Vp] <- (u_i, |delta_i|), 0 in the padding; lap / edge [B]; constrain [B]
// (optional) = ((constrain_add ? constrain : 0) + w_lap lap) + w_edge edge in float32, a term whose weight is 0 left out.
__global__ __launch_bounds__(MR_T) void mesh_reg_kernel(const float* __restrict__ verts, const int32_t* __restrict__ nv,
                                                        const int32_t* __restrict__ row_off, const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ ne, const float* __restrict__ target,
                                                        float target_scalar, int Vp, int nnz, float w_lap, float w_edge,
                                                        float* __restrict__ unit, float* __restrict__ lap,
                                                        float* __restrict__ edge, float* __restrict__ constrain, int constrain_add) {
  __shared__ double s_l[MR_T], s_e[MR_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nvb = ma_nv(nv, b, Vp);
  const float* V = verts + (size_t)b * 3 * Vp;
  float* Un = unit + (size_t)b * 4 * Vp;
  double lsum = 0.0, esum = 0.0;
  for (int v = tid; v < Vp; v += MR_T) {
    double un[4] = {0.0, 0.0, 0.0, 0.0};
    if (v < nvb) {
      const MaRow r = ma_row(row_off, (size_t)b * Vp + v, nnz);
      double xi[3], sum[3] = {0.0, 0.0, 0.0};
      ma_vertex(V, Vp, v, xi);
      for (int q = r.q0; q < r.q1; ++q) {
        const int j = col[q];
        if ((unsigned)j >= (unsigned)nvb) continue;
        double xj[3];
        ma_vertex(V, Vp, j, xj);
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += xj[c];
        if (j > v) {   // every undirected edge once, at its smaller end
          const double dl = ma_len(xi, xj) - (double)(target ? target[q] : target_scalar);
          esum += dl * dl;
        }
      }
      const int deg = r.q1 - r.q0;
      if (deg > 0) {
        double dlt[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) dlt[c] = sum[c] / (double)deg - xi[c];
        const double n = sqrt((dlt[0] * dlt[0] + dlt[1] * dlt[1]) + dlt[2] * dlt[2]);
        lsum += n;
        un[3] = n;
#pragma unroll
        for (int c = 0; c < 3; ++c) un[c] = n == 0.0 ? 0.0 : dlt[c] / n;   // (a NaN norm divides: NaN, not 0)
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) Un[(size_t)c * Vp + v] = (float)un[c];
  }
  s_l[tid] = lsum;
  s_e[tid] = esum;
  __syncthreads();
#pragma unroll
  for (int off = MR_T / 2; off > 0; off >>= 1) {
    if (tid < off) {
      s_l[tid] += s_l[tid + off];
      s_e[tid] += s_e[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int neb = ne[b] > 0 ? ne[b] : 0;
    // (an inf vertex sums to inf: a mesh with a non-finite vertex is NaN, as loud as the rest of the package)
    const float L = nvb > 0 ? (ma_finite(s_l[0]) ? (float)(s_l[0] / (double)nvb) : ma_nan()) : 0.f;
    const float E = neb > 0 ? (ma_finite(s_e[0]) ? (float)(s_e[0] / (double)neb) : ma_nan()) : 0.f;
    lap[b] = L;
    edge[b] = E;
    if (constrain) {
      float c = constrain_add ? constrain[b] : 0.f;
      if (w_lap != 0.f) c = c + w_lap * L;
      if (w_edge != 0.f) c = c + w_edge * E;
      constrain[b] = c;
    }
  }
}

// mesh_reg_grad: one thread per vertex, one pass over its row for both terms (the Laplacian's first).
//   g = w_lap g_lap[b] / V_b (-u_i [deg_i > 0] + sum_j u_j / deg_j)  +  w_edge g_edge[b] 2 / E_b sum_j (l_ij - t_ij)(v_i - v_j) / l_ij
// formed in double, rounded to float32 once, then g_verts = add ? g_verts + g : g.
__global__ __launch_bounds__(MA_T) void mesh_reg_grad_kernel(const float* __restrict__ verts, const int32_t* __restrict__ nv,
                                                             const int32_t* __restrict__ row_off,
                                                             const int32_t* __restrict__ col, const int32_t* __restrict__ ne,
                                                             const float* __restrict__ target, float target_scalar,
                                                             const float* __restrict__ unit, const float* __restrict__ g_lap,
                                                             const float* __restrict__ g_edge, float w_lap, float w_edge,
                                                             int Vp, int nnz, int BV, float* __restrict__ g_verts, int add) {
  const int d = blockIdx.x * MA_T + threadIdx.x;
  if (d >= BV) return;
  const int b = d / Vp, v = d - b * Vp;
  const int nvb = ma_nv(nv, b, Vp);
  const int neb = ne[b] > 0 ? ne[b] : 0;
  const bool do_lap = w_lap != 0.f, do_edge = w_edge != 0.f && neb > 0;
  double g[3] = {0.0, 0.0, 0.0};
  if (v < nvb) {
    const float* V = verts + (size_t)b * 3 * Vp;
    const float* Un = unit + (size_t)b * 4 * Vp;
    const MaRow r = ma_row(row_off, (size_t)d, nnz);
    double xi[3], a[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
    ma_vertex(V, Vp, v, xi);
    if (do_lap && r.q1 > r.q0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c] = -(double)Un[(size_t)c * Vp + v];
    }
    for (int q = r.q0; q < r.q1; ++q) {
      const int j = col[q];
      if ((unsigned)j >= (unsigned)nvb) continue;
      if (do_lap) {
        const MaRow rj = ma_row(row_off, (size_t)b * Vp + j, nnz);
        const int dj = rj.q1 - rj.q0;
        if (dj > 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a[c] += (double)Un[(size_t)c * Vp + j] / (double)dj;
        }
      }
      if (do_edge) {
        double xj[3];
        ma_vertex(V, Vp, j, xj);
        const double l = ma_len(xi, xj);
        if (l != 0.0) {   // (a NaN length is not 0: it is added)
          const double coef = (l - (double)(target ? target[q] : target_scalar)) / l;
#pragma unroll
          for (int c = 0; c < 3; ++c) e[c] += coef * (xi[c] - xj[c]);
        }
      }
    }
    if (do_lap) {
      const double cl = (double)w_lap * (g_lap ? (double)g_lap[b] : 1.0) / (double)nvb;
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] = cl * a[c];
    }
    if (do_edge) {
      const double ce = (double)w_edge * (g_edge ? (double)g_edge[b] : 1.0) * 2.0 / (double)neb;
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] += ce * e[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* out = g_verts + ((size_t)b * 3 + c) * Vp + v;
    const float gc = (float)g[c];
    *out = add ? *out + gc : gc;
  }
}

// mesh_edge_lengths: len [nnz] = l_ij of every CSR entry, the float32 the two kernels above work with (NaN for an entry
// whose neighbour lies outside [0,V_b)); one thread per vertex.
__global__ __launch_bounds__(MA_T) void mesh_edge_lengths_kernel(const float* __restrict__ verts, const int32_t* __restrict__ nv,
                                                                 const int32_t* __restrict__ row_off,
                                                                 const int32_t* __restrict__ col, int Vp, int nnz, int BV,
                                                                 float* __restrict__ len) {
  const int d = blockIdx.x * MA_T + threadIdx.x;
  if (d >= BV) return;
  const int b = d / Vp, v = d - b * Vp;
  const int nvb = ma_nv(nv, b, Vp);
  if (v >= nvb) return;
  const float* V = verts + (size_t)b * 3 * Vp;
  const MaRow r = ma_row(row_off, (size_t)d, nnz);
  double xi[3];
  ma_vertex(V, Vp, v, xi);
  for (int q = r.q0; q < r.q1; ++q) {
    const int j = col[q];
    float l = ma_nan();
    if ((unsigned)j < (unsigned)nvb) {
      double xj[3];
      ma_vertex(V, Vp, j, xj);
      l = (float)ma_len(xi, xj);
    }
    len[q] = l;
  }
}

// Sizes every entry accepts: B meshes of Vp padded vertices; B Vp + 1 rows and 3 S entries stay inside an int.
int ma_check_sizes(int B, int Vp) {
  if (B < 1 || Vp < 1) return GEOA3_EINVAL;
  if (B > MA_MAX_GRID_Y || (int64_t)B * ((int64_t)Vp + 1) > (int64_t)INT_MAX - 256) return GEOA3_ENOSUPPORT;
  return GEOA3_OK;
}
int ma_check_samples(int B, int Vp, int S, int64_t total_faces) {
  const int rc = ma_check_sizes(B, Vp);
  if (rc != GEOA3_OK) return rc;
  if (S < 1 || total_faces < 0) return GEOA3_EINVAL;
  if ((int64_t)S * 3 > (int64_t)INT_MAX - 256 || total_faces >= MA_MAX_TOTAL_FACES) return GEOA3_ENOSUPPORT;
  return GEOA3_OK;
}
int ma_check_csr(int B, int Vp, int nnz) {
  const int rc = ma_check_sizes(B, Vp);
  if (rc != GEOA3_OK) return rc;
  return nnz < 0 ? GEOA3_EINVAL : GEOA3_OK;
}

// the tables of launch_dest_lists inside `scratch` (dest_lists.h: start [B][M+1] | cursor [B][M] | bucket [B][E] | order [B][E])
void ma_lists(void* scratch, int B, int E, int M, const int** start, const int** order) {
  const int* s = static_cast<const int*>(scratch);
  *start = s;
  *order = s + (size_t)B * (M + 1) + (size_t)B * M + (size_t)B * E;
}

}  // namespace

extern "C" int geoa3_mesh_points(const float* verts, const int32_t* nv, const int32_t* faces, const int64_t* face_off,
                                 const int32_t* face_idx, const float* u, int B, int Vp, int S, int64_t total_faces,
                                 float* pts, void* stream) {
  const int rc = ma_check_samples(B, Vp, S, total_faces);
  if (rc != GEOA3_OK) return rc;
  if (!verts || !nv || !face_off || !face_idx || !u || !pts || (total_faces > 0 && !faces)) return GEOA3_EINVAL;
  hipLaunchKernelGGL(mesh_points_kernel, dim3((S + MA_T - 1) / MA_T, B), dim3(MA_T), 0, geoa3_stream(stream), verts, nv,
                     faces, face_off, face_idx, u, Vp, S, total_faces, pts);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_mesh_corner_index(const int32_t* nv, const int32_t* faces, const int64_t* face_off,
                                       const int32_t* face_idx, int B, int Vp, int S, int64_t total_faces, int32_t* corner,
                                       void* stream) {
  const int rc = ma_check_samples(B, Vp, S, total_faces);
  if (rc != GEOA3_OK) return rc;
  if (!nv || !face_off || !face_idx || !corner || (total_faces > 0 && !faces)) return GEOA3_EINVAL;
  hipLaunchKernelGGL(mesh_corner_index_kernel, dim3((S + MA_T - 1) / MA_T, B), dim3(MA_T), 0, geoa3_stream(stream), nv,
                     faces, face_off, face_idx, Vp, S, total_faces, corner);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int64_t geoa3_mesh_points_scratch_bytes(int B, int Vp, int S) {
  const int rc = ma_check_samples(B, Vp, S, 0);
  if (rc != GEOA3_OK) return rc;
  return (int64_t)dest_lists_scratch_bytes(B, 3 * S, Vp);
}

extern "C" int geoa3_mesh_points_lists(const int32_t* corner, int B, int Vp, int S, void* scratch, void* stream) {
  const int rc = ma_check_samples(B, Vp, S, 0);
  if (rc != GEOA3_OK) return rc;
  if (!corner || !scratch) return GEOA3_EINVAL;
  const int *start = nullptr, *order = nullptr, *start_at = nullptr, *order_at = nullptr;
  ma_lists(scratch, B, 3 * S, Vp, &start_at, &order_at);
  const int rb = launch_dest_lists<int32_t>(corner, B, 3 * S, Vp, scratch, geoa3_stream(stream), &start, &order);
  if (rb != GEOA3_OK) return rb;
  GEOA3_CHECK_LAUNCH();
  return (start == start_at && order == order_at) ? GEOA3_OK : GEOA3_ELAUNCH;   // (the layout ma_lists restates)
}

extern "C" int geoa3_mesh_points_grad(const float* g_pts, const float* u, const void* scratch, int B, int Vp, int S,
                                      float* g_verts, void* stream) {
  const int rc = ma_check_samples(B, Vp, S, 0);
  if (rc != GEOA3_OK) return rc;
  if (!g_pts || !u || !scratch || !g_verts) return GEOA3_EINVAL;
  const int *start = nullptr, *order = nullptr;
  ma_lists(const_cast<void*>(scratch), B, 3 * S, Vp, &start, &order);
  const int BV = B * Vp;
  hipLaunchKernelGGL(mesh_points_grad_kernel, dim3((BV + MA_T - 1) / MA_T), dim3(MA_T), 0, geoa3_stream(stream), g_pts, u,
                     start, order, Vp, S, BV, g_verts);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_mesh_reg(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col,
                              const int32_t* ne, const float* target, float target_scalar, int B, int Vp, int nnz,
                              float w_lap, float w_edge, float* unit, float* lap, float* edge, float* constrain,
                              int constrain_add, void* stream) {
  const int rc = ma_check_csr(B, Vp, nnz);
  if (rc != GEOA3_OK) return rc;
  if (!verts || !nv || !row_off || !ne || !unit || !lap || !edge || (nnz > 0 && !col)) return GEOA3_EINVAL;
  hipLaunchKernelGGL(mesh_reg_kernel, dim3(B), dim3(MR_T), 0, geoa3_stream(stream), verts, nv, row_off, col, ne, target,
                     target_scalar, Vp, nnz, w_lap, w_edge, unit, lap, edge, constrain, constrain_add);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_mesh_reg_grad(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col,
                                   const int32_t* ne, const float* target, float target_scalar, const float* unit,
                                   const float* g_lap, const float* g_edge, float w_lap, float w_edge, int B, int Vp, int nnz,
                                   float* g_verts, int add, void* stream) {
  const int rc = ma_check_csr(B, Vp, nnz);
  if (rc != GEOA3_OK) return rc;
  if (!verts || !nv || !row_off || !ne || !g_verts || (nnz > 0 && !col) || (w_lap != 0.f && !unit)) return GEOA3_EINVAL;
  const int BV = B * Vp;
  hipLaunchKernelGGL(mesh_reg_grad_kernel, dim3((BV + MA_T - 1) / MA_T), dim3(MA_T), 0, geoa3_stream(stream), verts, nv,
                     row_off, col, ne, target, target_scalar, unit, g_lap, g_edge, w_lap, w_edge, Vp, nnz, BV, g_verts, add);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}

extern "C" int geoa3_mesh_edge_lengths(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col,
                                       int B, int Vp, int nnz, float* len, void* stream) {
  const int rc = ma_check_csr(B, Vp, nnz);
  if (rc != GEOA3_OK) return rc;
  if (!verts || !nv || !row_off || (nnz > 0 && (!col || !len))) return GEOA3_EINVAL;
  if (nnz == 0) return GEOA3_OK;
  const int BV = B * Vp;
  hipLaunchKernelGGL(mesh_edge_lengths_kernel, dim3((BV + MA_T - 1) / MA_T), dim3(MA_T), 0, geoa3_stream(stream), verts, nv,
                     row_off, col, Vp, nnz, BV, len);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
}
