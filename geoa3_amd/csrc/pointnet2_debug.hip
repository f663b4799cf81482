// Single kernels of the PointNet++ SSG native path in isolation (geoa3_hip_debug.h; tests/test_gpu_pn2_kernels.py): each
// entry checks what the host can check (pointers, sizes), fills the launcher's arguments the way geoa3_pn2ssg_forward does
// and returns the launcher's status -- nothing else.  No entry looks at device data: an index table (gidx) must hold
// indices inside its table.
#include "pointnet_kernels.h"

extern "C" int geoa3_debug_pn2_frag_image(const float* W, int R, int K, void* img, float* un, void* stream) {
  if (!W || !img || !un || R <= 0 || K <= 0 || R % 32 != 0 || K % 16 != 0) return GEOA3_EINVAL;
  return launch_frag_image(W, R, K, img, un, geoa3_stream(stream));
}

extern "C" int geoa3_debug_pn2_sa2_pre(const float* X, int x_channel_major, int Np, const float* xyz, const void* wf_img,
                                       const float* wf_un, const float* Wx, float* Y, int64_t P, void* stream) {
  if (!X || !wf_img || !wf_un || !Y || P <= 0 || P % 32 != 0 || (xyz && !Wx)) return GEOA3_EINVAL;
  if (x_channel_major && (Np <= 0 || Np % 32 != 0 || P % Np != 0)) return GEOA3_EINVAL;
  return launch_sa2_pre(X, x_channel_major != 0, Np, xyz, wf_img, wf_un, Wx, Y, (long)P, geoa3_stream(stream));
}

extern "C" int64_t geoa3_debug_pn2_sa2b_scratch_bytes(int B) { return B > 0 ? (int64_t)sa2b_scratch_bytes(B) : 0; }

// the level's backward in the order of geoa3_pn2ssg_backward: prep -> the pass -> d xyz1 = W_x^T dr -> d c -= the centres' share
extern "C" int geoa3_debug_pn2_sa2b(const float* dout, const float* out, const int32_t* arg, const int32_t* gidx, const void* m1,
                                    const void* m0, const float* W2, const void* w1t_img, const float* w1t_un, const float* Wx,
                                    void* scratch, float* dr, float* dnx1, float* dnx2, int B, void* stream) {
  if (!dout || !out || !arg || !gidx || !m1 || !m0 || !W2 || !w1t_img || !w1t_un || !Wx || !scratch || !dr || !dnx1 || !dnx2)
    return GEOA3_EINVAL;
  if (B <= 0 || ((uintptr_t)scratch & 255) != 0) return GEOA3_EINVAL;
  hipStream_t s = geoa3_stream(stream);
  int rc = launch_sa2b_prep(dout, out, arg, gidx, scratch, dr, B, s);
  if (rc != GEOA3_OK) return rc;
  rc = launch_sa2b_bwd(scratch, static_cast<const unsigned*>(m1), static_cast<const unsigned*>(m0), W2, w1t_img, w1t_un, Wx, dr,
                       B, s);
  if (rc != GEOA3_OK) return rc;
  rc = launch_affine3_grad_pm(dr, Wx, dnx1, (long)B * 512, s);
  if (rc != GEOA3_OK) return rc;
  return launch_sa2b_centre(scratch, dnx2, B, s);
}

extern "C" int geoa3_debug_pn2_sa2_fwd(const float* rT, const int32_t* gidx, const float* shift, const void* w1_img,
                                       const float* w1_un, const float* b1, const void* w2_img, const float* w2_un,
                                       const float* b2, float* out, int32_t* arg, void* m0, void* m1, int B, int N1, int M,
                                       void* stream) {
  if (!rT || !gidx || !shift || !w1_img || !w1_un || !b1 || !w2_img || !w2_un || !b2 || !out || !arg || !m0 || !m1)
    return GEOA3_EINVAL;
  if (B <= 0 || N1 <= 0 || M <= 0 || M % 8 != 0 || (int64_t)B * M > 0x3fffffffL) return GEOA3_EINVAL;
  return launch_sa2_fwd(rT, gidx, shift, w1_img, w1_un, b1, w2_img, w2_un, b2, out, arg, static_cast<unsigned*>(m0),
                        static_cast<unsigned*>(m1), B, N1, M, geoa3_stream(stream));
}
