// PointNet eval forward and input-gradient: launch sequence over the kernels of pointnet_*.hip.
// Reference: Model/PointNet.py:56-94 (transform_net) and :96-160 (PointNet.forward); the backward is the
// hand-derived input-gradient of that graph (weights never receive gradients; the reference's autograd
// also forms the unused weight gradients, Attacker/geoA3_attack.py:326).
//
// Which kernels a call runs is decided ONCE, by pn_plan(), from the weights struct and the sizes; both entry points are
// sequences of named stages that read the plan (geoa3_debug_pointnet_route returns it; tests/test_pointnet_route.py).
#include <cstdlib>
#include "pointnet_host.h"

namespace {

// The workspace, one line per buffer: type, name, elements (b = B, s64 / s128 = B * 64 / 128 * N, n64 = ceil(N / 64)).
#define PN_WS(X)                                                                                                          \
  /* T-Net 3 (input transform); keys [B][1024]: packed running maxima of the 1024-wide layers (reused by all three) */    \
  X(float, a2, s128)                                                                                                      \
  X(unsigned long long, keys, b * 1024)                                                                                   \
  X(float, p3, b * 1024)                                                                                                  \
  X(int, i3, b * 1024)                                                                                                    \
  X(float, tf4, b * 512)                                                                                                  \
  X(float, tf5, b * 256)                                                                                                  \
  X(float, T3, b * 9)                                                                                                     \
  /* trunk + T-Net 64 (feature transform); W3eff [B][64][64] = W3 T64^T */                                                \
  X(float, h2, s64)                                                                                                       \
  X(float, c1, s64)                                                                                                       \
  X(float, c2, s128)                                                                                                      \
  X(float, q3, b * 1024)                                                                                                  \
  X(int, iq3, b * 1024)                                                                                                   \
  X(float, qf4, b * 512)                                                                                                  \
  X(float, qf5, b * 256)                                                                                                  \
  X(float, T64, b * 4096)                                                                                                 \
  X(float, W3eff, b * 4096)                                                                                               \
  X(float, h3, s64)                                                                                                       \
  X(float, h4, s128)                                                                                                      \
  X(float, p5, b * 1024)                                                                                                  \
  X(int, i5, b * 1024)                                                                                                    \
  X(float, f6, b * 512)                                                                                                   \
  X(float, f7, b * 256)                                                                                                   \
  /* backward temporaries; P64 [B][64][64] = h2 G64a^T.  Two serve twice: G128 is the FC k-split's scratch in the T-Nets' \
     backward, dh2 holds the Gram kernel's partial sums and then (chain form) the T-Net branch's gradient */              \
  X(float, G128, s128)                                                                                                    \
  X(float, G64a, s64)                                                                                                     \
  X(float, P64, b * 4096)                                                                                                 \
  X(float, dh2, s64)                                                                                                      \
  X(float, g1024, b * 1024)                                                                                               \
  X(float, g512, b * 512)                                                                                                 \
  X(float, g256, b * 256)                                                                                                 \
  X(float, gT64, b * 4096)                                                                                                \
  X(float, gT3, b * 16)                                                                                                   \
  X(float, dTpart, b * GEOA3_DT_PITCH * (size_t)((N + 255) / 256))                                                        \
  /* relu gates of the stored activations as bit masks [B][ceil(N/64)][C] x 64 bit (ConvArgs::Ymask / Zmask) */           \
  X(unsigned long long, m_a2, b * 128 * n64)                                                                              \
  X(unsigned long long, m_h2, b * 64 * n64)                                                                               \
  X(unsigned long long, m_c1, b * 64 * n64)                                                                               \
  X(unsigned long long, m_c2, b * 128 * n64)                                                                              \
  X(unsigned long long, m_h3, b * 64 * n64)                                                                               \
  X(unsigned long long, m_h4, b * 128 * n64)                                                                              \
  /* the sparse backward's hit lists, built by the forward's finalize passes (WideArgs::hits / hoff): lists [B][1024      \
     taps], column offsets [B][N + 1] -- T-Net 3, T-Net 64, conv5 */                                                      \
  X(int, hl3, b * 1024)                                                                                                   \
  X(int, ho3, b * ((size_t)N + 1))                                                                                        \
  X(int, hlq, b * 1024)                                                                                                   \
  X(int, hoq, b * ((size_t)N + 1))                                                                                        \
  X(int, hl5, b * 3072)                                                                                                   \
  X(int, ho5, b * ((size_t)N + 1))

struct Ws {
  PN_WS(GEOA3_WS_MEMBER)
  size_t total;
};

Ws carve(void* base, int B, int N) {
  Ws w{};
  size_t off = 0;
  char* p = static_cast<char*>(base);
  const size_t s64 = (size_t)B * 64 * N, s128 = (size_t)B * 128 * N, b = (size_t)B, n64 = (size_t)(N + 63) / 64;
  PN_WS(GEOA3_WS_TAKE)
  w.total = off;
  return w;
}

// What a call runs, decided once per entry point from the weights struct and the sizes (pointers are tested against NULL
// only; the library reads no environment).  Every form returns the same bits as the default one, except `split`: the
// callers that hand over split wide-layer fragments (w5h) get the whole network on the f16 matrix pipe, the others fp32
// MFMA throughout.  flags: geoa3_pointnet_weights.flags, the caller's A/B switches (include/geoa3_hip.h).
struct PnPlan {
  bool split;        // split-fp16 operands in every convolution
  bool chain;        // the trunk's 64-input layers as chain kernels, not one kernel each (GEOA3_PN_NO_CHAIN)
  // the sparse backward of a 1024-wide layer and the 128 -> 64 layer behind it in one kernel (GEOA3_PN_NO_FUSE_BWD; needs
  // that layer's transposed fragments): conv5 + conv4, T-Net 64, T-Net 3
  bool fuse_trunk, fuse_t64, fuse_t3;
  bool pre_lists;    // the forward's finalize passes build the sparse backward's hit lists (GEOA3_PN_NO_PRE_LISTS: every
                     // backward workgroup builds its own)
  bool fc_ksplit;    // the T-Nets' backward lends G128 to the FC kernel's k-split (K = 4096 for the feature transform: four
                     // workgroups per tile): its B * 128 * N floats hold the ceil(B / 16) * 16 tiles x 4096 partial values
  bool gram_f16;     // the backward's Gram product on the f16 matrix pipe (pointnet_gram.hip), not the FC kernel
  bool clear_keys;   // the forward zeroes the arg-max keys itself (GEOA3_PN_KEYS_CLEAN: the caller vouches they are)
};

PnPlan pn_plan(const geoa3_pointnet_weights& p, int B, int N) {
  PnPlan pl{};
  pl.split = p.w5h != nullptr;
  pl.chain = pl.split && !(p.flags & GEOA3_PN_NO_CHAIN);
  const bool fuse = pl.split && !(p.flags & GEOA3_PN_NO_FUSE_BWD);
  pl.fuse_trunk = fuse && p.w4th;
  pl.fuse_t64 = fuse && p.t64.w2th;
  pl.fuse_t3 = fuse && p.t3.w2th;
  pl.pre_lists = fuse && N <= 4096 && !(p.flags & GEOA3_PN_NO_PRE_LISTS);
  pl.fc_ksplit = (size_t)((B + 15) / 16) * 16 * 4096 <= (size_t)B * 128 * N;
  pl.gram_f16 = pl.split;
  pl.clear_keys = !(p.flags & GEOA3_PN_KEYS_CLEAN);
  return pl;
}

// what both directions refuse (besides their own null pointers), before any HIP call
int pn_check(const geoa3_pointnet_weights* pw, int B, int N, const void* workspace) {
  if (!pw || !workspace || B <= 0 || N <= 0) return GEOA3_EINVAL;
  if (pw->t3.K != 3 || pw->t64.K != 64 || pw->classes <= 0) return GEOA3_EINVAL;
  if (((uintptr_t)workspace & 255) != 0) return GEOA3_EINVAL;
  return GEOA3_OK;
}

// the buffers of one T-Net in the workspace
struct TnetBufs {
  float* act128; unsigned long long* m128;   // conv2's activation and its gate bits
  float* pooled; int* arg;
  float *f4, *f5, *T;
  int *hits, *hoff;
};

// One call of either entry point: the plan, the carved workspace and the sizes, shared by the launch helpers and the stages
// below (all of them members: nothing here outlives the call, nothing lives outside it).
struct Call {
  const geoa3_pointnet_weights& p;
  const PnPlan plan;
  const Ws w;
  const int B, N;
  const hipStream_t s;

  TnetBufs bufs_t3() const { return {w.a2, w.m_a2, w.p3, w.i3, w.tf4, w.tf5, w.T3, w.hl3, w.ho3}; }
  TnetBufs bufs_t64() const { return {w.c2, w.m_c2, w.q3, w.iq3, w.qf4, w.qf5, w.T64, w.hlq, w.hoq}; }

  // ---- launch helpers -------------------------------------------------------------------------------------------------
  // Y = act(W X + bias) over [B][K][N] -> [B][Co][N]; shared weights [Co][K]
  int conv(const float* X, int K, const float* W, const float* bias, float* Y, int Co, bool relu,
           unsigned long long* Ymask = nullptr, const unsigned long long* Zmask = nullptr) const {
    ConvArgs a{};
    a.split = plan.split;
    a.Ymask = Ymask; a.Zmask = Zmask;
    a.X = X; a.sXb = (long)K * N; a.ldX = N;
    a.W = W; a.sWb = 0; a.sWco = K; a.sWk = 1;
    a.bias = bias;
    a.sZb = (long)Co * N; a.ldZ = N;   // (no Z: every gate here is a bit mask)
    a.Y = Y; a.sYb = (long)Co * N; a.ldY = N;
    a.Co = Co; a.K = K; a.N = N; a.B = B;
    a.relu = relu;
    return launch_conv_cm(a, s);
  }

  // Y = act(W relu(w1 (T^T x) + b1) + bias): the 3-channel first layer (Model/PointNet.py:79,137-139) folded into the
  // 64-input convolution that follows it; its activation is never written
  int conv_first(const float* x, const float* T, const float* w1, const float* b1, const float* W, const float* bias,
                 float* Y, int Co, unsigned long long* Ymask, unsigned long long* poison_keys = nullptr) const {
    ConvArgs a{};
    a.split = plan.split;
    a.Ymask = Ymask;
    a.poison_keys = poison_keys;
    a.x3 = x; a.T3 = T; a.w1 = w1; a.b1 = b1; a.produce_first = 1;
    a.W = W; a.sWb = 0; a.sWco = 64; a.sWk = 1;
    a.bias = bias;
    a.Y = Y; a.sYb = (long)Co * N; a.ldY = N;
    a.Co = Co; a.K = 64; a.N = N; a.B = B;
    a.relu = 1;
    return launch_conv_cm(a, s);
  }

  // The first layer's backward behind the input-gradient convolution that feeds it, in one kernel: G64 = relu'(first layer)
  // * (W X) with the first layer's sign recomputed from x (no G64 in memory), dx (+)= T w1^T G64, and, with dTpart, the
  // per-workgroup partial sums of d/dT
  int conv_gate_first(const float* X, int K, const float* W, const float* x, const float* T, const float* w1,
                      const float* b1, float* dx, int accumulate, float* dTpart = nullptr) const {
    ConvArgs a{};
    a.split = plan.split;
    a.dx3 = dx; a.accumulate = accumulate; a.dTpart = dTpart;
    a.X = X; a.sXb = (long)K * N; a.ldX = N;
    a.W = W; a.sWb = 0; a.sWco = K; a.sWk = 1;
    a.x3 = x; a.T3 = T; a.w1 = w1; a.b1 = b1; a.gate_first = 1;
    a.sYb = (long)64 * N; a.ldY = N;
    a.Co = 64; a.K = K; a.N = N; a.B = B;
    return launch_conv_cm(a, s);
  }

  int wide(const float* X, const float* W, const void* Wh, float unscale, const float* bias, float* out, int* arg, int taps,
           int* hits, int* hoff) const {
    WideArgs a{};
    if (plan.pre_lists) { a.hits = hits; a.hoff = hoff; }
    a.keys = w.keys;
    a.keys_clean = 1;   // zeroed once per forward; every finalize leaves them zero
    a.Wh = Wh; a.unscale = unscale;
    a.X = X; a.sXb = (long)128 * N; a.ldX = N;
    a.W = W; a.bias = bias; a.out = out; a.arg = arg;
    a.Co = 1024; a.N = N; a.B = B; a.taps = taps;
    return launch_wide_max(a, s);
  }

  int wide_bwd(const float* g, const int* arg, const float* W, const float* Z, const unsigned long long* Zmask, float* dX,
               int taps) const {
    WideBwdArgs a{};
    a.Zmask = Zmask;
    a.g = g; a.arg = arg; a.W = W;
    a.Z = Z; a.sZb = (long)128 * N; a.ldZ = N;
    a.dX = dX; a.sXb = (long)128 * N; a.ldX = N;
    a.Co = 1024; a.N = N; a.B = B; a.taps = taps;
    return launch_wide_max_bwd(a, s);
  }

  // Sparse backward of a 1024-wide layer + the gated 128 -> 64 layer behind it in one kernel (split mode: bit gates): dY
  // [B][64][N] under Zmask2.  Or, with x3 (Zmask2 and W2t unused): that layer is the one behind the 3-channel first layer
  // w1 / b1, whose backward finishes in the same kernel: dY = dx [B][3][N] += w1^T (..)
  int wide_bwd_conv(const float* g, const int* arg, const float* W, const unsigned long long* Zmask, const float* W2t,
                    const unsigned long long* Zmask2, float* dY, int taps, const int* hits, const int* hoff,
                    const void* W2th, float w2th_unscale, const float* x3 = nullptr, const float* w1 = nullptr,
                    const float* b1 = nullptr) const {
    WideBwdArgs a{};
    a.W2th = W2th; a.w2th_unscale = w2th_unscale;
    if (plan.pre_lists) { a.hits = hits; a.hoff = hoff; }
    a.Zmask = Zmask;
    a.g = g; a.arg = arg; a.W = W;
    if (x3) { a.x3 = x3; a.w1 = w1; a.b1 = b1; a.dx3 = dY; }
    else {
      a.W2t = W2t; a.Zmask2 = Zmask2;
      a.dY = dY; a.sYb = (long)64 * N; a.ldY = N;
    }
    a.Co = 1024; a.N = N; a.B = B; a.taps = taps;
    return launch_wide_bwd_conv(a, s);
  }

  // transform_net.forward (Model/PointNet.py:78-87) after its first layer: conv2 (unless have128: act128 and its gate bits
  // already produced by the trunk's chain kernel), conv3 + max, the three FC layers.
  // act64 == nullptr: the T-Net reads the cloud itself (K = 3) and its first layer is folded into conv2 (x3 given)
  int tnet_tail_fwd(const geoa3_tnet_weights& t, const TnetBufs& u, const float* act64, const float* x3,
                    bool have128 = false) const {
    if (!have128) {
      if (act64) TRY(conv(act64, 64, t.w2, t.b2, u.act128, 128, true, u.m128));
      else if (plan.chain) {   // conv1 + conv2 of the 3-channel T-Net: the chain kernel with one stage
        ConvChainArgs a{};
        a.x3 = x3; a.w1 = t.w1; a.b1 = t.b1;
        a.poison_keys = w.keys;   // the first kernel that reads the cloud: the non-finite rule (pn_poison_keys)
        a.N = N; a.B = B; a.ns = 1;
        a.st[0] = ChainStage{t.w2, 0, t.b2, u.act128, (long)128 * N, u.m128, 128};
        TRY(launch_conv_chain(a, s));
      } else TRY(conv_first(x3, nullptr, t.w1, t.b1, t.w2, t.b2, u.act128, 128, u.m128, w.keys));
    }
    TRY(wide(u.act128, t.w3p, t.w3h, t.w3h_unscale, t.b3, u.pooled, u.arg, 1, u.hits, u.hoff));
    TRY(fc(u.pooled, 1024, t.f1, t.fb1, u.f4, 512, B, true, nullptr, s));
    TRY(fc(u.f4, 512, t.f2, t.fb2, u.f5, 256, B, true, nullptr, s));
    return fc(u.f5, 256, t.f3, t.fb3, u.T, t.K * t.K, B, false, nullptr, s);
  }

  // d/d(transform) gT [B][K*K] -> the gradient in front of the T-Net's first layer.  The 64-channel T-Net (x3 == nullptr):
  // G64out [B][64][N] = the gradient w.r.t. the pre-activation of its first layer, gated by m64.  The 3-channel T-Net: its
  // first layer's backward runs in the last kernel too, which ADDS the branch into G64out = dx.
  // fused: the plan's choice for this T-Net (PnPlan::fuse_t64 / fuse_t3)
  int tnet_bwd(const geoa3_tnet_weights& t, const TnetBufs& u, bool fused, const float* gT, const unsigned long long* m64,
               const float* x3, float* G64out) const {
    TRY(fc(gT, t.K * t.K, t.f3t, nullptr, w.g256, 256, B, false, u.f5, s, plan.fc_ksplit ? w.G128 : nullptr));
    TRY(fc(w.g256, 256, t.f2t, nullptr, w.g512, 512, B, false, u.f4, s));
    TRY(fc(w.g512, 512, t.f1t, nullptr, w.g1024, 1024, B, false, u.pooled, s));
    if (fused)
      return wide_bwd_conv(w.g1024, u.arg, t.w3, u.m128, t.w2t, m64, G64out, 1, u.hits, u.hoff, t.w2th, t.w2th_unscale, x3,
                           t.w1, t.b1);
    TRY(wide_bwd(w.g1024, u.arg, t.w3, u.act128, u.m128, w.G128, 1));
    if (!x3) return conv(w.G128, 128, t.w2t, nullptr, G64out, 64, false, nullptr, m64);
    return conv_gate_first(w.G128, 128, t.w2t, x3, nullptr, t.w1, t.b1, G64out, 1);
  }

  // ---- the forward's stages, in order ---------------------------------------------------------------------------------
  // input transform (Model/PointNet.py:137-138)
  int fwd_input_transform(const float* x) const { return tnet_tail_fwd(p.t3, bufs_t3(), nullptr, x); }

  // trunk conv1, conv2 (:139-140).  Chain form: ... and the feature transform's conv1, conv2 (:78-80) in the same kernel:
  // h2 is written (the backward and conv3 read it), c1 exists only as gate bits, c2 is the T-Net's 1024-wide layer's input
  int fwd_trunk_front(const float* x) const {
    if (!plan.chain) return conv_first(x, w.T3, p.w1, p.b1, p.w2, p.b2, w.h2, 64, w.m_h2);
    ConvChainArgs a{};
    a.x3 = x; a.T3 = w.T3; a.w1 = p.w1; a.b1 = p.b1;
    a.N = N; a.B = B; a.ns = 3;
    a.st[0] = ChainStage{p.w2, 0, p.b2, w.h2, (long)64 * N, w.m_h2, 64};
    a.st[1] = ChainStage{p.t64.w1, 0, p.t64.b1, nullptr, 0, w.m_c1, 64};
    a.st[2] = ChainStage{p.t64.w2, 0, p.t64.b2, w.c2, (long)128 * N, w.m_c2, 128};
    return launch_conv_chain(a, s);
  }

  // feature transform (:142-143), then folded into conv3 (:143-144): W3 (T64^T h2) = (W3 T64^T) h2 -- one 64^3 product per
  // instance instead of a pass over [B,64,N]
  int fwd_feature_transform() const {
    if (!plan.chain) TRY(conv(w.h2, 64, p.t64.w1, p.t64.b1, w.c1, 64, true, w.m_c1));
    TRY(tnet_tail_fwd(p.t64, bufs_t64(), w.c1, nullptr, /*have128=*/plan.chain));
    FcArgs g{};   // W3eff[b][o][i] = sum_j W3[o][j] T64[b][i][j]
    g.X = p.w3; g.ldX = 64; g.sXb = 0;
    g.W = w.T64; g.ldW = 64; g.sWb = 4096;
    g.Y = w.W3eff; g.ldY = 64; g.sYb = 4096;
    g.M = 64; g.Nout = 64; g.K = 64; g.batch = B;
    return launch_fc(g, s);
  }

  // conv3 with the per-instance W3eff, conv4 (:144-145).  Chain form: one kernel, h3 exists only as gate bits
  int fwd_conv3_conv4() const {
    if (plan.chain) {
      ConvChainArgs a{};
      a.X = w.h2; a.sXb = (long)64 * N; a.ldX = N;
      a.N = N; a.B = B; a.ns = 2;
      a.st[0] = ChainStage{w.W3eff, 4096, p.b3, nullptr, 0, w.m_h3, 64};
      a.st[1] = ChainStage{p.w4, 0, p.b4, w.h4, (long)128 * N, w.m_h4, 128};
      return launch_conv_chain(a, s);
    }
    ConvArgs a{};
    a.split = plan.split;
    a.X = w.h2; a.sXb = (long)64 * N; a.ldX = N;
    a.W = w.W3eff; a.sWb = 4096; a.sWco = 64; a.sWk = 1;
    a.bias = p.b3;
    a.Y = w.h3; a.sYb = (long)64 * N; a.ldY = N;
    a.Ymask = w.m_h3;
    a.Co = 64; a.K = 64; a.N = N; a.B = B; a.relu = 1;
    TRY(launch_conv_cm(a, s));
    return conv(w.h3, 64, p.w4, p.b4, w.h4, 128, true, w.m_h4);
  }

  // conv5 + max (:146-147), classifier head (:150-152; dropout is the identity in eval mode)
  int fwd_conv5_head(float* logits) const {
    TRY(wide(w.h4, p.w5p, p.w5h, p.w5h_unscale, p.b5, w.p5, w.i5, 3, w.hl5, w.ho5));
    TRY(fc(w.p5, 1024, p.f1, p.fb1, w.f6, 512, B, true, nullptr, s));
    TRY(fc(w.f6, 512, p.f2, p.fb2, w.f7, 256, B, true, nullptr, s));
    return fc(w.f7, 256, p.f3, p.fb3, logits, p.classes, B, false, nullptr, s, nullptr, w.T3, 9);   // NaN where T3[b] is
  }

  // ---- the backward's stages, in order --------------------------------------------------------------------------------
  // classifier head, then max + conv5 (sparse) and conv4: G64a = d/d(pre-activation of h3)
  int bwd_head_conv5_conv4(const float* dlogits) const {
    TRY(fc(dlogits, p.classes, p.f3t, nullptr, w.g256, 256, B, false, w.f7, s));
    TRY(fc(w.g256, 256, p.f2t, nullptr, w.g512, 512, B, false, w.f6, s));
    TRY(fc(w.g512, 512, p.f1t, nullptr, w.g1024, 1024, B, false, w.p5, s));
    if (plan.fuse_trunk)
      return wide_bwd_conv(w.g1024, w.i5, p.w5, w.m_h4, p.w4t, w.m_h3, w.G64a, 3, w.hl5, w.ho5, p.w4th, p.w4th_unscale);
    TRY(wide_bwd(w.g1024, w.i5, p.w5, w.h4, w.m_h4, w.G128, 3));
    return conv(w.G128, 128, p.w4t, nullptr, w.G64a, 64, false, nullptr, w.m_h3);
  }

  // conv3 + feature transform, merged as in forward -- the transform's share:
  //   gT64 = dT64[b][i][j] = sum_n h2[i][n] (W3^T G64a)[j][n] = ((h2 G64a^T) W3)[i][j]
  int bwd_feature_transform_grad() const {
    // P[b][i][o] = sum_n h2[b][i][n] G64a[b][o][n].  On the f16 matrix pipe the partial sums of the four workgroups per
    // instance go through dh2 (written only afterwards: 8 * 4096 floats per instance fit its 64 * N from N = 512 on, and
    // gram64_parts(N) is at most 4 below N = 897); otherwise the batched NT product of the FC kernel (K = N)
    if (plan.gram_f16) TRY(launch_gram64(w.h2, w.G64a, B, N, w.P64, w.dh2, s));
    else {
      FcArgs g{};
      g.X = w.h2; g.ldX = N; g.sXb = (long)64 * N;
      g.W = w.G64a; g.ldW = N; g.sWb = (long)64 * N;
      g.Y = w.P64; g.ldY = 64; g.sYb = 4096;
      g.M = 64; g.Nout = 64; g.K = N; g.batch = B;
      TRY(launch_fc(g, s));
    }
    FcArgs q{};   // dT64[b][i][j] = sum_o P[b][i][o] W3[o][j]
    q.X = w.P64; q.ldX = 64; q.sXb = 4096;
    q.W = p.w3t; q.ldW = 64; q.sWb = 0;
    q.Y = w.gT64; q.ldY = 64; q.sYb = 4096;
    q.M = 64; q.Nout = 64; q.K = 64; q.batch = B;
    return launch_fc(q, s);
  }

  // The rest of the trunk down to dx and the dT3 partials (per 256-point workgroup), chain form.  The T-Net branch's
  // gradient goes to the dh2 buffer (the Gram kernel's scratch is consumed by now); then ONE kernel: dh2 = gate_h2(W3eff^T
  // G64a + W_t64.conv1^T G), conv2's backward, trunk conv1 + input transform backward -- dh2 itself is never written
  int bwd_trunk_front_chain(const float* x, float* dx) const {
    TRY(tnet_bwd(p.t64, bufs_t64(), plan.fuse_t64, w.gT64, w.m_c1, nullptr, w.dh2));
    ConvBwdChainArgs a{};
    a.Xa = w.G64a; a.Wa = w.W3eff; a.sWa = 4096;
    a.Xb = w.dh2; a.Wb = p.t64.w1;
    a.Zmask = w.m_h2;
    a.W2t = p.w2t;
    a.x3 = x; a.T3 = w.T3; a.w1 = p.w1; a.b1 = p.b1;
    a.dx = dx; a.dTpart = w.dTpart;
    a.N = N; a.B = B;
    return launch_conv_bwd_chain(a, s);
  }

  // ... and layer by layer: dh2 = T64 W3^T G64a = W3eff^T G64a, the T-Net's backward (into G64a, free by then), dh2 +=
  // W_t64.conv1^T G64a under the relu gate of h2, conv2's backward fused with trunk conv1 + input transform backward
  int bwd_trunk_front_layers(const float* x, float* dx) const {
    ConvArgs a{};   // dh2[b][i][n] = sum_o W3eff[b][o][i] G64a[b][o][n]
    a.split = plan.split;
    a.X = w.G64a; a.sXb = (long)64 * N; a.ldX = N;
    a.W = w.W3eff; a.sWb = 4096; a.sWco = 1; a.sWk = 64;
    a.Y = w.dh2; a.sYb = (long)64 * N; a.ldY = N;
    a.Co = 64; a.K = 64; a.N = N; a.B = B;
    TRY(launch_conv_cm(a, s));
    TRY(tnet_bwd(p.t64, bufs_t64(), plan.fuse_t64, w.gT64, w.m_c1, nullptr, w.G64a));
    // the same launch with the T-Net's shared conv1 (W^T through the strided loader), added under the gate
    a.W = p.t64.w1; a.sWb = 0;
    a.Zmask = w.m_h2;
    a.accumulate = 1;
    TRY(launch_conv_cm(a, s));
    return conv_gate_first(w.dh2, 64, p.w2t, x, w.T3, p.w1, p.b1, dx, 0, w.dTpart);
  }

  // d/dT3 from its partial sums, then T-Net 3's backward; its last kernel adds the T-Net branch into dx
  int bwd_input_transform(const float* x, float* dx) const {
    TRY(launch_reduce_dT(w.dTpart, (N + 255) / 256, w.gT3, B, s));
    return tnet_bwd(p.t3, bufs_t3(), plan.fuse_t3, w.gT3, nullptr, x, dx);
  }
};

}  // namespace

extern "C" int64_t geoa3_pointnet_workspace_bytes(int B, int N, int classes) {
  if (B <= 0 || N <= 0 || classes <= 0) return -1;
  return (int64_t)carve(nullptr, B, N).total;
}

// diagnostics (geoa3_hip_debug.h): names and byte offsets of the workspace's buffers, in address order
extern "C" int geoa3_debug_pointnet_workspace_layout(int B, int N, int classes, const char** names, int64_t* offsets,
                                                     int cap) {
  if (B <= 0 || N <= 0 || classes <= 0) return -1;
  char* const base = reinterpret_cast<char*>(static_cast<uintptr_t>(1) << 40);
  const Ws w = carve(base, B, N);
  const WsField f[] = {PN_WS(GEOA3_WS_FIELD)};
  return ws_layout(f, (int)(sizeof(f) / sizeof(f[0])), base, names, offsets, cap);
}

// diagnostics (geoa3_hip_debug.h): the plan of a call as GEOA3_PN_ROUTE_* bits
extern "C" int geoa3_debug_pointnet_route(const geoa3_pointnet_weights* pw, int B, int N) {
  TRY(pn_check(pw, B, N, /*an aligned stand-in for the workspace*/ reinterpret_cast<const void*>(uintptr_t(256))));
  const PnPlan pl = pn_plan(*pw, B, N);
  return (pl.split ? GEOA3_PN_ROUTE_SPLIT : 0) | (pl.chain ? GEOA3_PN_ROUTE_CHAIN : 0) |
         (pl.fuse_trunk ? GEOA3_PN_ROUTE_FUSE_TRUNK : 0) | (pl.fuse_t64 ? GEOA3_PN_ROUTE_FUSE_T64 : 0) |
         (pl.fuse_t3 ? GEOA3_PN_ROUTE_FUSE_T3 : 0) | (pl.pre_lists ? GEOA3_PN_ROUTE_PRE_LISTS : 0) |
         (pl.fc_ksplit ? GEOA3_PN_ROUTE_FC_KSPLIT : 0) | (pl.gram_f16 ? GEOA3_PN_ROUTE_GRAM_F16 : 0) |
         (pl.clear_keys ? GEOA3_PN_ROUTE_CLEAR_KEYS : 0);
}

extern "C" int geoa3_pointnet_forward(const geoa3_pointnet_weights* pw, const float* x, int B, int N, float* logits,
                                      void* workspace, void* stream) {
  if (!x || !logits) return GEOA3_EINVAL;
  TRY(pn_check(pw, B, N, workspace));
  const Call c{*pw, pn_plan(*pw, B, N), carve(workspace, B, N), B, N, geoa3_stream(stream)};
  if (c.plan.clear_keys &&
      hipMemsetAsync(c.w.keys, 0, (size_t)B * 1024 * sizeof(unsigned long long), c.s) != hipSuccess)
    return GEOA3_ELAUNCH;
  TRY(c.fwd_input_transform(x));
  TRY(c.fwd_trunk_front(x));
  TRY(c.fwd_feature_transform());
  TRY(c.fwd_conv3_conv4());
  return c.fwd_conv5_head(logits);
}

extern "C" int geoa3_pointnet_backward(const geoa3_pointnet_weights* pw, const float* x, const float* dlogits, int B,
                                       int N, float* dx, void* workspace, void* stream) {
  if (!x || !dlogits || !dx) return GEOA3_EINVAL;
  TRY(pn_check(pw, B, N, workspace));
  const Call c{*pw, pn_plan(*pw, B, N), carve(workspace, B, N), B, N, geoa3_stream(stream)};
  TRY(c.bwd_head_conv5_conv4(dlogits));
  TRY(c.bwd_feature_transform_grad());
  TRY(c.plan.chain ? c.bwd_trunk_front_chain(x, dx) : c.bwd_trunk_front_layers(x, dx));
  return c.bwd_input_transform(x, dx);
}

// ------------------------------------------------------------------------------------------
// The forward's chain kernels in isolation (geoa3_hip_debug.h; tests/test_gpu_pointnet_fwd.py): the args struct as
// tnet_tail_fwd / fwd_trunk_front / fwd_conv3_conv4 fill it, then the launcher -- nothing else.
// ------------------------------------------------------------------------------------------
extern "C" int geoa3_debug_conv_chain(const float* X, const float* x3, const float* T3, const float* w1, const float* b1,
                                      int ns, const float* const* W, const int64_t* sWb, const float* const* bias,
                                      float* const* Y, void* const* Ymask, int B, int N, void* stream) {
  if (ns < 1 || ns > 3 || !W || !sWb || !bias || !Y || !Ymask || (X && x3)) return GEOA3_EINVAL;
  ConvChainArgs a{};
  if (x3) { a.x3 = x3; a.T3 = T3; a.w1 = w1; a.b1 = b1; }
  else { a.X = X; a.sXb = (long)64 * N; a.ldX = N; }
  a.N = N; a.B = B; a.ns = ns;
  for (int i = 0; i < ns; ++i) {
    const int Co = i + 1 < ns ? 64 : 128;
    a.st[i] = ChainStage{W[i], (long)sWb[i], bias[i], Y[i], (long)Co * N, static_cast<unsigned long long*>(Ymask[i]), Co};
  }
  return launch_conv_chain(a, geoa3_stream(stream));
}

// ------------------------------------------------------------------------------------------
// Single kernels of the backward in isolation (geoa3_hip_debug.h; tests/test_gpu_pointnet_bwd.py): each entry fills the
// args struct the way geoa3_pointnet_backward does and calls the kernel's launcher -- nothing else.
// ------------------------------------------------------------------------------------------
extern "C" int geoa3_debug_wide_bwd_conv(const float* g, const int32_t* arg, const float* W, const void* Zmask,
                                         const float* W2t, const void* W2th, float w2th_unscale, const void* Zmask2,
                                         float* dY, const float* x3, const float* w1, const float* b1, float* dx3,
                                         const int32_t* hits, const int32_t* hoff, int B, int N, int taps, void* stream) {
  if (!g || !arg || !W || B <= 0 || N <= 0) return GEOA3_EINVAL;
  WideBwdArgs a{};
  a.g = g; a.arg = arg; a.W = W;
  a.Zmask = static_cast<const unsigned long long*>(Zmask);
  a.W2t = W2t; a.W2th = W2th; a.w2th_unscale = w2th_unscale;
  a.Zmask2 = static_cast<const unsigned long long*>(Zmask2);
  a.dY = dY; a.sYb = (long)64 * N; a.ldY = N;
  a.x3 = x3; a.w1 = w1; a.b1 = b1; a.dx3 = dx3;
  a.hits = hits; a.hoff = hoff;
  a.Co = 1024; a.N = N; a.B = B; a.taps = taps;
  return launch_wide_bwd_conv(a, geoa3_stream(stream));
}

extern "C" int geoa3_debug_gram64(const float* A, const float* G, int B, int N, float* P, float* scratch, void* stream) {
  if (!A || !G || !P || B <= 0 || N <= 0) return GEOA3_EINVAL;
  return launch_gram64(A, G, B, N, P, scratch, geoa3_stream(stream));
}

extern "C" int geoa3_debug_conv_bwd_chain(const float* Xa, const float* Wa, int64_t sWa, const float* Xb, const float* Wb,
                                          const void* Zmask, const float* W2t, const float* x3, const float* T3,
                                          const float* w1, const float* b1, float* dx, float* dTpart, float* dT, int B, int N,
                                          void* stream) {
  if (!dTpart || !dT) return GEOA3_EINVAL;
  ConvBwdChainArgs a{};
  a.Xa = Xa; a.Wa = Wa; a.sWa = (long)sWa;
  a.Xb = Xb; a.Wb = Wb;
  a.Zmask = static_cast<const unsigned long long*>(Zmask);
  a.W2t = W2t;
  a.x3 = x3; a.T3 = T3; a.w1 = w1; a.b1 = b1;
  a.dx = dx; a.dTpart = dTpart;
  a.N = N; a.B = B;
  hipStream_t s = geoa3_stream(stream);
  TRY(launch_conv_bwd_chain(a, s));
  return launch_reduce_dT(dTpart, (N + 255) / 256, dT, B, s);
}

extern "C" int geoa3_debug_fc_ex(const float* X, int ldX, int64_t sXb, const float* W, int ldW, int64_t sWb,
                                 const float* bias, const float* Z, int ldZ, float* Y, int ldY, int64_t sYb, int M, int Nout,
                                 int K, int batch, int relu, int ksplit, float* kscratch, void* stream) {
  if (!X || !W || !Y || M <= 0 || Nout <= 0 || K <= 0) return GEOA3_EINVAL;
  FcArgs a{};
  a.X = X; a.ldX = ldX; a.sXb = (long)sXb;
  a.W = W; a.ldW = ldW; a.sWb = (long)sWb;
  a.bias = bias;
  a.Z = Z; a.ldZ = ldZ;
  a.Y = Y; a.ldY = ldY; a.sYb = (long)sYb;
  a.M = M; a.Nout = Nout; a.K = K; a.batch = batch; a.relu = relu;
  a.ksplit = ksplit & 0xff; a.tile = ksplit >> 8;   // as geoa3_debug_fc: (tile << 8) | waves, 0 = the shipped choice
  a.kscratch = kscratch;
  return launch_fc(a, geoa3_stream(stream));
}
