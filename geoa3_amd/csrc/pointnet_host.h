// Host-only helpers shared by the two victims' launch sequences (pointnet.hip, pointnet2_net.hip).  No device code.
#pragma once
#include "pointnet_kernels.h"

#define TRY(expr)               \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ != 0) return rc__; \
  } while (0)

// Y[M][Nout] = act(X[M][K] W[Nout][K]^T + bias), gated by Z > 0 when given (FcArgs::kscratch: see there)
static inline int fc(const float* X, int K, const float* W, const float* bias, float* Y, int Nout, int M, bool relu,
                     const float* Z, hipStream_t s, float* kscratch = nullptr, const float* poison = nullptr, int ldP = 0) {
  FcArgs a{};
  a.kscratch = kscratch;
  a.poison = poison; a.ldP = ldP;
  a.X = X; a.ldX = K;
  a.W = W; a.ldW = K;
  a.bias = bias;
  a.Z = Z; a.ldZ = Nout;
  a.Y = Y; a.ldY = Nout;
  a.M = M; a.Nout = Nout; a.K = K; a.relu = relu;
  return launch_fc(a, s);
}

// A workspace is stated ONCE, as a list macro with one X(type, name, elements) line per buffer in address order.  The three
// expansions below make the struct's members, the carve-up (every buffer starts on a 256-byte boundary; `p` = base or null,
// `off` = running offset, `w` = the struct) and the names of the debug layout function from that one list.
#define GEOA3_WS_MEMBER(T, name, elements) T* name;
#define GEOA3_WS_TAKE(T, name, elements)                   \
  w.name = reinterpret_cast<T*>(p ? p + off : nullptr);    \
  off += ((size_t)(elements) * sizeof(T) + 255) / 256 * 256;
#define GEOA3_WS_FIELD(T, name, elements) {#name, w.name},

struct WsField {
  const char* name;
  const void* p;
};
// names and byte offsets of the first `cap` of the n fields of a workspace carved at `base`; returns n
static inline int ws_layout(const WsField* f, int n, const char* base, const char** names, int64_t* offsets, int cap) {
  for (int i = 0; i < n && i < cap; ++i) {
    names[i] = f[i].name;
    offsets[i] = (int64_t)(static_cast<const char*>(f[i].p) - base);
  }
  return n;
}
