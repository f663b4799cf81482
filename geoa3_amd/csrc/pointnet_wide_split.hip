// The T-Nets' 1024-wide layer (conv3, one tap) of pointnet_wide.hip on the f16 matrix pipe with split fp32 operands
// (gfx950).
//
// gfx950 has no tf32/xf32 MFMA and its fp32 MFMA runs at 1/16 of the 16-bit rate.  Every fp32 operand v (after a
// power-of-two scaling that puts the largest magnitude of its tensor / tile into [2^13, 2^14)) is carried as two fp16
// values,
//     hi = rn16(v),   lo = rn16(v - hi)                   (|v - hi - lo| <= 2^-24 |v| while lo is a normal fp16),
// and a product a*w is evaluated as  a_hi*w_hi + a_hi*w_lo + a_lo*w_hi  with fp32 accumulation in the matrix core
// (`v_mfma_f32_32x32x16_f16`; a product of two fp16 values is exact in fp32).  The dropped a_lo*w_lo term is 2^-24
// relative.  Three 32-cycle MFMAs do the work of eight 64-cycle fp32 ones.  Error model: an operand smaller than
// 2^-16 of the largest one of its tile has a subnormal (possibly flushed) lo part and keeps 11 bits -- an absolute
// error below 2^-28 of the largest term, i.e. 1/16 ulp of a sum that contains it.  Measured (tools/wide_accuracy.py):
// the logits' and the input gradient's error against a float64 evaluation equals that of the fp32 MFMA kernel and of
// the fp32 CPU oracle.
// The activation scale is chosen PER WORK UNIT from the tile's own maximum while it is staged (no range restriction;
// a non-finite activation poisons the instance's features with NaN); the weights are scaled on the host
// (geoa3_amd/pointnet.py pack_wide_split); the maxima are scaled back before they are published.
//
// Why this shape for this layer: measured on MI355X, the T-Nets' conv3 (K = 128: a third of conv5's MFMAs between two
// epilogues) takes 0.182 ms on 32x32x16 against 0.292 ms on the 16x16x32 kernel of pointnet_wide16.hip; conv5 (K = 384)
// goes the other way (0.495 ms here, 0.444 ms there) and runs there.
//
// Structure: the unit schedule, the staging pass, the hand-off of a unit's maxima and the launcher are those of
// wide_unit.h, shared with conv5's kernel.  This file's own: the LDS image has rows padded to 272 B, so the A operand of
// a k-step (8 consecutive ci of one point) is one conflict-free ds_read_b128; each wave owns CB x 32 channels x 128 points
// (4 point tiles per channel tile); the weight fragments stream from L2 (2 x 16 B per lane per channel tile and k-step of
// 16) through a register ring across the channel groups; a unit's maxima wait in an array of their own (s_keys).  Keys and
// the finalize kernel are those of the fp32 path; the epilogue is the two-pass, branch-free first maximum of
// wide_epilogue.h (the lane's maximum over its 64 values, then the lowest point that equals it; ragged tiles masked to
// -inf first): the layer alone 188.0 -> 183.4 us against the one-pass compare / select chain, same bits (NOTEBOOK 10).
//
// The k loop's operand pipeline (NOTEBOOK 10, "T-Net conv3 dissected"; profiles/tnet_conv3_ab.txt):
//   A: the fragments of one whole k-step live in registers (4 point tiles x hi / lo = 8 x half8).  A tile's pair is refilled
//      for the NEXT k-step right behind the tile's own three MFMAs, so a read has the other three tiles' 9 MFMAs (~290
//      cycles) of cover -- the finest form of conv5's half-k-step refill, +16 registers (220 of 256, no scratch).  The
//      fragments do not depend on the channel group: the last k-step of a group reads k-step 0 again and the next group
//      starts with its operands present.  After a unit's last group that read is dead; the epilogue's LDS traffic and the
//      __syncthreads() in front of the next staging pass wait for it (lgkmcnt(0)) before any wave overwrites the image.
//   B: ring slot f is reloaded for k-step s + PF behind the 12 MFMAs that read it (36 MFMAs ahead of its next use, no copy).
//   `sched_barrier(0)` holds both in place.  Left to itself the scheduler sank every load to its use: each ds_read_b128
//   directly in front of its MFMA behind an lgkmcnt(0), and the ring's global loads to the end of the block with a
//   vmcnt wait and a register copy behind them -- the matrix pipe idle for an LDS or an L2 round trip every few MFMAs
//   whenever the CU's other workgroup was staging or in an epilogue.
//   C: the first MFMA of each accumulator takes a literal zero C operand (+0, what the 64 v_mov per group wrote before);
//   the first block of PF k-steps is a copy of the block's code for that, so a group's 96 MFMAs are straight-line code.
// The MFMAs on each accumulator are the same, in the same order (hh, hl, lh per k-step, k ascending): same bits.
#include "pointnet_kernels.h"
#include "wide_epilogue.h"
#include "wide_unit.h"
#include <type_traits>

namespace {

constexpr int SP_OCC = 2;                    // workgroups per CU
constexpr int SP_ROWB = 272;                 // bytes per LDS row: 128 fp16 + 16 B pad (row stride = 4 banks mod 64)
constexpr int SP_PIECEB = WIDE_PTS * SP_ROWB;  // 34,816
constexpr int SP_LDS = 2 * SP_PIECEB;        // 69,632 B: two workgroups per CU

// Timing-only variant builds (tools/build_w16_variants.sh, never the shipped library): the bit mask of pointnet_wide16.hip's
// GEOA3_W16_CUT.  1 = no staging (the LDS image is left as it is, the barriers stay), 2 = no epilogue / keys, 4 = no
// weight-fragment loads (the ring is reused).  A cut build computes wrong values; it touches no byte the shipped kernel does not.
#ifndef GEOA3_WSP_CUT
#define GEOA3_WSP_CUT 0
#endif

__global__ __launch_bounds__(WIDE_THREADS, SP_OCC) void wide_split_kernel(WideArgs a, int slots_per_xcd) {
  // channel tiles of 32 per wave.  (Round 4: CB = 2 -- half the LDS reads per MFMA -- 186.2 against 185.2 us: LDS
  // bandwidth is not what holds this kernel at ~1.1-1.2 PF on the f16 pipe.)  The loops over c stay: the same loops
  // without them compile to other machine code (more scratch).
  constexpr int CB = 1;
  constexpr int KS = 8;                      // k-steps of 16 per channel tile
  constexpr int PF = 4;                      // k-steps of weight fragments in flight; KS % PF == 0
  constexpr int NBLK = KS / PF;              // blocks of PF k-steps
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ float s_max[4];
  // packed maxima of the current unit until wide_flush publishes them (on its own within run-to-run noise)
  __shared__ unsigned long long s_keys[4][WIDE_GROUPS * CB][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 5, l31 = lane & 31;
  const int N = a.N;
  const half8* Wall = reinterpret_cast<const half8*>(a.Wh);
  const WideSchedule sch = wide_schedule(a, slots_per_xcd, s_max);
  int nstamp = 0;
  auto stamp = [&]() {   // diagnostic build only (a.stamps != null): wave 0 of workgroup 0 records s_memtime
    if (a.stamps && blockIdx.x == 0 && tid == 0 && nstamp < 255) a.stamps[1 + nstamp++] = __builtin_amdgcn_s_memtime();
  };
  WidePending pend;
  auto flush = [&]() { wide_flush(pend, a, lane, [&](int i, int l) { return &s_keys[wave][i][l]; }); };
  for (int it = 0; it < sch.iterations(); ++it) {
    const WideUnit un = wide_unit(sch, it);
    const int b = un.b, n0 = un.n0, g_begin = un.g_begin, g_end = un.g_end;
    const float* X = a.X + (size_t)b * a.sXb;
    stamp();
    // ---- stage (wide_unit.h): rows 0..127 of the image = points n0 .. n0+127
    float unscale = a.unscale;
    if (GEOA3_WSP_CUT & 1) {   // the barriers of the staging pass, none of its loads, arithmetic or LDS writes
      stamp();
      flush();
      __syncthreads();
      __syncthreads();
      __syncthreads();
    } else {
      float xv[2][4][8];
      int ldx = a.ldX;
      asm volatile("" : "+s"(ldx));   // opaque: see wide_load_tile
      wide_load_tile(X, ldx, n0, N, lane, wave, xv);
      const float m = wide_abs_max(xv, 0.f);
      stamp();
      flush();           // the previous unit's maxima, behind this unit's loads
      float scale;
      bool bad = wide_tile_scale(m, s_max, lane, wave, scale, unscale);
      unscale *= a.unscale;
      bad |= wide_split_store<SP_ROWB, SP_PIECEB>(xv, scale, smem_raw, lane, wave);
      wide_poison(a, b, bad);
    }
    stamp();
    // A operand of lane (r = l31, h = kh), tile t, k-step s (ci0 = 16 s): row 32t + r, bytes (ci0 + 8h) * 2
    const unsigned char* abase = smem_raw + l31 * SP_ROWB + kh * 16;
    // fragments of the wave's channel tile c (< CB) of group step g: [T][s][piece][lane].  (Since the never-instantiated
    // unit split left this expression the stream's base pointers stay in registers across the group loop: 212 -> 220.)
    auto wbase = [&](int g, int c) {
      const int co = g * CB * 128 + wave * 32 * CB + 32 * c;
      return Wall + (size_t)(co / 32) * KS * 2 * 64 + lane;
    };
    half8 wf[PF][CB][2];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const half8* W0 = wbase(g_begin, c);
#pragma unroll
      for (int f = 0; f < PF; ++f) {
        wf[f][c][0] = W0[(size_t)(2 * f) * 64];
        wf[f][c][1] = W0[(size_t)(2 * f + 1) * 64];
      }
    }
    // A fragments of k-step f of the block at `base` (ci0 = 16 (PF sb + f)), point tile t
    auto a_rd = [&](const unsigned char* base, int f, int t, half8& h, half8& l) {
      const unsigned char* ap = base + 32 * t * SP_ROWB + f * 32;
      h = *reinterpret_cast<const half8*>(ap);
      l = *reinterpret_cast<const half8*>(ap + SP_PIECEB);
    };
    // k-step 0 of the unit's first group; every later k-step, and k-step 0 of the following groups, is read under MFMAs
    half8 Ah[4], Al[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) a_rd(abase, 0, t, Ah[t], Al[t]);
#pragma unroll 1
    for (int g = g_begin; g < g_end; ++g) {
      const half8 *Wp[CB], *Wn[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        Wp[c] = wbase(g, c);
        Wn[c] = wbase(g + 1 < g_end ? g + 1 : g, c);
      }
      f32x16 acc[CB][4];
      // one block of PF k-steps (PF sb .. PF sb + PF - 1: ci0 = 16 PF sb + 16 f); FIRST: the group's first block, whose
      // first k-step starts the accumulators from a zero C operand
      auto kblock = [&](int sb, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const unsigned char* ap0 = abase + sb * (PF * 32);
        const unsigned char* ap1 = abase + (sb + 1 < NBLK ? sb + 1 : 0) * (PF * 32);   // the last block wraps to k-step 0
#pragma unroll
        for (int f = 0; f < PF; ++f) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            __builtin_amdgcn_sched_barrier(0);
            // operands swapped as in the fp32 kernel: rows = points, columns = channels
#pragma unroll
            for (int c = 0; c < CB; ++c) {
              f32x16 c0 = acc[c][t];
              if (FIRST && f == 0)
#pragma unroll
                for (int i = 0; i < 16; ++i) c0[i] = 0.f;
              acc[c][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[t], wf[f][c][0], c0, 0, 0, 0);
              acc[c][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[t], wf[f][c][1], acc[c][t], 0, 0, 0);
              acc[c][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al[t], wf[f][c][0], acc[c][t], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // tile t is consumed: refill it for the next k-step while the other tiles' 9 MFMAs run
            if (f + 1 < PF) a_rd(ap0, f + 1, t, Ah[t], Al[t]);
            else a_rd(ap1, 0, t, Ah[t], Al[t]);
          }
          __builtin_amdgcn_sched_barrier(0);
          // ring slot f is consumed: refill it for k-step s + PF (36 MFMAs ahead)
          if (!(GEOA3_WSP_CUT & 4)) {
#pragma unroll
            for (int c = 0; c < CB; ++c) {
              const half8* src = sb + 1 < NBLK ? Wp[c] + (size_t)(2 * PF * 64) * (sb + 1) : Wn[c];
              wf[f][c][0] = src[(2 * f) * 64];
              wf[f][c][1] = src[(2 * f + 1) * 64];
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      kblock(0, std::true_type{});
#pragma unroll 1
      for (int sb = 1; sb < NBLK; ++sb) kblock(sb, std::false_type{});
      stamp();
      // lane: channel co0 + l31; acc[t][r]: point n0 + 32t + (r&3) + 8(r>>2) + 4kh.  Ascending point order, strict >
      const bool full = n0 + WIDE_PTS <= N;
      if (GEOA3_WSP_CUT & 2) {   // the accumulators stay live, nothing is reduced or published
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
          for (int t = 0; t < 4; ++t) asm volatile("" ::"v"(acc[c][t]));
        continue;
      }
      if (!full) {               // points past the end lose to every valid one (point n0 is valid and finite)
        const int left = N - n0 - 4 * kh;
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r16 = 0; r16 < 16; ++r16)
              acc[c][t][r16] = 32 * t + mfma_row(r16, 0) < left ? acc[c][t][r16] : -__builtin_inff();
      }
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        float v;
        int col;
        wide_lane_first_max<64>([&](int i) { return acc[c][i >> 4][i & 15]; },
                                [](int i) { return 32 * (i >> 4) + mfma_row(i & 15, 0); }, v, col);
        col += n0 + 4 * kh;
        const float ov = __shfl_xor(v, 32, 64);
        const int oc = __shfl_xor(col, 32, 64);
        const bool take = wide_merge_take(ov, oc, v, col);
        v = take ? ov : v;
        col = take ? oc : col;
        if (lane < 32) s_keys[wave][(g - g_begin) * CB + c][lane] = wide_key(v * unscale, col);
      }
    }
    stamp();
    if (GEOA3_WSP_CUT & 2) continue;
    pend.b = b;
    pend.co = g_begin * CB * 128 + wave * 32 * CB;
    pend.n = (g_end - g_begin) * CB;
  }
  flush();
  if (a.stamps && blockIdx.x == 0 && tid == 0) a.stamps[0] = nstamp;
}

}  // namespace

int launch_wide_max_split(const WideArgs& a, hipStream_t s) {
  return wide_launch(wide_split_kernel, SP_LDS, SP_OCC, 1, GEOA3_PROF_TNETWIDE, a, s);
}

// One 1024-wide layer in isolation (tools/bench_wide.py, tests): Wp = fp32 fragments; Wh = split fragments in the layout
// the library uses for this tap count (1: pack_wide_split, 3: pack_wide_split16) or NULL.
extern "C" int geoa3_debug_wide_fwd(const float* X, const float* Wp, const void* Wh, float unscale, const float* bias,
                                    float* out, int32_t* arg, void* keys, int B, int N, int taps, void* stamps,
                                    void* stream) {
  WideArgs a{};
  a.X = X; a.sXb = (long)128 * N; a.ldX = N;
  a.W = Wp; a.Wh = Wh; a.unscale = unscale; a.bias = bias;
  a.out = out; a.arg = arg; a.keys = (unsigned long long*)keys;
  a.Co = 1024; a.N = N; a.B = B; a.taps = taps;
  a.stamps = (unsigned long long*)stamps;
  return launch_wide_max(a, geoa3_stream(stream));
}
