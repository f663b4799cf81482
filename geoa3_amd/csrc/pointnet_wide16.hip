// conv5 (the trunk's 1024-wide layer: kernel 3, pad 1) on the 16x16x32 shape of the f16 matrix core (gfx950).
//
// Same arithmetic as pointnet_wide_split.hip (every fp32 operand as hi + lo fp16 values, a*w = a_hi*w_hi + a_hi*w_lo +
// a_lo*w_hi, fp32 accumulate, per-unit power-of-two activation scale), same keys / finalize; what changes is the MFMA
// shape: `v_mfma_f32_16x16x32_f16` takes the same cycles per flop as `32x32x16`, but the chip holds a
// higher clock on it under 16-bit matrix load (MI355X_MICROARCH.md, DVFS give-back item 7: 1.12-1.15x the FLOP/s at
// equal cycles).  Measured on MI355X: conv5 (K = 384 per channel group) 0.495 ms on the 32x32x16 kernel, 0.444 ms here;
// the T-Nets' conv3 (K = 128: a third of the MFMAs between two epilogues) goes the other way (0.182 ms there, 0.292 ms
// here) and runs there.
//
// Operand roles as before (rows = points, columns = channels): a wave owns 32 channels (two 16-channel tiles) x 128
// points (eight 16-point tiles), 16 accumulators of 4 registers.  A k-step covers 32 input channels:
//   A (activations, LDS): lane (p = lane & 15, q = lane >> 4) reads the 8 channels 32 s + 8 q .. + 7 of point row
//     16 t + p + tap (rows 0 and 129 hold the halo points n0 - 1 and n0 + 128): one ds_read_b128 per piece.  Rows are
//     288 bytes apart: with 2 p + q (mod 16) distinct over every 16-lane service group of a b128 read, the reads are
//     conflict free (272 bytes, the 32x32 layout's pitch, would put (p, q) and (p + 1, q - 1) on the same banks);
//   B (weights, L2 -> registers): fragments [T16 = co / 16][s = k / 32][piece][lane][8] = piece(w[16 T16 + (lane & 15)]
//     [32 s + 8 (lane >> 4) + j]) (geoa3_amd/pointnet.py pack_wide_split16), 64 bytes per lane and k-step, through a
//     two-step register ring that runs across the channel groups.
// The A fragments are double-buffered by HALF k-steps (four point tiles): the half just consumed is refilled for the next
// k-step while the other half's 24 MFMAs run.  The first MFMA of each accumulator takes a literal zero C operand (+0, what
// the 64 v_mov per channel group wrote before); the group's first PF k-steps are a copy of the loop body for that (conv5
// alone 417.4 -> 413.4 us, same bits: profiles/tnet_conv3_ab.txt).
//
// Unit schedule, staging pass, key hand-off and launcher are those of wide_unit.h, shared with the T-Net kernel: a tile
// is read, scaled, split and written to LDS once per unit.  (Until the unit was widened a tile's two channel halves were
// separate units and each staged the tile for itself: conv5 alone at B = 250, N = 1024 449.0 -> 428.9 us, same bits;
// NOTEBOOK 10, "conv5 dissected".)  This file's own: the two halo rows, staged between the shared pieces (one value
// per thread, part of the tile's maximum), and where the unit's 4 x 8 x 32 packed maxima wait for their atomicMax -- in
// the padding bytes of the image's rows: a second 8 KB array beside the 74,880-byte image would leave no room for two
// workgroups per CU.  The kernel sits at 256 registers and spills (4 VGPRs, 20 bytes per lane), but every scratch
// access lies in the staging part of the unit loop, none inside the channel-group or k loops.  (Sharing the pieces,
// whichever, cost the layer 1.5-2 us of 404 against the same statements in place, the group loop identical: NOTEBOOK 10.)
//
// Epilogue of a channel group (wide_epilogue.h): the lane's maximum first (v_max3_f32), then the lowest point whose
// accumulator equals it (one compare + one select per value, no branch), then the shuffles across the four lanes of a
// channel.  Points past the end of a ragged tile are set to -inf beforehand.  (The one-pass `(full || n < N) && x > v`
// scan it replaces had compiled to an exec-mask region with a branch per value: conv5 alone 442.3 -> 419.8 us, same bits;
// NOTEBOOK 10.  Running the next group's first k-step under the index scan was built as well and lost: NOTEBOOK 8 row 41.)
#include "pointnet_kernels.h"
#include "wide_epilogue.h"
#include "wide_unit.h"
#include <type_traits>

namespace {

constexpr int W16_OCC = 2;                        // workgroups per CU
constexpr int W16_ROWS = WIDE_PTS + 2;
constexpr int W16_ROWB = 288;
constexpr int W16_PIECEB = W16_ROWS * W16_ROWB;   // 37,440
constexpr int W16_LDS = 2 * W16_PIECEB;           // 74,880 B: two workgroups per CU

// Timing-only variant builds (tools/gpu_w16_dissect.sh, never the shipped library): a bit mask of phases compiled out.
//   1 = no staging (the LDS image is left as it is), 2 = no epilogue / keys, 4 = no weight-fragment loads (ring reused)
#ifndef GEOA3_W16_CUT
#define GEOA3_W16_CUT 0
#endif

__global__ __launch_bounds__(WIDE_THREADS, W16_OCC) void wide16_kernel(WideArgs a, int slots_per_xcd) {
  constexpr int TAPS = 3;
  constexpr int KS = TAPS * 4;               // k-steps of 32 per channel tile
  constexpr int PF = 2;                      // k-steps of weight fragments in flight
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ float s_max[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p16 = lane & 15, q4 = lane >> 4;
  // the unit's packed maxima (wide_flush) live in the 32 pad bytes of the image's rows (4 keys per row, 2 x 128 rows = the
  // 4 x 8 x 32 keys of a unit): neither the staging writes nor the A reads touch bytes 256..287 of a row
  auto key_slot = [&](int i, int l) {   // channel tile i (< WIDE_GROUPS) of this wave, channel l (< 32)
    const int k = (wave * WIDE_GROUPS + i) * 32 + l;
    unsigned char* row = smem_raw + (k >> 9) * W16_PIECEB + ((k >> 2) & 127) * W16_ROWB;
    return reinterpret_cast<unsigned long long*>(row + 256 + (k & 3) * 8);
  };
  const int N = a.N;
  const half8* Wall = reinterpret_cast<const half8*>(a.Wh);
  const WideSchedule sch = wide_schedule(a, slots_per_xcd, s_max);
  WidePending pend;
  auto flush = [&]() { wide_flush(pend, a, lane, key_slot); };
  for (int it = 0; it < sch.iterations(); ++it) {
    const WideUnit un = wide_unit(sch, it);
    const int b = un.b, n0 = un.n0, g_begin = un.g_begin, g_end = un.g_end;
    const float* X = a.X + (size_t)b * a.sXb;
    // ---- stage (wide_unit.h): rows 1..128 of the image = points n0 .. n0 + 127;
    // the two halo rows (points n0 - 1, n0 + 128): one value per thread
    float unscale = a.unscale;
    if (GEOA3_W16_CUT & 1) {
      flush();
      __syncthreads();
    } else {
      float xv[2][4][8], xhalo = 0.f;
      {
        int ldx = a.ldX;
        asm volatile("" : "+s"(ldx));   // opaque: see wide_load_tile
        wide_load_tile(X, ldx, n0, N, lane, wave, xv);
        const int nh = tid < 128 ? n0 - 1 : n0 + WIDE_PTS;
        if (nh >= 0 && nh < N) xhalo = X[(size_t)((tid & 127) * ldx) + nh];
      }
      const float m = wide_abs_max(xv, __builtin_fabsf(xhalo));
      flush();
      float scale;
      bool bad = wide_tile_scale(m, s_max, lane, wave, scale, unscale);
      unscale *= a.unscale;
      bad |= wide_split_store<W16_ROWB, W16_PIECEB>(xv, scale, smem_raw + W16_ROWB, lane, wave);
      {
        const float xs = xhalo * scale;
        bad |= xs != xs;
        _Float16 h, l;
        sf_split(xs, h, l);
        unsigned char* dst = smem_raw + (tid < 128 ? 0 : W16_ROWS - 1) * W16_ROWB + (tid & 127) * 2;
        *reinterpret_cast<_Float16*>(dst) = h;
        *reinterpret_cast<_Float16*>(dst + W16_PIECEB) = l;
      }
      wide_poison(a, b, bad);
    }
    // A operand of lane (p16, q4), point tile t, k-step s (tap = s / 4, ci0 = 32 (s % 4)):
    //   row 16 t + p16 + tap, bytes (ci0 + 8 q4) * 2
    const unsigned char* abase = smem_raw + p16 * W16_ROWB + q4 * 16;
    auto a_rd = [&](int s, int t, half8& h, half8& l) {
      const unsigned char* ap = abase + ((s >> 2) + 16 * t) * W16_ROWB + (s & 3) * 64;
      h = *reinterpret_cast<const half8*>(ap);
      l = *reinterpret_cast<const half8*>(ap + W16_PIECEB);
    };
    // weight fragments of the wave's channel tile c2 (< 2) of group g: [T16][s][piece][lane]
    auto wbase = [&](int g, int c2) {
      const int co = g * 128 + wave * 32 + 16 * c2;
      return Wall + (size_t)(co / 16) * KS * 2 * 64 + lane;
    };
    half8 wf[PF][2][2];
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const half8* W0 = wbase(g_begin, c2);
#pragma unroll
      for (int f = 0; f < PF; ++f) {
        wf[f][c2][0] = W0[(size_t)(2 * f) * 64];
        wf[f][c2][1] = W0[(size_t)(2 * f + 1) * 64];
      }
    }
    // A fragments of k-step 0: they do not depend on the channel group, so the last k-step of a group refills them for
    // the next one (the pre-loop reads were exposed once per group: 8 groups x 16 ds_read_b128 per T-Net unit)
    half8 Ah[2][4], Al[2][4];     // [half of the point tiles][tile within the half]
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int t = 0; t < 4; ++t) a_rd(0, 4 * hf + t, Ah[hf][t], Al[hf][t]);
#pragma unroll 1
    for (int g = g_begin; g < g_end; ++g) {
      const half8 *Wp[2], *Wn[2];
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        Wp[c2] = wbase(g, c2);
        Wn[c2] = wbase(g + 1 < g_end ? g + 1 : g, c2);
      }
      f32x4 acc[8][2];
      // PF k-steps from s0 on; FIRST: the group's first ones, whose first k-step starts from a zero C operand
      auto ksteps = [&](int s0, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
#pragma unroll
        for (int f = 0; f < PF; ++f) {
          const int s = s0 + f;
          const int sn = s + 1 < KS ? s + 1 : 0;          // the last step loads k-step 0 for the next channel group
          half8 wh[2], wl[2];
#pragma unroll
          for (int c2 = 0; c2 < 2; ++c2) {
            wh[c2] = wf[f][c2][0];
            wl[c2] = wf[f][c2][1];
            if (GEOA3_W16_CUT & 4) continue;
            const half8* src = s + PF < KS ? Wp[c2] + (size_t)(2 * 64) * (s + PF) : Wn[c2] + (size_t)(2 * 64) * (s + PF - KS);
            wf[f][c2][0] = src[0];
            wf[f][c2][1] = src[64];
          }
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int c2 = 0; c2 < 2; ++c2) {
                f32x4 c0 = acc[4 * hf + t][c2];
                if (FIRST && f == 0) c0 = f32x4{0.f, 0.f, 0.f, 0.f};
                acc[4 * hf + t][c2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[hf][t], wh[c2], c0, 0, 0, 0);
                acc[4 * hf + t][c2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[hf][t], wl[c2], acc[4 * hf + t][c2], 0, 0, 0);
                acc[4 * hf + t][c2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al[hf][t], wh[c2], acc[4 * hf + t][c2], 0, 0, 0);
              }
            __builtin_amdgcn_sched_barrier(0);
            // this half is consumed: refill it for the next k-step while the other half's MFMAs run
#pragma unroll
            for (int t = 0; t < 4; ++t) a_rd(sn, 4 * hf + t, Ah[hf][t], Al[hf][t]);
          }
        }
      };
      ksteps(0, std::true_type{});
#pragma unroll 1
      for (int s0 = PF; s0 < KS; s0 += PF) ksteps(s0, std::false_type{});
      // lane: channel co0 + 16 c2 + p16; acc[t][c2][r]: point n0 + 16 t + 4 q4 + r.  Ascending point order, strict >
      const bool full = n0 + WIDE_PTS <= N;
      if (GEOA3_W16_CUT & 2) {   // the accumulators stay live, nothing is reduced or published
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
          for (int c2 = 0; c2 < 2; ++c2) asm volatile("" ::"v"(acc[t][c2]));
        continue;
      }
      if (!full) {               // points past the end lose to every valid one (point n0 is valid and finite)
        const int left = N - n0 - 4 * q4;
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
          for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) acc[t][c2][r4] = 16 * t + r4 < left ? acc[t][c2][r4] : -__builtin_inff();
      }
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        float v;
        int col;
        wide_lane_first_max<32>([&](int i) { return acc[i >> 2][c2][i & 3]; }, [](int i) { return 16 * (i >> 2) + (i & 3); },
                                v, col);
        col += n0 + 4 * q4;
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const float ov = __shfl_xor(v, o, 64);
          const int oc = __shfl_xor(col, o, 64);
          const bool take = wide_merge_take(ov, oc, v, col);
          v = take ? ov : v;
          col = take ? oc : col;
        }
        if (lane < 16) *key_slot(g - g_begin, 16 * c2 + lane) = wide_key(v * unscale, col);
      }
    }
    if (GEOA3_W16_CUT & 2) continue;
    pend.b = b;
    pend.co = g_begin * 128 + wave * 32;
    pend.n = g_end - g_begin;
  }
  flush();
}

}  // namespace

int launch_wide_max_split16(const WideArgs& a, hipStream_t s) {
  return wide_launch(wide16_kernel, W16_LDS, W16_OCC, 3, GEOA3_PROF_CONV5, a, s);
}
