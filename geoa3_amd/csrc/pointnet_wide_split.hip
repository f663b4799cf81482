// The T-Nets' 1024-wide layer (conv3, one tap) of pointnet_wide.hip on the f16 matrix pipe with SPLIT fp32 operands
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
// Structure (differences from wide_max2_kernel): a work unit is (instance, 128-point tile, GROUPS x 128 channels); the
// activation tile is split while it is staged and stored POINT-major in LDS ([piece][point][128 ci] fp16, rows padded to
// 272 B), so the A operand of a k-step (8 consecutive ci of one point) is one conflict-free ds_read_b128; each wave owns
// CB x 32 channels x 128 points (4 point tiles per channel tile); the weight fragments stream from L2 (2 x 16 B per lane per
// channel tile and k-step of 16) through a register ring across the channel groups.  Keys and the finalize kernel are
// those of the fp32 path; the epilogue is the two-pass, branch-free first maximum of wide_epilogue.h (the lane's maximum
// over its 64 values, then the lowest point that equals it; ragged tiles masked to -inf first): the layer alone 188.0 ->
// 183.4 us against the one-pass compare / select chain, same bits (NOTEBOOK 10).
//
// The k loop's operand pipeline (NOTEBOOK 10, "T-Net conv3 dissected"; profiles/tnet_conv3_ab.txt):
//   A: the fragments of one whole k-step live in registers (4 point tiles x hi / lo = 8 x half8).  A tile's pair is refilled
//      for the NEXT k-step right behind the tile's own three MFMAs, so a read has the other three tiles' 9 MFMAs (~290
//      cycles) of cover -- the finest form of conv5's half-k-step refill, +16 registers (212 of 256, no scratch).  The
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
#include "profile.h"
#include "wide_epilogue.h"
#include <type_traits>

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_OCC = 2;                    // workgroups per CU
constexpr int SP_PTS = 128;                  // points per unit
constexpr int SP_ROWB = 272;                 // bytes per LDS row: 128 fp16 + 16 B pad (row stride = 4 banks mod 64)
constexpr int SP_PIECEB = SP_PTS * SP_ROWB;  // 34,816
constexpr int SP_LDS = 2 * SP_PIECEB;        // 69,632 B: two workgroups per CU

// Timing-only variant builds (tools/build_w16_variants.sh, never the shipped library): the bit mask of pointnet_wide16.hip's
// GEOA3_W16_CUT.  1 = no staging (the LDS image is left as it is, the barriers stay), 2 = no epilogue / keys, 4 = no
// weight-fragment loads (the ring is reused).  A cut build computes wrong values; it touches no byte the shipped kernel does not.
#ifndef GEOA3_WSP_CUT
#define GEOA3_WSP_CUT 0
#endif

__global__ __launch_bounds__(SP_THREADS, SP_OCC) void wide_split_kernel(WideArgs a, int slots_per_xcd) {
  constexpr int GROUPS = 8;                  // channel groups of 128 per unit
  // channel tiles of 32 per wave.  (Round 4: CB = 2 -- half the LDS reads per MFMA -- 186.2 against 185.2 us: LDS
  // bandwidth is not what holds this kernel at ~1.1-1.2 PF on the f16 pipe.)  The loops over c stay: the same loops
  // without them compile to other machine code (more scratch).
  constexpr int CB = 1;
  constexpr int KS = 8;                      // k-steps of 16 per channel tile
  constexpr int PF = 4;                      // k-steps of weight fragments in flight; KS % PF == 0
  constexpr int NBLK = KS / PF;              // blocks of PF k-steps
  constexpr int GSTEPS = GROUPS / CB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ float s_max[4];
  // packed maxima of the current unit, published (atomicMax) while the NEXT unit is being staged: keeps the atomics
  // out of the in-order vmcnt queue in front of the weight stream (on its own within run-to-run noise)
  __shared__ unsigned long long s_keys[4][GROUPS][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 5, l31 = lane & 31;
  const int N = a.N, tiles = (N + SP_PTS - 1) / SP_PTS;
  constexpr int SPLIT = 8 / GROUPS;
  const int per_inst = tiles * SPLIT;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int inst_x = (a.B - xcd + 7) / 8;
  const int units = inst_x * per_inst;
  const half8* Wall = reinterpret_cast<const half8*>(a.Wh);
  // The two workgroups that share a CU start together and do identical work.  The workgroup in the odd wave slot of its
  // SIMD (HW_ID.wave_id) runs half of its first unit's channel groups first and the other half at the very end (one extra
  // staging pass), which shifts its phases by half a period, so one workgroup's staging and epilogues run under the
  // other's MFMAs.  (s_memtime trace, tools/bench_wide.py --stamps: per unit 7 % waiting for the tile, 7 % splitting it,
  // 4 x 20.7 % channel groups of which 2 % epilogue.)  Worth 0-10 % depending on the device: the kernel sits at the
  // clock-limited ceiling of the 16-bit matrix pipe (1.25 PFLOP/s executed at 1.86 GHz, 66 % busy).
  if (tid == 0) s_max[0] = __int_as_float(__builtin_amdgcn_s_getreg((3 << 11) | 4) & 1);   // HW_REG_HW_ID[3:0]
  __syncthreads();
  bool late = __float_as_int(s_max[0]) != 0;
  const int nmine = units > slot ? (units - slot + slots_per_xcd - 1) / slots_per_xcd : 0;
  late = late && nmine > 0;
  int nstamp = 0;
  auto stamp = [&]() {   // diagnostic build only (a.stamps != null): wave 0 of workgroup 0 records s_memtime
    if (a.stamps && blockIdx.x == 0 && tid == 0 && nstamp < 255) a.stamps[1 + nstamp++] = __builtin_amdgcn_s_memtime();
  };
  int pend_b = -1, pend_co = 0, pend_n = 0;     // unit whose maxima wait in s_keys: instance, first channel, tiles
  auto flush = [&]() {
    if (pend_b < 0) return;
    for (int i = kh; i < pend_n; i += 2)       // the two half-waves publish two channel tiles per instruction
      atomicMax(a.keys + (size_t)pend_b * a.Co + pend_co + (i / CB) * (128 * CB) + (i % CB) * 32 + l31, s_keys[wave][i][l31]);
    pend_b = -1;
  };
  for (int it = 0; it < nmine + (late ? 1 : 0); ++it) {
    const int u = slot + (it == nmine ? 0 : it) * slots_per_xcd;
    const int g_begin = late && it == nmine ? GSTEPS / 2 : 0;
    const int g_end = late && it == 0 ? GSTEPS / 2 : GSTEPS;
    const int q = u / per_inst, r = u - q * per_inst;
    const int b = xcd + 8 * q, tile = r / SPLIT, half = r - tile * SPLIT;
    const int n0 = tile * SP_PTS;
    const float* X = a.X + (size_t)b * a.sXb;
    stamp();
    // ---- stage: every value of the tile goes through registers once: maximum -> scale -> split -> LDS.
    // Wave w takes the channel octets w, w+4, ..; a lane one point per pass (rows 0..127 of the image = points
    // n0 .. n0+127): 8 coalesced row reads per octet.
    float unscale = a.unscale;
    if (GEOA3_WSP_CUT & 1) {   // the barriers of the staging pass, none of its loads, arithmetic or LDS writes
      stamp();
      flush();
      __syncthreads();
      __syncthreads();
      __syncthreads();
    } else {
      float xv[2][4][8];
      {
        int ldx = a.ldX;
        asm volatile("" : "+s"(ldx));              // opaque: keeps the row offsets from being hoisted out of the unit
                                                   // loop (they were spilled to scratch)
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const int n = n0 + pass * 64 + lane;
          const bool in = n < N;
          const float* px = X + (in ? n : 0);
#pragma unroll
          for (int oc = 0; oc < 4; ++oc)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const float v = px[(size_t)(((wave + 4 * oc) * 8 + i) * ldx)];
              xv[pass][oc][i] = in ? v : 0.f;
            }
        }
      }
      float m = 0.f;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int oc = 0; oc < 4; ++oc)
#pragma unroll
          for (int i = 0; i < 8; ++i) m = fmaxf(m, __builtin_fabsf(xv[pass][oc][i]));   // NaN is caught through xs below
      m = wave_max(m);
      stamp();
      flush();           // the previous unit's maxima, behind this unit's loads
      __syncthreads();   // every wave is done with the previous tile (LDS image and s_max)
      if (lane == 0) s_max[wave] = m;
      __syncthreads();
      m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
      unsigned E = (__float_as_uint(m) >> 23) & 0xffu;
      bool bad = E == 255u;    // inf (a NaN does not survive fmaxf: caught below)
      E = sf_clamp(E);
      const float scale = sf_scale(E);
      unscale = a.unscale * sf_unscale(E);
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int p = pass * 64 + lane;
#pragma unroll
        for (int oc = 0; oc < 4; ++oc) {
          half8 hi, lo;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float xs = xv[pass][oc][i] * scale;
            bad |= xs != xs;
            _Float16 h, l;
            sf_split(xs, h, l);
            hi[i] = h;
            lo[i] = l;
          }
          unsigned char* dst = smem_raw + p * SP_ROWB + (wave + 4 * oc) * 16;
          *reinterpret_cast<half8*>(dst) = hi;
          *reinterpret_cast<half8*>(dst + SP_PIECEB) = lo;
        }
      }
      if (__syncthreads_or(bad))   // loud, not silently wrong: key ~0 decodes to NaN in wide_finalize_kernel
        for (int c = tid; c < a.Co; c += SP_THREADS) atomicMax(a.keys + (size_t)b * a.Co + c, ~0ull);
    }
    stamp();
    // A operand of lane (r = l31, h = kh), tile t, k-step s (ci0 = 16 s): row 32t + r, bytes (ci0 + 8h) * 2
    const unsigned char* abase = smem_raw + l31 * SP_ROWB + kh * 16;
    // fragments of the wave's channel tile c (< CB) of group step g: [T][s][piece][lane]
    auto wbase = [&](int g, int c) {
      const int co = (half * GROUPS + g * CB) * 128 + wave * 32 * CB + 32 * c;
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
      const bool full = n0 + SP_PTS <= N;
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
    pend_b = b;
    pend_co = (half * GROUPS + g_begin * CB) * 128 + wave * 32 * CB;
    pend_n = (g_end - g_begin) * CB;
  }
  flush();
  if (a.stamps && blockIdx.x == 0 && tid == 0) a.stamps[0] = nstamp;
}

}  // namespace

int launch_wide_max_split(const WideArgs& a, hipStream_t s) {
  if (a.Co != 1024 || a.taps != 1 || !a.keys || !a.Wh) return GEOA3_ENOSUPPORT;
  geoa3_prof_begin(GEOA3_PROF_TNETWIDE, s);
  if (!a.keys_clean &&
      hipMemsetAsync(a.keys, 0, (size_t)a.B * a.Co * sizeof(unsigned long long), s) != hipSuccess)
    return GEOA3_ELAUNCH;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(wide_split_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            SP_LDS);
  constexpr int SLOTS = 32 * SP_OCC;
  hipLaunchKernelGGL(wide_split_kernel, dim3(SLOTS * 8), dim3(SP_THREADS), SP_LDS, s, a, SLOTS);
  launch_wide_finalize(a, s);
  geoa3_prof_end(GEOA3_PROF_TNETWIDE, s);
  GEOA3_CHECK_LAUNCH();
  return GEOA3_OK;
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
