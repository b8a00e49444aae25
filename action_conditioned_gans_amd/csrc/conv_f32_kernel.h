// Kernel template of the fp32 MFMA implicit-GEMM convolution; see conv_f32.hip for the design notes.
// Included by conv_f32_{fwd,dgrad,wgrad}.hip, each of which instantiates one MODE (parallel compilation).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "conv_tile.h"

namespace acgconv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

// f(0), f(1), ... f(N-1) while f returns true; false as soon as one call does
template <int I, int N, class F>
__device__ __forceinline__ bool run_unrolled(F&& f) {
  if constexpr (I < N) {
    if (!f(std::integral_constant<int, I>{})) return false;
    return run_unrolled<I + 1, N>(f);
  } else {
    return true;
  }
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}
constexpr int BK = 32;  // k per K-step = 8 quads

// Branch-free guarded loads through buffer descriptors.  A divergent `if (ok) load` makes hipcc wait for every
// load inside its branch (vmcnt(0) per load: the loads of a K-step serialise), and selecting the loaded VALUE
// drags the wait up to the load as well.  Instead each operand tensor is addressed through a raw buffer
// resource (base + 32-bit byte offset, hardware range check): a masked lane gets an offset beyond the buffer
// and the load returns zeros without touching memory.  One v_cndmask on a 32-bit offset per load, no 64-bit
// pointer arithmetic, and every load of a stage issues back to back; the first wait is NST-1 K-steps later.
typedef unsigned u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 guarded_quad(__amdgpu_buffer_rsrc_t rs, int elem_off, bool ok) {
  const unsigned off = ok ? (unsigned)elem_off * 4u : kOob;
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}
// Ragged quad (channel count not a multiple of 4): only the first nvalid (1..3) elements exist.
__device__ __forceinline__ f4 guarded_ragged(__amdgpu_buffer_rsrc_t rs, int elem_off, bool ok, int nvalid) {
  f4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned off = (ok && e < nvalid) ? (unsigned)(elem_off + e) * 4u : kOob;
    r[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
  }
  return r;
}
__device__ __forceinline__ float guarded_scalar(__amdgpu_buffer_rsrc_t rs, int elem_off, bool ok) {
  const unsigned off = ok ? (unsigned)elem_off * 4u : kOob;
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
}

// ---- BatchNorm statistics of a tile, out of the accumulators -----------------------------------------------------------
// E[x^2] - E[x]^2 from plain float32 sums loses the variance once |mean| >> std (late GAN training: d/conv layers with a
// drifted mean).  So nothing here ever squares an uncentred value: a thread centres its rows of a column on the first of
// them, turns the result into (count, sum, M2 about its own mean), and partial results are merged pairwise with the
// parallel-variance formula (Chan, Golub, LeVeque): M2 = M2a + M2b + (mean_b - mean_a)^2 * na * nb / (na + nb).
struct TileStat { float n, sum, m2; };
__device__ __forceinline__ TileStat stat_merge(const TileStat a, const TileStat b) {
  const float n = a.n + b.n;
  const float ma = a.sum / fmaxf(a.n, 1.f), mb = b.sum / fmaxf(b.n, 1.f), d = mb - ma;
  return TileStat{n, a.sum + b.sum, a.m2 + b.m2 + d * d * (a.n * b.n / fmaxf(n, 1.f))};
}
// equal, non-zero counts (full tiles): no divisions by the counts
__device__ __forceinline__ TileStat stat_merge_equal(const TileStat a, const TileStat b) {
  const float d = (b.sum - a.sum) / a.n;
  return TileStat{a.n + b.n, a.sum + b.sum, a.m2 + b.m2 + d * d * (0.5f * a.n)};
}
// The epilogue step shared by the fp32 and the bf16 kernel.  `value(a, b, r)` = accumulator element as it will be stored;
// `red`: >= 3 * WM * BN floats of LDS that nothing reads any more (the A tiles after the K loop's last barrier).
template <int BM, int BN, int WM, int TA, int TB, class V>
__device__ __forceinline__ void tile_stats_epilogue(V&& value, float* red, float* out_sum, int N, int M, int m0, int n0, int wm0,
                                                    int wn0, int wr, int lrow, int lk, int tid) {
  const bool rows_full = m0 + BM <= M;                      // block-uniform: full tiles skip the per-element row test
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    TileStat t;
    if (rows_full) {
      const float c = value(0, b, 0);
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float d = value(a, b, r) - c; s1 += d; s2 += d * d; }
      constexpr float n = 16.f * TA;
      t = TileStat{n, n * c + s1, fmaxf(s2 - s1 * s1 * (1.f / n), 0.f)};
      const TileStat o{n, __shfl_xor(t.sum, 32, 64), __shfl_xor(t.m2, 32, 64)};
      t = stat_merge_equal(t, o);
    } else {
      float c = 0.f, n = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (m0 + row < M) {
            const float v = value(a, b, r);
            if (n == 0.f) c = v;
            const float d = v - c;
            n += 1.f; s1 += d; s2 += d * d;
          }
        }
      t = TileStat{n, n * c + s1, fmaxf(s2 - s1 * s1 / fmaxf(n, 1.f), 0.f)};
      const TileStat o{__shfl_xor(t.n, 32, 64), __shfl_xor(t.sum, 32, 64), __shfl_xor(t.m2, 32, 64)};
      t = stat_merge(t, o);
    }
    if (lk == 0) {
      float* const q = red + (wr * BN + wn0 + 32 * b + lrow) * 3;
      q[0] = t.n; q[1] = t.sum; q[2] = t.m2;
    }
  }
  __syncthreads();
  if (tid < BN && n0 + tid < N) {
    TileStat t{red[tid * 3], red[tid * 3 + 1], red[tid * 3 + 2]};
#pragma unroll
    for (int w = 1; w < WM; ++w) {
      const float* const q = red + (w * BN + tid) * 3;
      t = stat_merge(t, TileStat{q[0], q[1], q[2]});
    }
    out_sum[n0 + tid] = t.sum; out_sum[N + n0 + tid] = t.m2;
  }
}

// RAGGED: gathered channel count not a multiple of 4; NVEC: dense operand rows are float4-loadable (N % 4 == 0).
// Both are compile-time so that the slow variants never share registers (and waits) with the fast one.
// (bf16 tensors take their own kernel: conv_bf16_kernel.h.)
//
// Pipeline (one barrier per K-step): LDS holds TWO K-steps of both tiles.  In iteration ks a wave (1) drains the
// register stage of step ks+1 into the other LDS buffer, (2) runs the MFMAs of step ks out of the current buffer and
// (3) issues the global loads of step ks+NST into the stage that was drained one iteration earlier.
// What the measurements behind this shape say (tools/conv_kloop.py, tools/micro/*.hip, profiles/r1):
//  * v_mfma_f32_32x32x2_f32 runs on the SIMD's fp32 vector ALUs (MI355X quotes the same 157.3 TFLOP/s for fp32
//    vector and fp32 matrix): VALU instructions of ANY wave on the SIMD do not overlap it - SIMD time per K-step is
//    the SUM of the MFMA passes and every VALU instruction issued, whatever the occupancy; LDS instructions overlap
//    only partly (tools/micro/mfma_overlap.hip with 1, 2 and 4 waves per SIMD).  More resident blocks hide latency,
//    not issue cycles.  Hence a loader that costs as few VALU instructions as possible: running offsets instead of
//    divisions and multiplies, 32-bit mask tests, LDS lookups fetched once per iteration, row infos in registers;
//  * the loop body must be ONE basic block with a single predecessor per unrolled copy, every load predicated by an
//    out-of-range offset instead of a branch: only then does hipcc count outstanding loads exactly (vmcnt(N), N > 0)
//    and the loads really run NST-1 K-steps ahead;
//  * a chain of dependent MFMAs through one accumulator already issues every 68-74 cycles (no extra sets needed).
// The block program.  (bx, by, bz) / gx stand in for blockIdx / gridDim.x so that conv_pair_f32 below can run the blocks
// of two contractions out of one 1-D grid.
// LDS of one block program: two K-steps of both tiles, the row infos, the tap tables.
// (UW: the weight gradient's row table as three arrays of 2 x 256 words, see conv_body.)
template <int MODE, int BM, int BN, bool UW = false>
constexpr int conv_lds_bytes() {
  return 2 * 8 * (BM + BN) * (int)sizeof(f4) + (UW ? 3 * 2 * 256 * (int)sizeof(unsigned) : ((MODE == MODE_WGRAD) ? 2 * 256 : BM) * (int)sizeof(RowInfo)) +
         2 * kMaxTaps * (int)sizeof(int);
}

// LIN (FWD, !RAGGED, NVEC): the gathered channel count is a multiple of 4 (Cs == Cp), so filter row k of W[(tap, c)][n] is
// row k of the [Kdim][N] matrix - the dense operand needs no (tap, channel) state (conv_body: run_boff).
//
// UK (FWD with LIN, or DGRAD; !RAGGED, NVEC): the gathered channel count is a multiple of BK, so a K-step lies inside ONE tap and
// everything the loaders derive from k - tap, channel origin, tap-table entries, `live`, the dense row offset - is the same for
// every lane of the block.  That state then lives in scalar registers and reaches the loads through the buffer descriptors (base
// moved by the step's uniform offset, zero records for a dead step); a lane keeps loop-invariant byte offsets and spends its
// VALU on the tap-mask test alone.  Same loads into the same LDS slots as the generic loaders: results are bit-identical.
//
// UW (WGRAD; !RAGGED, NVEC): the weight gradient's counterpart.  Its gathered ROWS change every K-step, so what goes to the scalar
// side is the rest: `live` and the dense row origin reach the loads through the descriptors (dY rows at or beyond Kdim and dead steps
// fall to the hardware range check), a lane keeps loop-invariant byte offsets, and a gathered row costs its offset plus the mask
// test.  The row table holds byte offsets and complemented masks as three word arrays, written UNR K-steps at a time by
// straight-line code in ONE fixed unrolled copy of the loop and read at compile-time slots.  Same loads, same LDS slots, same bits.
#ifndef ACG_NST
#define ACG_NST 3      // whole-step sweep: 2 -> 339.5, 3 -> 349, 4 -> 344, 5 -> 340 steps/s
#endif
template <int MODE, int BM, int BN, int WM, int WN, bool RAGGED, bool NVEC, bool EPI = false, bool LIN = false, bool UK = false, bool UW = false>
__device__ __forceinline__ void conv_body(const ConvArgs& p, const int bx, const int by, const int bz, const int gx, char* smem) {
  static_assert(WM * WN == 4, "4 waves per block");
  constexpr int TA = BM / (32 * WM), TB = BN / (32 * WN);
  constexpr int QA = BM / 32, QB = BN / 32;  // quads per thread per K-step
  constexpr int NROW = (MODE == MODE_WGRAD) ? 2 * 256 : BM;  // WGRAD: row infos of 2 x 8 K-steps (chunk parity)
  constexpr int NST = ACG_NST;           // register stages: global loads run NST K-steps ahead of their MFMAs
  constexpr int UNR = (NST % 2 == 0) ? NST : 2 * NST;      // the K-loop's unroll: (stage, LDS buffer) repeat with period lcm(NST, 2)

  constexpr int KSLOTS = 8;              // 16-byte k-slots (quads) per tile column
  constexpr int ASZ = KSLOTS * BM, BSZ = KSLOTS * BN;
  constexpr int ROWB = UW ? 3 * 2 * 256 * (int)sizeof(unsigned) : NROW * (int)sizeof(RowInfo);
  static_assert(conv_lds_bytes<MODE, BM, BN, UW>() == (2 * ASZ + 2 * BSZ) * (int)sizeof(f4) + ROWB + 2 * kMaxTaps * (int)sizeof(int), "LDS layout");
  static_assert(!UW || BM != 64 || BN != 64 || conv_lds_bytes<MODE, BM, BN, UW>() + 8 <= 40960, "UW 64x64: four blocks per CU, also beside compact_taps' two words in conv_pair_f32");
  f4* const As_all = reinterpret_cast<f4*>(smem);                         // [2 * ASZ]
  f4* const Bs_all = As_all + 2 * ASZ;                                    // [2 * BSZ]
  RowInfo* const rows = reinterpret_cast<RowInfo*>(Bs_all + 2 * BSZ);     // [NROW]
  // UW: [3][2][256] words - byte offset, ~mask_lo, ~mask_hi of the rows of two chunks of UNR K-steps (chunk parity)
  char* const uw_tab = reinterpret_cast<char*>(Bs_all + 2 * BSZ);
  int* const tapA = reinterpret_cast<int*>(uw_tab + ROWB);                // [kMaxTaps]
  int* const tapB = tapA + kMaxTaps;                                      // [kMaxTaps]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gsrc), 0, p.g_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dense), 0, p.d_bytes, 0x00020000);

  // ---- problem geometry, tap tables, per-row gather info (conv_tile.h) ---------------------------------
  constexpr bool COMPACT = MODE != MODE_WGRAD;      // small maps: pixel-major rows, dead taps dropped (ConvArgs::compact)
  TileGeom g = tile_geometry<MODE, F32Tensors>(p, bx, by, gx, BM, BN);
  if (g.empty) return;  // block-uniform: DGRAD classes smaller than class 0
  fill_taps<MODE, F32Tensors>(p, g, tapA, tapB, tid);
  if constexpr (MODE != MODE_WGRAD) {
    for (int r = tid; r < BM; r += 256) rows[r] = row_info<MODE, F32Tensors, COMPACT>(p, g, g.m0 + r, g.M);
  }
  __syncthreads();
  if constexpr (COMPACT) {
    if (p.compact) { g.ntaps = compact_taps<BM>(g.ntaps, rows, tapA, tapB, tid); g.Kdim = g.ntaps * g.Cp; }      // block-uniform
  }
  // Cs: channels of the gathered tensor; Cp: Cs padded to a multiple of 4 (quad granularity per tap).
  const int M = g.M, N = g.N, Kdim = g.Kdim, Cs = g.Cs, Cp = g.Cp, ntaps = g.ntaps;
  const int tm = g.tm, m0 = g.m0, n0 = g.n0;
  const int NS = p.K;      // floats between two rows of the dense operand (FWD: filter rows W[(tap, c)][0..K))
  const KRange kr = split_range((Kdim + BK - 1) / BK, p.splits, bz);
  const int ks_begin = kr.begin, ks_end = kr.end;

  // ---- loaders: NST register stages ---------------------------------------------------------------
  // k-fast operands (A of FWD/DGRAD, B of DGRAD) are gathered one quad per (row, k/4); the others
  // (B of FWD, A and B of WGRAD) are contiguous along the tile column, so a thread loads a 4x4 block
  // (4 k-rows x float4 of columns) and transposes it in registers into 4 quads.
  // Transposed loaders: the 32 x (BN/4) row-quads of a K-step are dealt evenly to the 256 threads - LPB = BN/32
  // consecutive k-rows (4, 2 or 1) of one column quad each, i.e. a whole, half or quarter 4x4 block - so every
  // thread runs the same instruction stream (no idle waves, no divergent branch in the loop) and the transposed
  // pieces are written as 16-, 8- or 4-byte parts of the k-quads in LDS.
  constexpr int LPA = BM / 32, LPB = BN / 32;
  static_assert(!LIN || (MODE == MODE_FWD && NVEC && !RAGGED), "LIN: float4-able forward contraction");
  static_assert(!UK || (NVEC && !RAGGED && (MODE == MODE_DGRAD || (MODE == MODE_FWD && LIN))), "UK: FWD LIN or DGRAD, 16-byte gathers");
  static_assert(!UW || (MODE == MODE_WGRAD && NVEC && !RAGGED && !UK), "UW: weight gradient with 16-byte loads on both sides");
  static_assert(!UW || (NST == 3 && UNR * BK <= 256), "UW: the row-table schedule below is written for three stages (a chunk of 6 K-steps, one row per thread)");
  // (Filter rows as column quads - a thread owns one column and fetches the four k-rows of a quad with four dword loads off
  // one offset register, so the quad arrives in LDS order without a register transpose - was measured on top of LIN: 31.5
  // instead of 36.8 VALU instructions per K-step but 10 instead of 4 VMEM instructions, 404.4 vs 406.0 steps/s: dropped.)
  constexpr int RA = (MODE == MODE_WGRAD) ? LPA : QA;
  constexpr int RB = (MODE == MODE_DGRAD) ? QB : (NVEC ? LPB : QB);
  f4 ra[NST][RA], rb[NST][RB];

  // (tap, channel) of a k index by multiply-high: the loaders are straight-line code (no running state, no loops)
  auto tap_of = [&](int kp, int& t, int& c) { t = div_fast(kp, p.mg_cp, p.sh_cp); c = kp - t * Cp; };
  // transposed loaders: thread -> (column quad jn, k quad kq); active while kq < 8
  const int jb = tid % (BN / 4), r0b = (tid / (BN / 4)) * LPB, kqb = r0b >> 2, subb = r0b & 3;
  constexpr bool nvec = NVEC;         // dense rows are 16-byte aligned and quads never straddle N
  const int ja = tid % (BM / 4), r0a = (tid / (BM / 4)) * LPA, kqa = r0a >> 2, suba = r0a & 3;
  int wg_t = 0, wg_off = 0, wg_nvalid = 0;   // WGRAD: this thread's fixed (padded) output-row quad -> (tap, channel)
  if constexpr (MODE == MODE_WGRAD) {
    const int mp = m0 + 4 * ja;
    if (mp < M) {
      wg_t = mp / Cp;
      const int c = mp - wg_t * Cp;
      wg_nvalid = Cs - c;            // >= 1
      wg_off = tapA[wg_t] + c;
    }
  }


  constexpr bool ragged = RAGGED;     // quads at the end of a tap are partial

  // `live` false (a step beyond this block's K range): every lane addresses out of range, the loads return zeros
  // without touching memory - the loop body stays branch-free, so hipcc counts outstanding loads exactly
  // (s_waitcnt vmcnt(N), N > 0) instead of draining them at every control-flow join.
  // The loads of a K-step are NLD independent "pieces" (A pieces first, then B) so that the K-loop can deal them out
  // between MFMAs; shared address arithmetic is written per piece and merged by the compiler.
  constexpr int NLD = RA + RB;
  // Everything a K-step's loads need from LDS (tap table entry, WGRAD row infos) is fetched by load_prep at the top
  // of an iteration, so no piece waits on an LDS round trip between two MFMAs; the row infos of the k-fast gathers
  // never change and live in registers.
  RowInfo myrow[MODE == MODE_WGRAD ? 1 : QA];
  if constexpr (MODE != MODE_WGRAD) {
#pragma unroll
    for (int u = 0; u < QA; ++u) myrow[u] = rows[(tid >> 3) + 32 * u];
  }
  // Running (tap, channel) state of this thread's k-fast quad and dense rows, advanced by one K-step (32 k) per
  // load_prep call with adds and ONE conditional wrap (32 = step_t * Cp + step_c with step_c < Cp): the K-loop has
  // no division, no multiply and no 64-bit arithmetic.  load_prep must therefore be called for consecutive ks,
  // starting at ks_begin - which is how the pipeline below issues its loads.
  const int step_t = BK / Cp, step_c = BK - step_t * Cp;
  int run_kt = 0, run_kc = 0, run_bt = 0, run_bc = 0, run_boff = 0;
  if constexpr (MODE != MODE_WGRAD) tap_of(ks_begin * BK + 4 * (tid & 7), run_kt, run_kc);
  const int nB = n0 + 4 * jb;                       // first column of the dense-row quads (nvec)
  // LIN: the filter rows are linear in k, one running offset, valid while k < Kdim.
  int run_bk = 0;                                   // LIN: k of this thread's first dense row
  if constexpr (LIN) {
    run_bk = ks_begin * BK + r0b;
    run_boff = run_bk * NS + nB;
  } else if constexpr (MODE == MODE_FWD && nvec) {
    tap_of(ks_begin * BK + 4 * kqb, run_bt, run_bc);
    run_boff = (run_bt * Cs + run_bc + subb) * NS + nB;
  }
  if constexpr (MODE == MODE_WGRAD && nvec) run_boff = (ks_begin * BK + r0b) * p.Ky + nB;
  int nK[MODE == MODE_DGRAD ? QB : 1];                                     // DGRAD: n * K of this thread's filter rows
  bool nOk[MODE == MODE_DGRAD ? QB : 1];
  if constexpr (MODE == MODE_DGRAD) {
#pragma unroll
    for (int u = 0; u < QB; ++u) { const int n = n0 + (tid >> 3) + 32 * u; nK[u] = n * p.K; nOk[u] = n < N; }
  }
  // UK: (tap, channel origin) of the K-step in scalar registers - kernel arguments, block indices and the loop counter only -
  // and per lane what never changes in the loop: the byte offset of each gathered row-quad and of each dense quad (kOob where
  // the lane's column does not exist) and the complement of the row's tap mask.  The tap tables sit in one VGPR each, entry t
  // in lane t (kMaxTaps = the 64 lanes of a wave), so a step fetches its entry with v_readlane instead of an LDS round trip.
  // Nothing here relies on how the hardware treats soffset in its range check: the step's uniform offset moves the BASE of the
  // descriptor (64-bit scalar adds) and shrinks its record count by the same bytes, so the check stays "voffset + 16 <=
  // records" with soffset 0, exactly the test the generic loaders pass.  uk_shift makes every lane offset non-negative: FWD
  // rows start up to (pt, pl) pixels in front of the tensor (RowInfo::base < 0), so the lane offsets are taken relative to
  // that corner and the descriptor base moves back by as much; a descriptor base in front of the tensor is never
  // dereferenced, because a lane whose tap reads inside the tensor lands inside it and every other lane is masked.
  // (Host side, uniform_k_variant: both operands and the corner are at most 2^29 bytes, so a record count stays below 2^31,
  // the byte arithmetic of a step fits 32 bits, and the masked offsets - kOob, or a lane offset with bit 31 set - are beyond it.)
  static_assert(kMaxTaps == 64, "UK: a tap table per wave register");
  int uk_t = 0, uk_c0 = 0, uk_shift = 0, uk_tabA = 0, uk_tabB = 0;
  unsigned uk_va[UK ? QA : 1], uk_inv_lo[UK ? QA : 1], uk_inv_hi[UK ? QA : 1], uk_vb[(UK || UW) ? RB : 1];
  if constexpr (UK) {
    const int k0 = ks_begin * BK;
    uk_t = div_fast(k0, p.mg_cp, p.sh_cp); uk_c0 = k0 - uk_t * Cp;
    uk_shift = MODE == MODE_FWD ? (p.pt * p.W + p.pl) * p.Cx : 0;
    uk_tabA = tapA[lane];
    if constexpr (MODE == MODE_DGRAD) uk_tabB = tapB[lane];
#pragma unroll
    for (int u = 0; u < QA; ++u) {
      uk_va[u] = (unsigned)(myrow[u].base + uk_shift + 4 * (tid & 7)) * 4u;
      uk_inv_lo[u] = ~myrow[u].mask_lo; uk_inv_hi[u] = ~myrow[u].mask_hi;
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      if constexpr (MODE == MODE_DGRAD) uk_vb[u] = nOk[u] ? (unsigned)(nK[u] + 4 * (tid & 7)) * 4u : kOob;
      else uk_vb[u] = nB < N ? (unsigned)((r0b + u) * NS + nB) * 4u : kOob;
    }
  }
  // UW.  Gathered side: a row's table entry is its byte offset from the padding corner (uk_shift, as in UK: never negative) and
  // its complemented mask; the lane adds uw_lane = its (tap, channel quad) in bytes - 2^31 where its output rows do not exist, so
  // it stays masked whatever the row - and ors in bit wg_t of the complement, moved to bit 31 (shift uw_sh; the lo / hi word is
  // chosen once, by the table address uw_rm).  Offsets stay below 2^31 + 2^30 * 1.5: masked ones are beyond every record count
  // and short of wrapping.  The gathered descriptor starts at the corner and has zero records in a dead step; the dense one starts
  // at the step's first dY row and ends at row Kdim (uw_dlim).  uw_ro / uw_rm: byte positions in uw_tab of this thread's reads
  // (offset array; its mask word's array) in the table half of the chunk a round of the unrolled loop starts in ([0]) and in the
  // other half ([1]).  They are set at the top of a round from the round's number - no state is carried around the loop.
  constexpr unsigned UW_ARR = 2 * 256 * sizeof(unsigned), UW_HALF = 256 * sizeof(unsigned);
  unsigned uw_lane = 0, uw_sh = 0, uw_ro[2] = {0, 0}, uw_rm[2] = {0, 0}, uw_half = 0, uw_dlim = 0;
  unsigned long long uw_rep = 0ull;
  if constexpr (UW) {
    uk_shift = (p.pt * p.W + p.pl) * p.Cx;
    uw_lane = wg_nvalid > 0 ? (unsigned)wg_off * 4u : 0x80000000u;
    uw_sh = 31u - ((unsigned)wg_t & 31u);
    uw_ro[0] = (unsigned)r0a * 4u; uw_rm[0] = uw_ro[0] + (wg_t < 32 ? 1u : 2u) * UW_ARR;      // (prologue: chunk 0 in half 0)
    uw_rep = tap_rep(p.KH, p.KW);
    const unsigned long long dend = (unsigned long long)Kdim * (unsigned long long)p.Ky * 4ull;
    uw_dlim = dend < (unsigned long long)p.d_bytes ? (unsigned)dend : p.d_bytes;
#pragma unroll
    for (int u = 0; u < RB; ++u) uk_vb[u] = nB < N ? (unsigned)((r0b + u) * p.Ky + nB) * 4u : kOob;
  }
#ifdef ACG_NORM_PROBE
  // COST PROBE (tools only, `make probe`; never in the shipped library): what normalise-on-load would add to the loaders -
  // act((x - mean) * rstd + beta) on every GATHERED element on its way into LDS, zero padding applied after the activation.
  // Parameters that leave the values unchanged (scale 1, shift 0, floor -inf) come from LDS so that nothing folds away;
  // the in-bounds flag of every gathered quad is carried from its load to its store, as the real thing would have to.
  __shared__ f4 probe_par[3][16];
  if (tid < 16) { probe_par[0][tid] = f4{1.f, 1.f, 1.f, 1.f}; probe_par[1][tid] = f4{0.f, 0.f, 0.f, 0.f}; probe_par[2][tid] = f4{-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f}; }
  bool probe_ok[NST][RA];
  f4 probe_s = {1.f, 1.f, 1.f, 1.f}, probe_t = {0.f, 0.f, 0.f, 0.f}, probe_lo = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
  __syncthreads();
  if constexpr (MODE == MODE_WGRAD) { probe_s = probe_par[0][tid & 15]; probe_t = probe_par[1][tid & 15]; probe_lo = probe_par[2][tid & 15]; }   // a thread's channel quad is fixed
  auto probe_apply = [&](f4 q, const f4& ps, const f4& pt, const f4& pl, bool ok) {
    f4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float z = fmaf(q[e], ps[e], pt[e]); r[e] = ok ? fmaxf(z, pl[e]) : 0.f; }
    return r;
  };
#endif
  struct Prep {
    int t, kc, aoff, tb, bt, bc, boff, brow;
    bool kv;
    RowInfo wri[MODE == MODE_WGRAD ? LPA : 1];
    const float* ug; const float* ud;      // UK: the step's descriptor bases and record counts (scalar registers)
    unsigned ug_bytes, ud_bytes;
    unsigned uoff[UW ? LPA : 1], uinv[UW ? LPA : 1];      // UW: table entries of the step's rows (this lane's mask word)
  };
  // UK: descriptor base `ptr + off` (elements; may lie in front of the tensor, see above) and what is left of `bytes` behind it
  auto uk_window = [](const float* ptr, unsigned bytes, int off, bool on, const float*& base, unsigned& left) {
    const int ob = off * 4, rem = (int)bytes - ob;      // 32-bit (uniform_k_variant: |ob| and bytes are at most 2^29): scalar compares only
    base = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(ptr) + (uintptr_t)(long long)ob);
    left = (on && rem > 0) ? (unsigned)rem : 0u;
  };
  // sc, wc (UW only): the step's slot in its row-table chunk, (ks - ks_begin) % UNR, and whether that chunk is the one behind
  // the chunk the round started in - compile-time constants of the unrolled copy
  auto load_prep = [&](int ks, bool live, auto sc, auto wc) {
    Prep q{};
    if constexpr (UW) {
      constexpr int S = decltype(sc)::value, W = decltype(wc)::value;
      typedef unsigned urow __attribute__((ext_vector_type(LPA)));
      const urow o = *reinterpret_cast<const urow*>(uw_tab + uw_ro[W] + S * BK * 4);
      const urow m = *reinterpret_cast<const urow*>(uw_tab + uw_rm[W] + S * BK * 4);
#pragma unroll
      for (int e = 0; e < LPA; ++e) { q.uoff[e] = o[e]; q.uinv[e] = m[e]; }
      uk_window(p.gsrc, p.g_bytes, -uk_shift, live, q.ug, q.ug_bytes);
      uk_window(p.dense, uw_dlim, ks * (BK * p.Ky), live, q.ud, q.ud_bytes);      // rows at or beyond Kdim: beyond the record count
      return q;
    }
    if constexpr (UK) {
      q.kv = live && uk_t < ntaps;
      q.t = q.kv ? uk_t : 0;
      const int ta = __builtin_amdgcn_readlane(uk_tabA, q.t);
      uk_window(p.gsrc, p.g_bytes, ta + uk_c0 - uk_shift, q.kv, q.ug, q.ug_bytes);
      if constexpr (MODE == MODE_DGRAD) uk_window(p.dense, p.d_bytes, __builtin_amdgcn_readlane(uk_tabB, q.t) + uk_c0, q.kv, q.ud, q.ud_bytes);
      else uk_window(p.dense, p.d_bytes, ks * (BK * NS), live, q.ud, q.ud_bytes);      // LIN: filter row ks * BK; live => the step lies below Kdim (a multiple of BK)
      uk_t += step_t; uk_c0 += step_c;
      const bool wrap = uk_c0 >= Cp;
      uk_c0 -= wrap ? Cp : 0; uk_t += wrap ? 1 : 0;
      return q;
    }
    if constexpr (MODE == MODE_WGRAD) {
#pragma unroll
      for (int e = 0; e < LPA; ++e) q.wri[e] = rows[((ks - ks_begin) & 15) * BK + r0a + e];
    } else {
      q.kc = run_kc;
      q.kv = live && run_kt < ntaps;
      q.t = q.kv ? run_kt : 0;
      q.aoff = tapA[q.t] + run_kc;
      if constexpr (MODE == MODE_DGRAD) q.tb = tapB[q.t] + run_kc;
      run_kt += step_t; run_kc += step_c;
      const bool wrap = run_kc >= Cp;
      run_kc -= wrap ? Cp : 0; run_kt += wrap ? 1 : 0;
    }
    if constexpr (LIN) {
      q.boff = run_boff; q.brow = run_bk;
      run_boff += BK * NS; run_bk += BK;
    } else if constexpr (MODE == MODE_FWD && nvec) {
      // (tap, channel) state + the tap's first filter row from the table: the taps of a compacted tile are not consecutive
      q.bt = run_bt; q.bc = run_bc + subb; q.boff = tapB[min(run_bt, ntaps - 1)] + (run_bc + subb) * NS + nB;
      run_bt += step_t; run_bc += step_c;
      const bool wrap = run_bc >= Cp;
      run_bc -= wrap ? Cp : 0; run_bt += wrap ? 1 : 0;
    }
    if constexpr (MODE == MODE_WGRAD && nvec) {
      q.boff = run_boff; q.brow = ks * BK + r0b;
      run_boff += BK * p.Ky;
    }
    return q;
  };
  auto load_piece = [&](auto stage, int ks, bool live, const Prep& q, auto pc) {
    constexpr int ST = decltype(stage)::value;
    constexpr int I = decltype(pc)::value;
    if constexpr (UW) {
      if constexpr (I < RA) {      // raw rows now; the transpose happens at store time
        const unsigned dead = (q.uinv[I] << uw_sh) & 0x80000000u;
#ifdef ACG_NORM_PROBE
        probe_ok[ST][I] = live && dead == 0u && uw_lane < 0x80000000u;
#endif
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q.ug), 0, q.ug_bytes, 0x00020000);
        ra[ST][I] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (q.uoff[I] + uw_lane) | dead, 0, 0));
      } else {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q.ud), 0, q.ud_bytes, 0x00020000);
        rb[ST][I - RA] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, uk_vb[I - RA], 0, 0));
      }
    } else if constexpr (UK) {
      if constexpr (I < RA) {
        // the one per-lane decision left: is the step's tap inside the tensor for this row?  bit t of the complemented mask,
        // moved to bit 31, turns the lane offset of a dead tap into one of 2^31 or more: beyond any record count, and still
        // 16 bytes short of wrapping
        const unsigned inv = q.t < 32 ? uk_inv_lo[I] : uk_inv_hi[I];
        const unsigned dead = (inv << (31u - ((unsigned)q.t & 31u))) & 0x80000000u;
#ifdef ACG_NORM_PROBE
        probe_ok[ST][I] = q.kv && dead == 0u;
#endif
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q.ug), 0, q.ug_bytes, 0x00020000);
        ra[ST][I] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, uk_va[I] | dead, 0, 0));
      } else {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q.ud), 0, q.ud_bytes, 0x00020000);
        rb[ST][I - RA] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, uk_vb[I - RA], 0, 0));
      }
    } else if constexpr (I < RA) {
      if constexpr (MODE == MODE_WGRAD) {   // raw rows now; the transpose happens at store time
        const RowInfo ri = q.wri[I];
        const bool ok = live && wg_nvalid > 0 && tap_ok(ri, wg_t);
#ifdef ACG_NORM_PROBE
        probe_ok[ST][I] = ok;
#endif
        if constexpr (!ragged) ra[ST][I] = guarded_quad(rs_g, ri.base + wg_off, ok);
        else ra[ST][I] = guarded_ragged(rs_g, ri.base + wg_off, ok, wg_nvalid);
      } else {
        // k-fast gather: 8 consecutive lanes walk 8 quads (128 contiguous bytes) of one gathered row
        const RowInfo ri = myrow[I];
#ifdef ACG_NORM_PROBE
        probe_ok[ST][I] = q.kv && tap_ok(ri, q.t);
#endif
        if constexpr (!ragged) ra[ST][I] = guarded_quad(rs_g, ri.base + q.aoff, q.kv && tap_ok(ri, q.t));
        else ra[ST][I] = guarded_ragged(rs_g, ri.base + q.aoff, q.kv && tap_ok(ri, q.t), Cs - q.kc);
      }
    } else {
      constexpr int U = I - RA;
      if constexpr (MODE == MODE_DGRAD) {  // B[k=(tap,o)][n=c] = W[tap][c][o], contiguous along o
        if constexpr (!ragged) rb[ST][U] = guarded_quad(rs_d, q.tb + nK[U], q.kv && nOk[U]);
        else rb[ST][U] = guarded_ragged(rs_d, q.tb + nK[U], q.kv && nOk[U], Cs - q.kc);
      } else if constexpr (nvec) {
        // dense operand: FWD W[(tap,c)][n] rows, WGRAD dY[(b,p,q)][n] rows; raw row, transposed at store time
        bool ok;
        if constexpr (LIN) ok = q.brow < Kdim;          // the LPB rows of a thread lie in one k-quad; Kdim % 4 == 0
        else if constexpr (MODE == MODE_FWD) ok = q.bt < ntaps && q.bc + U < Cs;
        else ok = q.brow + U < Kdim;
        rb[ST][U] = guarded_quad(rs_d, q.boff + U * (MODE == MODE_WGRAD ? p.Ky : NS), live && ok && nB < N);
      } else {  // ragged N (25, 5, 3, 1 ...): 4 k-rows of one column per quad, lanes along n
        constexpr int stepB = 256 / BN;
        const int n = n0 + (tid % BN), kq = tid / BN + stepB * U;
        f4 v;
        if constexpr (MODE == MODE_FWD) {
          int t2, c2;
          tap_of(ks * BK + 4 * kq, t2, c2);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] = guarded_scalar(rs_d, tapB[min(t2, ntaps - 1)] + (c2 + e) * NS + n, live && t2 < ntaps && c2 + e < Cs && n < N);
        } else {
          const int r = ks * BK + 4 * kq;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = guarded_scalar(rs_d, (r + e) * p.Ky + n, live && r + e < Kdim && n < N);
        }
        rb[ST][U] = v;
      }
    }
  };
  auto load_tiles = [&](auto stage, int ks, bool live) {
    const Prep q = load_prep(ks, live, stage, std::integral_constant<int, 0>{});      // (prologue: stage J holds step ks_begin + J = slot J of chunk 0)
    static_for<0, NLD>([&](auto pc) { load_piece(stage, ks, live, q, pc); });
  };

  // LDS column permutation: physical = P(col) ^ kq with P(32q + 4j + e) = 32q + 8e + (j ^ 4(e>>1)).
  // Conflict-free for (i) k-fast stores (8 lanes: one column, kq = 0..7), (ii) transposed stores (8 lanes:
  // columns 4j+e for 8 consecutive j) and (iii) the MFMA operand reads (32 consecutive columns, one kq).
  auto pcol = [](int col, int kq) {
    const int j = (col >> 2) & 7, e = col & 3;
    return ((col & ~31) | (e << 3) | (j ^ ((e >> 1) << 2))) ^ kq;
  };

  // write quad `kq` of tile column `col`
  auto put = [&](f4* tile, int width, int kq, int col, const f4& q) { tile[kq * width + pcol(col, kq)] = q; };

  // write k-rows sub..sub+L-1 of quad `kq` of tile column `col` (L = 4, 2, 1: a whole, half or quarter quad)
  // The values of a part come from L different load registers.  A ds_write_b64 wants them in a consecutive register pair, which
  // costs one v_mov per value in the K-loop; ds_write2_b32 takes its two dwords from any two registers (same LDS slots, same
  // bytes, same bank pattern), so the half quad is stored with it, in inline assembly: written as two float stores the compiler
  // proves the 8-byte alignment and re-forms the b64 store together with the moves.  The compiler's wait-count insertion does
  // not see LDS traffic issued from inline assembly: lds_pair_wait() below is what orders these stores before the barrier.
  // The whole quad (L == 4, the gathered side of a 128-row weight gradient) keeps its ds_write_b128 and its 16 moves: as two
  // ds_write2_b32 per column the 128x32 weight gradients measured slower (profiles/lds_pair_store).
  // ACG_LDS_PAIR_B64 (tools only, `make pairb64`; never in the shipped library) keeps the paired store for A/B runs.
#ifdef ACG_LDS_PAIR_B64
  constexpr bool PAIR_ASM = false;
#else
  constexpr bool PAIR_ASM = true;
#endif
  constexpr bool ASM_STORES = PAIR_ASM && ((MODE == MODE_WGRAD && LPA == 2) || (MODE != MODE_DGRAD && NVEC && LPB == 2));      // store_tiles issues some
  auto put_part = [&](f4* tile, int width, int kq, int sub, int col, auto lc, const float* v) {
    constexpr int L = decltype(lc)::value;
    char* dst = reinterpret_cast<char*>(tile + kq * width + pcol(col, kq)) + sub * 4;
    if constexpr (L == 4) *reinterpret_cast<f4*>(dst) = f4{v[0], v[1], v[2], v[3]};
    else if constexpr (L == 2 && PAIR_ASM) {
      const unsigned at = (unsigned)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)dst);      // LDS byte address
      asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" : : "v"(at), "v"(v[0]), "v"(v[1]) : "memory");
    } else if constexpr (L == 2) *reinterpret_cast<f2*>(dst) = f2{v[0], v[1]};
    else *reinterpret_cast<float*>(dst) = v[0];
  };
  // every LDS store issued so far, the inline-assembly ones included, has completed
  auto lds_pair_wait = [] {
    if constexpr (ASM_STORES) __builtin_amdgcn_s_waitcnt(0xc07f);      // gfx9 encoding of lgkmcnt(0) alone: vmcnt and expcnt fields at their maxima
  };

  auto store_tiles = [&](auto stage, int buf) {
    constexpr int ST = decltype(stage)::value;
    f4* const As = As_all + buf * ASZ;
    f4* const Bs = Bs_all + buf * BSZ;
    if constexpr (MODE == MODE_WGRAD) {
#ifdef ACG_NORM_PROBE
#pragma unroll
      for (int e = 0; e < LPA; ++e) ra[ST][e] = probe_apply(ra[ST][e], probe_s, probe_t, probe_lo, probe_ok[ST][e]);
#endif
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v[LPA];
#pragma unroll
        for (int e = 0; e < LPA; ++e) v[e] = ra[ST][e][i];
        put_part(As, BM, kqa, suba, 4 * ja + i, std::integral_constant<int, LPA>{}, v);
      }
    } else {
      const int kq = tid & 7, rg = tid >> 3;
#ifdef ACG_NORM_PROBE
      {   // the channel quad of this K-step's gathers: one parameter lookup per K-step (all QA quads of a thread share it)
        const int c4 = (kq + ST) & 15;
        const f4 ps = probe_par[0][c4], pt = probe_par[1][c4], pl = probe_par[2][c4];
#pragma unroll
        for (int u = 0; u < QA; ++u) ra[ST][u] = probe_apply(ra[ST][u], ps, pt, pl, probe_ok[ST][u]);
      }
#endif
#pragma unroll
      for (int u = 0; u < QA; ++u) put(As, BM, kq, rg + 32 * u, ra[ST][u]);
      if constexpr (MODE == MODE_DGRAD) {
#pragma unroll
        for (int u = 0; u < QB; ++u) put(Bs, BN, kq, rg + 32 * u, rb[ST][u]);
      }
    }
    if constexpr (MODE != MODE_DGRAD) {
      if constexpr (nvec) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v[LPB];
#pragma unroll
          for (int e = 0; e < LPB; ++e) v[e] = rb[ST][e][i];
          put_part(Bs, BN, kqb, subb, 4 * jb + i, std::integral_constant<int, LPB>{}, v);
        }
      } else {
        constexpr int stepB = 256 / BN;
        const int nb = tid % BN, kq0 = tid / BN;
#pragma unroll
        for (int u = 0; u < QB; ++u) put(Bs, BN, kq0 + stepB * u, nb, rb[ST][u]);
      }
    }
  };

  // ---- main loop ----------------------------------------------------------------------------------
  // Accumulator sets rotated by k within a K-step (summed in the epilogue).  Measured (tools/micro/mfma_rate.hip):
  // a chain of dependent v_mfma_f32_32x32x2_f32 through ONE accumulator already issues every 68-74 cycles, so one
  // set is enough; the knob stays for experiments.
#ifndef ACG_NSET
#define ACG_NSET 1
#endif
  constexpr int NSET = (TA * TB >= 4) ? 1 : ACG_NSET;
  f32x16 accs[NSET][TA][TB];
  auto& acc = accs[0];
#pragma unroll
  for (int a = 0; a < TA; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int z = 0; z < NSET; ++z) accs[z][a][b][r] = 0.f;
      }

  const int wr = wave / WN, wc = wave - wr * WN;
  const int wm0 = wr * (BM / WM), wn0 = wc * (BN / WN);
  const int lrow = lane & 31, lk = lane >> 5;

  // MFMA work of one K-step as NM single instructions in NT groups (a group = one k-slot per lane half): group t
  // reads quad 2t+h of BOTH tiles for lane half h - the MFMA contracts slot (lane>>5) of A with the same slot of B,
  // so the k order inside a K-step is free - and feeds it to GM MFMAs.
  constexpr int NT = 4, GM = 4 * TA * TB, NM = NT * GM;
  f4 av[2][TA], bv[2][TB];        // operand fragments of group t live in av[t & 1]
  auto frag_read = [&](int buf, auto tc) {
    constexpr int T = decltype(tc)::value;
    const f4* const As = As_all + buf * ASZ;
    const f4* const Bs = Bs_all + buf * BSZ;
    const int kq = 2 * T + lk;
#pragma unroll
    for (int a = 0; a < TA; ++a) av[T & 1][a] = As[kq * BM + pcol(wm0 + 32 * a + lrow, kq)];
#pragma unroll
    for (int b = 0; b < TB; ++b) bv[T & 1][b] = Bs[kq * BN + pcol(wn0 + 32 * b + lrow, kq)];
  };
  auto mfma = [&](auto ic) {
    constexpr int I = decltype(ic)::value;
    constexpr int T = I / GM, R = I % GM, AB = R % (TA * TB), A = AB / TB, B = AB % TB;
    constexpr int E = R / (TA * TB);
    accs[E % NSET][A][B] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[T & 1][A][E], bv[T & 1][B][E], accs[E % NSET][A][B], 0, 0, 0);
  };

  // WGRAD gathers along the reduction: the row infos change every K-step.  They are derived 8 K-steps (256 rows,
  // one per thread) at a time into the half of `rows` selected by the chunk parity, one barrier ahead of their
  // first use, so the K-loop itself carries no divergent "first 32 threads" section.
  auto wgrad_rows = [&](int chunk) {
    if constexpr (MODE == MODE_WGRAD) rows[(chunk & 1) * 256 + tid] = row_info<MODE, F32Tensors, false>(p, g, (ks_begin + 8 * chunk) * BK + tid, Kdim);
  };
  // UW: a chunk is UNR K-steps (192 of the 256 rows the threads derive are read), so a step's slot in its chunk is the unrolled
  // copy's own constant and the refill sits in ONE copy - the one whose successor issues the first loads of the next chunk -
  // as straight-line code: no condition (rows at or beyond Kdim come out dead), no loop, nothing divergent.
  auto uw_rows = [&](int row0, unsigned half) {
    const WgradRow w = wgrad_row<F32Tensors>(p, row0 + tid, Kdim, uk_shift, uw_rep);
    const unsigned at = ((unsigned)tid * 4u) ^ half;
    *reinterpret_cast<unsigned*>(uw_tab + at) = w.off;
    *reinterpret_cast<unsigned*>(uw_tab + UW_ARR + at) = w.inv_lo;
    *reinterpret_cast<unsigned*>(uw_tab + 2 * UW_ARR + at) = w.inv_hi;
  };

  // prologue: stages 0..NST-1 <- steps ks_begin..+NST-1; step ks_begin -> LDS buffer 0
  if (ks_begin < ks_end) {
    if constexpr (UW) { uw_rows(ks_begin * BK, 0u); __syncthreads(); }
    else if constexpr (MODE == MODE_WGRAD) { wgrad_rows(0); __syncthreads(); }
    static_for<0, NST>([&](auto jc) {
      constexpr int J = decltype(jc)::value;
      load_tiles(jc, ks_begin + J, ks_begin + J < ks_end);
    });
    store_tiles(std::integral_constant<int, 0>{}, 0);
    lds_pair_wait();
    __syncthreads();
  }
  // iteration ks: LDS[buf] holds step ks; stage J (its source) is free; stage J+1 holds step ks+1.
  // The loads of the step NST ahead are dealt out between the MFMAs and the order is pinned with sched_barrier: it
  // keeps the fragment reads of group t+1 in front of the MFMAs of group t and spreads the VMEM issue over the K-step.
  auto iterate = [&](auto uc, int ks) {
    constexpr int C = decltype(uc)::value, J = C % NST;      // C: the unrolled copy = (ks - ks_begin) % UNR
    const std::integral_constant<int, J> jc{};
    const int buf = C & 1;
    using SN = std::integral_constant<int, (J + 1) % NST>;
    const bool live = ks + NST < ks_end;
    if constexpr (UW && C == 0) {      // round (ks - ks_begin) / UNR starts in chunk half `round & 1`: derived, not carried (see the loop below)
      uw_half = ((__umulhi((unsigned)(ks - ks_begin), 0xAAAAAAABu) >> 2) & 1u) * UW_HALF;
      static_assert(!UW || UNR == 6, "UW: x / 6 = umulhi(x, 0xAAAAAAAB) >> 2");
      uw_ro[0] = ((unsigned)r0a * 4u) ^ uw_half; uw_ro[1] = uw_ro[0] ^ UW_HALF;
      uw_rm[0] = uw_ro[0] + (wg_t < 32 ? 1u : 2u) * UW_ARR; uw_rm[1] = uw_rm[0] ^ UW_HALF;
    }
    frag_read(buf, std::integral_constant<int, 0>{});
    const Prep q = load_prep(ks + NST, live, std::integral_constant<int, (C + NST) % UNR>{}, std::integral_constant<int, (C + NST) / UNR>{});
    store_tiles(SN{}, buf ^ 1);       // overlaps the LDS latency of the first fragments and of the lookups
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, NM>([&](auto ic) {
      constexpr int I = decltype(ic)::value;
      // the last fragment group is waited for here with the LDS counter at zero anyway; said in the source, the same wait also
      // covers this iteration's inline-assembly stores, and no more of them follow before the barrier
      if constexpr (I == (NT - 1) * GM) lds_pair_wait();
      mfma(ic);
      if constexpr (I % GM == 0 && I / GM + 1 < NT) frag_read(buf, std::integral_constant<int, I / GM + 1>{});
      static_for<0, NLD>([&](auto pc) {
        constexpr int P = decltype(pc)::value;
        if constexpr ((P * NM) / NLD == I) load_piece(jc, ks + NST, live, q, pc);
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    if constexpr (UW) {
      if constexpr ((C + NST + 1) % UNR == 0) uw_rows((ks + NST + 1) * BK, uw_half ^ UW_HALF);      // the chunk whose loads start in the NEXT iteration
    } else if constexpr (MODE == MODE_WGRAD) {
      const int rel = ks - ks_begin + NST + 1;      // first step whose loads are issued in the NEXT iteration
      if ((rel & 7) == 0 && ks + NST + 1 < ks_end) wgrad_rows(rel >> 3);
    }
    __syncthreads();
  };
  // (stage, LDS buffer) repeat with period UNR = lcm(NST, 2); every unrolled iteration has exactly ONE predecessor
  // besides the loop entry, so the compiler's outstanding-load bookkeeping stays exact (chained `if (ks+j < end)`
  // do not: each skipped iteration is a second path into the next one and the merge drains vmcnt to 0)
  if (ks_begin < ks_end) {
    int ks = ks_begin;
    while (run_unrolled<0, UNR>([&](auto ic) {
      iterate(ic, ks);
      return ++ks < ks_end;
    })) {
    }
  }

  if constexpr (NSET > 1) {
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        if constexpr (NSET == 4) acc[a][b] = (accs[0][a][b] + accs[1][a][b]) + (accs[2][a][b] + accs[3][a][b]);
        else acc[a][b] = accs[0][a][b] + accs[NSET - 1][a][b];
      }
  }
  // ---- epilogue: C/D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) --------------
  if constexpr (MODE != MODE_WGRAD) {
    if (p.stats != nullptr) {     // BatchNorm statistics of this tile (ConvArgs::stats): thread -> lane-half pair -> waves of a column
      tile_stats_epilogue<BM, BN, WM, TA, TB>([&](int a, int b, int r) { return acc[a][b][r]; }, reinterpret_cast<float*>(smem),
                                              p.stats + stats_block<MODE>(p, by, tm) * 2 * N, N, M, m0, n0, wm0, wn0, wr, lrow, lk, tid);
    }
  }
  if constexpr (EPI) {          // bias + activation of a layer built with normalizer_fn = None (models.py:20-21: tanh(deconv + b))
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      const int n = n0 + wn0 + 32 * b + lrow;
      const float bv = n < N ? p.bias[n] : 0.f;
#pragma unroll
      for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = acg::act_apply(p.act, acc[a][b][r] + bv, p.leak);
    }
  }
  float* outp = p.out + (p.splits > 1 ? (long long)bz * p.out_numel : 0ll);
  store_tile<MODE, BM, TA, TB, false>(acc, out_map<MODE, F32Tensors, COMPACT>(p, g), rows, outp, false, wm0, wn0, lrow, lk);
}

template <int MODE, int BM, int BN, int WM, int WN, bool RAGGED, bool NVEC, bool EPI = false, bool LIN = false, bool UK = false, bool UW = false>
__global__ __launch_bounds__(256) void conv_mfma_f32(const ConvArgs p) {
  __shared__ __align__(16) char smem[conv_lds_bytes<MODE, BM, BN, UW>()];
  if constexpr (MODE == MODE_WGRAD) {      // grid (tiles, 1, splits)
    int tile, split;
    wgrad_xcd_map((int)(blockIdx.x + gridDim.x * blockIdx.z), (int)gridDim.x, (int)gridDim.z, tile, split);
    conv_body<MODE, BM, BN, WM, WN, RAGGED, NVEC, false, false, false, UW>(p, tile, 0, split, (int)gridDim.x, smem);
  } else {
    conv_body<MODE, BM, BN, WM, WN, RAGGED, NVEC, EPI, LIN, UK>(p, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, (int)gridDim.x, smem);
  }
}


// ---- two contractions in one launch -------------------------------------------------------------------------------
// A layer's input gradient (DGRAD, or FWD on the adjoint descriptor for a transposed layer) and its weight gradient
// both consume dy and are independent of each other.  Launched one after the other, each runs with about one block
// per CU and pays its own launch gap, prologue and tail; out of ONE grid the blocks of the second contraction become
// the second resident block of every CU (0.74 -> 0.53 us per K-step) and fill the first one's tail.  Two streams
// would do the same, but a cross-stream edge costs ~18 us on this stack (profiles/r1/w_stream_edges.txt).
// Blocks [0, nA) run contraction A with the grid (gxA, gyA, *), the rest run the weight gradient with (gxB, 1, *).
struct PairGeom { int nA, gxA, gyA, gxB; };

template <int MODE_A, int BMA, int BNA, int WMA, int WNA, int BMB, int BNB, int WMB, int WNB, bool RAGGED, bool LIN_A = false, bool UK_A = false, bool UW_B = false>
__global__ __launch_bounds__(256) void conv_pair_f32(const ConvArgs a, const ConvArgs b, const PairGeom g) {
  constexpr int LA = conv_lds_bytes<MODE_A, BMA, BNA>(), LB = conv_lds_bytes<MODE_WGRAD, BMB, BNB, UW_B>();
  __shared__ __align__(16) char smem[LA > LB ? LA : LB];      // one block runs one of the two programs
  const int L = (int)blockIdx.x;
  if (L < g.nA) {
    const int t = L / g.gxA;
    conv_body<MODE_A, BMA, BNA, WMA, WNA, RAGGED, true, false, LIN_A, UK_A>(a, L - t * g.gxA, t % g.gyA, t / g.gyA, g.gxA, smem);
  } else {
    int tile, split;
    wgrad_xcd_map(L - g.nA, g.gxB, b.splits, tile, split);
    conv_body<MODE_WGRAD, BMB, BNB, WMB, WNB, RAGGED, true, false, false, false, UW_B>(b, tile, 0, split, g.gxB, smem);
  }
}

struct Plan {
  int cfg;       // 2: 128x32, 3: 64x64 (0 and 1 were the retired 128x128 / 128x64 tiles)
  int bm, bn;
  long long M, N;  // per class (class 0 = largest) GEMM extents (M padded per tap for WGRAD)
  int classes, nk, splits;
  bool ragged, nvec, bf16;
  bool direct;     // a few-MFLOP float32 contraction with at most 8 output channels: the direct kernels of conv_direct.hip, one launch, no slabs
  long long tiles, out_numel;
  int out_pitch, out_cols;   // FWD / DGRAD: channel pitch of the output tensor and the channels the contraction computes (the rest of a
                             // row - pad channels, channels at or beyond dgrad_c / adj_dgrad_c - is never written, by the reduction neither)
};

// conv_direct.hip
int launch_direct(int which, const ConvArgs& a, hipStream_t st);
int launch_direct_pair(const ConvArgs& a, const ConvArgs& b, hipStream_t st);

template <int MODE>
int launch_mode(const Plan& pl, const ConvArgs& a, hipStream_t st);

// conv_f32_pair.hip: A (modeA = MODE_FWD or MODE_DGRAD) and a weight gradient B in one launch; fp32, float4-able dense
// operands, both gathers ragged or neither (pair_supported) - the caller launches the two separately otherwise.
static inline bool pair_supported(int modeA, const Plan& pa, const Plan& pb) {
  return (modeA == MODE_FWD || modeA == MODE_DGRAD) && !pa.bf16 && !pb.bf16 && pa.ragged == pb.ragged && pa.nvec && pb.nvec &&
         (long long)pa.tiles * pa.splits + (long long)pb.tiles * pb.splits < (1ll << 30);
}
// conv_f32_dgrad.hip / conv_bf16_dgrad.hip: the one EPI instantiation each (a transposed layer's forward on the 128x32 tile)
int launch_deconv_fwd_epi(const Plan& pl, const ConvArgs& a, hipStream_t st);
int launch_deconv_fwd_epi16(const Plan& pl, const ConvArgs& a, hipStream_t st);
int launch_pair(int modeA, const Plan& pa, const ConvArgs& a, const Plan& pb, const ConvArgs& b, hipStream_t st);

// The LIN variant (filter rows linear in k; FWD with float4-able operands only): gathered channels a multiple of 4 and the taps in
// natural order.  One rule for the single launch (launch_cfg), the paired one (launch_pair) and the path query (acgan_conv_plan.h).
static inline bool lin_variant(int mode, const Plan& pl, const ConvArgs& a) {
  return mode == MODE_FWD && !pl.ragged && pl.nvec && (a.C & 3) == 0 && !a.compact && !a.tap_classes;
}

// The UK variant (K-step state in scalar registers, conv_body): FWD where it is LIN, and DGRAD, with 16-byte gathers of a
// channel count that is a multiple of the K-step - so a K-step lies inside one tap, also of a compacted tile or a stride class,
// whose tables it reads like the generic loaders.  Weight gradients never take it (their gathered rows change every K-step; they
// have a variant of their own, uniform_w_variant below).  Operands of at most 2^29 bytes and a padding corner of at most that: conv_body's masked offsets of 2^31 and more
// are then beyond every record count.  g_uniform_k: acg_conv2d_uniform_k (acgan_conv_plan.h), the variant alone - never a plan.
// One rule for launch_cfg, launch_pair, the bias + activation entry and the path query.
extern int g_uniform_k;
static inline bool uniform_k_variant(int mode, const Plan& pl, const ConvArgs& a) {
  if (!g_uniform_k || pl.bf16 || pl.direct || pl.ragged) return false;
  if (mode != MODE_DGRAD && !lin_variant(mode, pl, a)) return false;      // (FWD: LIN brings float4-able filter rows with it; DGRAD never reads NVEC)
  const int cs = mode == MODE_DGRAD ? a.K : a.C;
  const long long corner = mode == MODE_FWD ? (long long)(a.pt * (long long)a.W + a.pl) * a.Cx * 4 : 0;
  return cs % BK == 0 && a.g_bytes <= (1u << 29) && a.d_bytes <= (1u << 29) && corner <= (1ll << 29);
}

// The UW variant (conv_body): a weight gradient with 16-byte loads on both sides - gathered channels a multiple of 4 (any such
// count: nothing in it needs a K-step inside one tap), dY rows float4-able.  The same 2^29-byte bounds as UK on both operands and
// the padding corner, for the same reason.  g_uniform_w: acg_conv2d_uniform_w (acgan_conv_plan.h), the variant alone - never a plan.
// One rule for launch_cfg, launch_pair and the path query (launch_pair leaves one tile combination out: conv_f32_pair.hip, launch_b).
extern int g_uniform_w;
static inline bool uniform_w_variant(int mode, const Plan& pl, const ConvArgs& a) {
  if (!g_uniform_w || mode != MODE_WGRAD || pl.bf16 || pl.direct || pl.ragged || !pl.nvec) return false;
  const long long corner = (long long)(a.pt * (long long)a.W + a.pl) * a.Cx * 4;
  return a.g_bytes <= (1u << 29) && a.d_bytes <= (1u << 29) && corner <= (1ll << 29);
}

template <int MODE, bool RAGGED, bool NVEC>
static inline void launch_cfg(const Plan& pl, const ConvArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(acg::ceil_div(pl.M, pl.bm) * acg::ceil_div(pl.N, pl.bn)), (unsigned)pl.classes, (unsigned)pl.splits);
  if constexpr (MODE == MODE_WGRAD && !RAGGED && NVEC) {
    if (uniform_w_variant(MODE, pl, a)) {
      if (pl.cfg == 2) ACG_LAUNCH((conv_mfma_f32<MODE, 128, 32, 4, 1, false, true, false, false, false, true>), grid, dim3(256), 0, st, a);
      else ACG_LAUNCH((conv_mfma_f32<MODE, 64, 64, 2, 2, false, true, false, false, false, true>), grid, dim3(256), 0, st, a);
      return;
    }
  }
  if constexpr (MODE != MODE_WGRAD && !RAGGED) {
    if (uniform_k_variant(MODE, pl, a)) {      // (one instantiation per tile: the DGRAD body is the same code for either NVEC)
      constexpr bool LIN = MODE == MODE_FWD;
      if (pl.cfg == 2) ACG_LAUNCH((conv_mfma_f32<MODE, 128, 32, 4, 1, false, true, false, LIN, true>), grid, dim3(256), 0, st, a);
      else ACG_LAUNCH((conv_mfma_f32<MODE, 64, 64, 2, 2, false, true, false, LIN, true>), grid, dim3(256), 0, st, a);
      return;
    }
  }
  // two tile shapes: 128x32 for narrow N, 64x64 otherwise.  128x128 / 128x64 variants existed through v4; with the
  // one-barrier pipeline they lost every layer of the tuning sweep (profiles/r1) and were dropped.
  if constexpr (MODE == MODE_FWD && !RAGGED && NVEC) {
    if (lin_variant(MODE, pl, a)) {
      if (pl.cfg == 2) ACG_LAUNCH((conv_mfma_f32<MODE, 128, 32, 4, 1, RAGGED, NVEC, false, true>), grid, dim3(256), 0, st, a);
      else ACG_LAUNCH((conv_mfma_f32<MODE, 64, 64, 2, 2, RAGGED, NVEC, false, true>), grid, dim3(256), 0, st, a);
      return;
    }
  }
  if (pl.cfg == 2) ACG_LAUNCH((conv_mfma_f32<MODE, 128, 32, 4, 1, RAGGED, NVEC>), grid, dim3(256), 0, st, a);
  else ACG_LAUNCH((conv_mfma_f32<MODE, 64, 64, 2, 2, RAGGED, NVEC>), grid, dim3(256), 0, st, a);
}
template <int MODE>
static inline void launch_variant(const Plan& pl, const ConvArgs& a, hipStream_t st) {
  if (pl.ragged) {
    if (pl.nvec) launch_cfg<MODE, true, true>(pl, a, st);
    else launch_cfg<MODE, true, false>(pl, a, st);
  } else {
    if (pl.nvec) launch_cfg<MODE, false, true>(pl, a, st);
    else launch_cfg<MODE, false, false>(pl, a, st);
  }
}

#define ACG_DEFINE_CONV_LAUNCH(MODE)                                                    \
  template <>                                                                           \
  int launch_mode<MODE>(const Plan& pl, const ConvArgs& a, hipStream_t st) {            \
    launch_variant<MODE>(pl, a, st);                                                    \
    return acg::check_launch("conv_mfma_f32");                                          \
  }

}  // namespace acgconv
