// What a block program of the implicit-GEMM convolutions does around its K loop, written once for the three of them
// (conv_f32_kernel.h, conv_bf16_kernel.h, conv_bf16_glds.h): the launch arguments, the problem geometry of a tile, the tap
// tables, the per-row gather infos, the tap compaction of small maps, and the map from an accumulator element to its place in
// the output.  Integer arithmetic only - no MFMA, no buffer builtin - so this header also compiles as plain C++ against
// tools/micro/hip_host/hip/hip_runtime.h, where tools/micro/conv_tile_host.cpp holds every address it produces against the
// definition of the convolution (tests/test_conv_tile_host.py).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/acgan_hip.h"

namespace acgconv {

enum { MODE_FWD = 0, MODE_DGRAD = 1, MODE_WGRAD = 2 };

constexpr int kMaxTaps = 64;

struct ConvArgs {
  const float* gsrc;   // gathered tensor: x (FWD, WGRAD) or dy (DGRAD)
  const float* dense;  // w (FWD, DGRAD) or dy (WGRAD)
  float* out;          // final tensor (splits == 1) or `splits` slabs of out_numel floats
  long long out_numel;
  unsigned g_bytes, d_bytes;   // sizes of gsrc / dense for the buffer descriptors (hardware range check)
  float accumulate;    // WGRAD with splits == 1: out = accumulate * out + value
  int batch, H, W, C, OH, OW, K, KH, KW, sh, sw, pt, pl;
  int Cx;              // channel pitch of x / dx in memory (>= C)
  int Ky;              // channel pitch of y / dy in memory (>= K)
  int splits;
  unsigned mg_ow, mg_oh, mg_cp;   // magic multipliers: r / OW = (r * mg_ow) >> sh_ow for 0 <= r < 2^31 (host: fast_div)
  int sh_ow, sh_oh, sh_cp;        // _cp: division by the gathered channel count padded to a multiple of 4
  // FWD / DGRAD with splits == 1, optional: the layer's BatchNorm statistics out of the epilogue.  Each block leaves the
  // per-channel SUM of ITS tile rows (of the values as stored) and their sum of squared deviations from the tile's own
  // mean (M2) at stats[((g * stats_nblk + b) * 2 + {0: sum, 1: M2}) * N + n]; bn.hip merges the tiles (conv_f32_kernel.h: tile_stats_epilogue);
  // FWD: g = tile_row / stats_tpg, b = tile_row % stats_tpg; DGRAD (one group): b = class * stats_tpg + tile_row.
  float* stats;
  int stats_nblk, stats_tpg;
  // FWD / DGRAD slabs (splits > 1) handed to the layer's BatchNorm: 0 = each slab [rows][pitch] like the tensor; > 0 = the
  // ACG_SLABS_QUADS layout [channels / 4][slab_rows][4] (slab_rows = all rows of the tensor), element (m, n) at
  // ((n >> 2) * slab_rows + m) * 4 + (n & 3)
  int slab_rows;
  // FWD launched as the merged input gradient of a stride-2 layer with few input channels (conv_f32.hip run_merged): the N =
  // 4 * shuf_c output columns of pixel (b, p, q) are the shuf_c channels of the 2 x 2 output pixels (2p + ph, 2q + pw) of a
  // tensor that is shuf_w pixels wide at the channel pitch shuf_pitch; column n = (2 ph + pw) * shuf_c + c.  0 = off.
  int shuf_c, shuf_w, shuf_pitch;
  // Small maps (DGRAD; conv_f32.hip prepare): rows are ordered pixel-major - m = pixel * batch + b, so a tile covers one or
  // two pixels over the batch - and the tile walks only the taps ANY of its rows can see: on a 4 x 4 map half the taps of a
  // 5 x 5 filter fall into the padding for every row of such a tile, and their K-steps would multiply zeros.
  int compact;
  int Nv;              // FWD / DGRAD: only the first Nv output columns are computed (acg_conv_desc dgrad_c / adj_dgrad_c); 0 = all
  int tap_classes;     // FWD, stride > 1: 1 = the taps are walked class by class (tap_class_pos below); 0 = row-major
  int korder;          // bf16 kernels, FWD / DGRAD, gathered channels a multiple of 64: 1 = K-steps walk the taps of one 64-channel chunk
                       // before the next chunk (0: all channels of a tap before the next tap) - conv_bf16_kernel.h
  int out_f32;         // bf16 kernels, FWD / DGRAD: the result is stored as float32 (at the bf16 tensor's pitch, round8): a head layer
  // EPI kernel variants only (acg_deconv2d_fwd_bias_act): out = act(acc + bias[n]), stored as float32 at the pitch Cx
  const float* bias;
  int act;
  float leak;
};

// Division by a launch-constant through multiply-high (Granlund-Montgomery, N = 31): a runtime integer division is
// ~40 VALU instructions on this ISA, and WGRAD derives 32 gather rows per K-step.
struct FastDiv { unsigned magic; int shift; };
static inline FastDiv fast_div(int d) {
  int s = 0;
  while ((1ll << s) < d) ++s;
  const unsigned long long num = 1ull << (31 + s);
  return FastDiv{(unsigned)((num + (unsigned long long)d - 1) / (unsigned long long)d), 31 + s};
}
__device__ __forceinline__ int div_fast(int r, unsigned magic, int shift) {
  return (int)(((unsigned long long)(unsigned)r * magic) >> shift);
}

// Weight-gradient blocks: block l of gx * splits (x fastest) -> (tile, split).  The hardware deals workgroups round-robin
// over the 8 XCDs in dispatch order, so blocks l, l+8, l+16 ... share an XCD; all gx tiles of one split read the same
// pixel range of both operands (each at its own filter taps): give them to ONE XCD, so that range comes out of HBM / the
// Infinity Cache once instead of once per XCD (measured: g/tconv4's pair at 128x128 fetched 878 MB per launch, 6x its
// operands).  Splits that are not a multiple of 8 keep the plain order.  Placement only: results do not change.
__device__ __forceinline__ void wgrad_xcd_map(int l, int gx, int splits, int& tile, int& split) {
  if ((splits & 7) == 0) {
    const int x8 = l & 7, q = l >> 3, grp = q / gx;
    tile = q - grp * gx;
    split = grp * 8 + x8;
  } else {
    split = l / gx;
    tile = l - split * gx;
  }
}

struct alignas(16) RowInfo {
  int base;            // element offset of the row's (tap 0, channel 0) source element (may be virtual)
  unsigned mask_lo, mask_hi;  // bit t set <=> filter tap t reads inside the tensor
  int out_off;         // DGRAD: element offset of the output pixel; unused otherwise
};

__device__ __forceinline__ unsigned long long tap_mask(int lo_a, int hi_a, int lo_b, int hi_b, int nb) {
  // bits (a * nb + b) for a in [lo_a, hi_a), b in [lo_b, hi_b)
  if (hi_a <= lo_a || hi_b <= lo_b) return 0ull;
  const unsigned long long row = ((1ull << (hi_b - lo_b)) - 1ull) << lo_b;
  unsigned long long m = 0ull;
  for (int a = lo_a; a < hi_a; ++a) m |= row << (a * nb);
  return m;
}

// Class-major tap order of a STRIDED forward convolution (ConvArgs::tap_classes).  Tap (i, j) of a stride-(sh, sw) conv reads
// the input lattice (y = sh * p + i - pt, x = sw * q + j - pl): taps with equal (i % sh, j % sw) read the SAME sub-lattice of the
// input, shifted by whole output pixels, and taps of different classes read DISJOINT sub-lattices.  In row-major order the taps
// that share a cache line are up to two filter rows (10 K-steps x channel chunks x every tile running on the XCD) apart: the
// vertical re-use misses the 4 MB L2 and every input byte is fetched from the memory side ~3.5 times (TCC_MISS 36 % of the
// K-loop's requests, profiles/r4/h_bf16_kloop_load_path.txt).  Walking one class after the other keeps a tile on one sub-lattice - its
// window / (sh * sw), 43 KB for a 256-row tile of 64 channels - for all of the class's taps; it is a permutation of the K index
// only (tap tables and row masks are built in that order), so results differ by summation order alone.
// Built for stride 2 x 2 (every strided layer of the reference's models): class (a, b) = (i & 1, j & 1), na(a) x nb(b) taps each.
__device__ __forceinline__ int tap_class_pos(int i, int j, int KH, int KW) {
  const int a = i & 1, b = j & 1;
  const int na0 = (KH + 1) >> 1, nb0 = (KW + 1) >> 1;
  const int na = a ? KH >> 1 : na0, nb = b ? KW >> 1 : nb0;
  return (a ? na0 * KW : 0) + (b ? na * nb0 : 0) + (i >> 1) * nb + (j >> 1);
}
__device__ __forceinline__ unsigned long long tap_mask_classes(int lo_i, int hi_i, int lo_j, int hi_j, int KH, int KW) {
  // the rectangle [lo_i, hi_i) x [lo_j, hi_j) of taps is a rectangle of (ti, tj) in each of the four classes
  unsigned long long m = 0ull;
  const int na0 = (KH + 1) >> 1, nb0 = (KW + 1) >> 1;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int na = a ? KH >> 1 : na0, nb = b ? KW >> 1 : nb0;
      const int base = (a ? na0 * KW : 0) + (b ? na * nb0 : 0);
      m |= tap_mask(max(0, (lo_i - a + 1) >> 1), max(0, (hi_i - a + 1) >> 1), max(0, (lo_j - b + 1) >> 1), max(0, (hi_j - b + 1) >> 1), nb) << base;
    }
  return m;
}

// 32-bit operations only: 64-bit shifts and compares are quarter-rate on the VALU, and a wave's VALU work does NOT
// hide behind its own MFMAs (tools/conv_kloop.py experiments in profiles/), so every instruction in the K-loop counts
__device__ __forceinline__ bool tap_ok(const RowInfo& ri, int t) {
  const unsigned w = t < 32 ? ri.mask_lo : ri.mask_hi;
  return (w >> (t & 31)) & 1u;
}

constexpr unsigned kOob = 0xFFFFFF00u;   // >= any num_records (tensors are < 2^30 elements)

// ---- row table of the weight gradient's UW loaders (conv_f32_kernel.h) ----------------------------------------------------------
// tap_mask without its loop: the column range of one filter row, repeated into every filter row by a multiply with
// rep = sum over a < KH of 2^(a * nb) (tap_rep; no carries, the range is narrower than nb bits), cut to the rows [lo_a, hi_a).
__device__ __forceinline__ unsigned long long bit_range(int lo, int hi) {      // bits [lo, hi) with 0 <= lo and hi <= 64; none where hi <= lo
  const int n = hi - lo;
  return n > 0 ? (~0ull >> ((64 - n) & 63)) << (lo & 63) : 0ull;
}
__device__ __forceinline__ unsigned long long tap_rep(int na, int nb) {
  unsigned long long rep = 0ull;
  for (int a = 0; a < na; ++a) rep |= 1ull << (a * nb);
  return rep;
}
__device__ __forceinline__ unsigned long long tap_mask_closed(int lo_a, int hi_a, int lo_b, int hi_b, int nb, unsigned long long rep) {
  return (bit_range(lo_b, hi_b) * rep) & bit_range(lo_a * nb, hi_a * nb);
}
// Output pixel r = (b, p, q) as a K position of the weight gradient: the BYTE offset of its (tap 0, channel 0) source element,
// taken from the padding corner (`shift` elements in front of the tensor: never negative), and the COMPLEMENT of its tap mask.
// Straight-line code: a row at or beyond `limit` is selected to (0, all taps dead), not branched around.
struct WgradRow { unsigned off, inv_lo, inv_hi; };
template <class TR>
__device__ __forceinline__ WgradRow wgrad_row(const ConvArgs& p, const int r, const int limit, const int shift, const unsigned long long rep) {
  const int t2 = div_fast(r, p.mg_ow, p.sh_ow), q = r - t2 * p.OW, b = div_fast(t2, p.mg_oh, p.sh_oh), pp = t2 - b * p.OH;
  const int y0 = pp * p.sh - p.pt, x0 = q * p.sw - p.pl;
  const unsigned long long m = tap_mask_closed(max(0, -y0), min(p.KH, p.H - y0), max(0, -x0), min(p.KW, p.W - x0), p.KW, rep);
  const bool in = r < limit;
  const unsigned off = (unsigned)(((b * p.H + y0) * p.W + x0) * TR::x_pitch(p) + shift) * 4u;
  return WgradRow{in ? off : 0u, in ? ~(unsigned)m : ~0u, in ? ~(unsigned)(m >> 32) : ~0u};
}

// ---- storage traits: what the element type of the tensors changes in the addressing -----------------------------------------
// unit: channels per 16-byte load, every gathered channel count is padded to it per tap; x_pitch / y_pitch: channels between two
// pixels of x (dx) / y (dy) in memory; tap_fwd / tap_dgrad: elements between two taps of the filter copy FWD / DGRAD reads;
// dx_pitch: pitch of the tensor DGRAD writes.
struct F32Tensors {      // pitches from the descriptor; one filter [tap][c][o] for both contractions
  static constexpr int unit = 4;
  static __device__ __forceinline__ int x_pitch(const ConvArgs& p) { return p.Cx; }
  static __device__ __forceinline__ int y_pitch(const ConvArgs& p) { return p.Ky; }
  static __device__ __forceinline__ int tap_fwd(const ConvArgs& p) { return p.C * p.K; }
  static __device__ __forceinline__ int tap_dgrad(const ConvArgs& p) { return p.C * p.K; }
  static __device__ __forceinline__ int dx_pitch(const ConvArgs& p) { return p.Cx; }
};
// activations at pitch round8(channels); the prepared filter copies [tap][o][c8] (FWD) and [tap][c][o8] (DGRAD).
// EPI: bf16 operands, the bias + activation result as float32 rows at the pitch Cx.
template <bool EPI = false>
struct Bf16Tensors {
  static constexpr int unit = 8;
  static __device__ __forceinline__ int x_pitch(const ConvArgs& p) { return (p.C + 7) & ~7; }
  static __device__ __forceinline__ int y_pitch(const ConvArgs& p) { return (p.K + 7) & ~7; }
  static __device__ __forceinline__ int tap_fwd(const ConvArgs& p) { return p.K * x_pitch(p); }
  static __device__ __forceinline__ int tap_dgrad(const ConvArgs& p) { return p.C * y_pitch(p); }
  static __device__ __forceinline__ int dx_pitch(const ConvArgs& p) { return EPI ? p.Cx : x_pitch(p); }
};

// ---- problem geometry of a tile (wave-uniform) ---------------------------------------------------------------------------
// Cs: channels of the gathered tensor; Cp: Cs padded to the unit (granularity per tap).  DGRAD runs one stride class
// (ph, pw) = (by / sw, by % sw) per grid row: the Hc x Wc input pixels (ph + sh * h2, pw + sw * w2), reached by the nti x ntj
// taps (i0 + sh * ti, j0 + sw * tj) from dY[h2 + dp0 - ti][w2 + dq0 - tj].
struct TileGeom {
  int M, N, Kdim, Cs, Cp, ntaps;
  int ph, pw, i0, j0, nti, ntj, dp0, dq0, Hc, Wc;
  int tm, tn, m0, n0;
  bool empty;      // block-uniform: a tile beyond M (DGRAD classes smaller than class 0) - the block returns
};

template <int MODE, class TR>
__device__ __forceinline__ TileGeom tile_geometry(const ConvArgs& p, const int bx, const int by, const int gx, const int BM, const int BN) {
  TileGeom g{};
  g.nti = 1; g.ntj = 1;
  if constexpr (MODE == MODE_FWD) {
    g.Cs = p.C; g.Cp = (g.Cs + TR::unit - 1) & ~(TR::unit - 1); g.ntaps = p.KH * p.KW;
    g.M = p.batch * p.OH * p.OW; g.N = p.K; g.Kdim = g.ntaps * g.Cp;
  } else if constexpr (MODE == MODE_DGRAD) {
    const int cls = by;
    g.ph = cls / p.sw; g.pw = cls - g.ph * p.sw;
    g.Hc = g.ph < p.H ? (p.H - g.ph + p.sh - 1) / p.sh : 0;
    g.Wc = g.pw < p.W ? (p.W - g.pw + p.sw - 1) / p.sw : 0;
    g.Cs = p.K; g.Cp = (g.Cs + TR::unit - 1) & ~(TR::unit - 1);
    g.M = p.batch * g.Hc * g.Wc; g.N = p.C;
    g.i0 = (g.ph + p.pt) % p.sh; g.j0 = (g.pw + p.pl) % p.sw;
    g.nti = g.i0 < p.KH ? (p.KH - g.i0 + p.sh - 1) / p.sh : 0;
    g.ntj = g.j0 < p.KW ? (p.KW - g.j0 + p.sw - 1) / p.sw : 0;
    g.dp0 = (g.ph + p.pt - g.i0) / p.sh; g.dq0 = (g.pw + p.pl - g.j0) / p.sw;
    g.ntaps = g.nti * g.ntj; g.Kdim = g.ntaps * g.Cp;
  } else {
    g.Cs = p.C; g.Cp = (g.Cs + TR::unit - 1) & ~(TR::unit - 1); g.ntaps = p.KH * p.KW;
    g.M = g.ntaps * g.Cp; g.N = p.K; g.Kdim = p.batch * p.OH * p.OW;
  }
  if (MODE != MODE_WGRAD && p.Nv > 0) g.N = p.Nv;      // only the first Nv output columns (acg_conv_desc dgrad_c / adj_dgrad_c)
  const int tiles_n = (g.N + BN - 1) / BN;
  // XCD-aware order: consecutive workgroup ids are dealt round-robin over the 8 XCDs (each with its own L2), so
  // give every XCD a CONTIGUOUS run of tiles - neighbours in the run share A rows / filter columns in that L2.
  // Bijective for any grid size; placement affects speed only.
  int bid = bx;
  if constexpr (MODE != MODE_WGRAD) {      // (weight gradients are placed by wgrad_xcd_map in the kernel wrappers)
    const int nwg = gx, q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  }
  g.tm = bid / tiles_n; g.tn = bid - g.tm * tiles_n;
  g.m0 = g.tm * BM; g.n0 = g.tn * BN;
  g.empty = g.m0 >= g.M;
  return g;
}

// K-steps [begin, end) of split bz out of `splits`
struct KRange { int begin, end; };
__device__ __forceinline__ KRange split_range(const int nk, const int splits, const int bz) {
  const int per = (nk + splits - 1) / splits;
  const int begin = bz * per;
  return KRange{begin, min(nk, begin + per)};
}

// ---- tap tables (element offsets), entry of thread tid: tapA = the tap's offset in the gathered tensor, tapB = in the filter ----
template <int MODE, class TR>
__device__ __forceinline__ void fill_taps(const ConvArgs& p, const TileGeom& g, int* tapA, int* tapB, const int tid) {
  if (tid < kMaxTaps && tid < g.ntaps) {
    const int t = tid;
    if constexpr (MODE == MODE_DGRAD) {
      const int ti = t / g.ntj, tj = t - ti * g.ntj;
      tapA[t] = -(ti * p.OW + tj) * TR::y_pitch(p);
      tapB[t] = ((g.i0 + p.sh * ti) * p.KW + (g.j0 + p.sw * tj)) * TR::tap_dgrad(p);
    } else {
      const int i = t / p.KW, j = t - i * p.KW;
      const int u = (MODE == MODE_FWD && p.tap_classes) ? tap_class_pos(i, j, p.KH, p.KW) : t;      // position in the K order
      tapA[u] = (i * p.W + j) * TR::x_pitch(p);
      tapB[u] = MODE == MODE_FWD ? t * TR::tap_fwd(p) : 0;      // FWD: the tap's first filter element (a weight gradient's dense operand is dy)
    }
  }
}

// ---- per-row gather info ---------------------------------------------------------------------------------------------------
// MODE_DGRAD: row r of the block's stride class.  Otherwise output pixel r = (b, p, q) of the forward convolution - a row of
// FWD, and a K position of WGRAD (conv_body: wgrad_rows).  Rows at or beyond `limit` carry zero masks.
// COMPACT: the kernel can be launched with p.compact (pixel-major rows).  LAYOUTS: off for a kernel that is never launched as
// the merged input gradient nor with slabs (conv_bf16_glds.h).
template <int MODE, class TR, bool COMPACT, bool LAYOUTS = true>
__device__ __forceinline__ RowInfo row_info(const ConvArgs& p, const TileGeom& g, const int r, const int limit) {
  RowInfo ri; ri.base = 0; ri.mask_lo = 0; ri.mask_hi = 0; ri.out_off = 0;
  if (r < limit) {
    if constexpr (MODE == MODE_DGRAD) {
      int w2, h2, b;
      if (COMPACT && p.compact) { b = r % p.batch; const int pq = r / p.batch; w2 = pq % g.Wc; h2 = pq / g.Wc; }     // pixel-major rows
      else { w2 = r % g.Wc; const int t2 = r / g.Wc; h2 = t2 % g.Hc; b = t2 / g.Hc; }
      const int y0 = h2 + g.dp0, x0 = w2 + g.dq0;  // dY coordinates of tap (0,0)
      ri.base = ((b * p.OH + y0) * p.OW + x0) * TR::y_pitch(p);
      ri.out_off = ((b * p.H + h2 * p.sh + g.ph) * p.W + (w2 * p.sw + g.pw)) * ((LAYOUTS && p.slab_rows) ? 4 : TR::dx_pitch(p));
      // tap (ti,tj) reads dY[y0 - ti][x0 - tj]
      const unsigned long long mk = tap_mask(max(0, y0 - p.OH + 1), min(g.nti, y0 + 1), max(0, x0 - p.OW + 1), min(g.ntj, x0 + 1), g.ntj);
      ri.mask_lo = (unsigned)mk; ri.mask_hi = (unsigned)(mk >> 32);
    } else {
      int q, b, pp;
      if (MODE == MODE_FWD && COMPACT && p.compact) { b = r % p.batch; const int px = r / p.batch; q = px % p.OW; pp = px / p.OW; }    // pixel-major rows
      else { const int t2 = div_fast(r, p.mg_ow, p.sh_ow); q = r - t2 * p.OW; b = div_fast(t2, p.mg_oh, p.sh_oh); pp = t2 - b * p.OH; }
      const int y0 = pp * p.sh - p.pt, x0 = q * p.sw - p.pl;
      ri.base = ((b * p.H + y0) * p.W + x0) * TR::x_pitch(p);
      if (LAYOUTS && p.shuf_c) ri.out_off = ((b * (2 * p.OH) + 2 * pp) * p.shuf_w + 2 * q) * p.shuf_pitch;     // merged input gradient (ConvArgs::shuf_c)
      else if (MODE == MODE_FWD && COMPACT && p.compact) ri.out_off = ((b * p.OH + pp) * p.OW + q) * (p.slab_rows ? 4 : TR::y_pitch(p));
      const unsigned long long m = (MODE == MODE_FWD && p.tap_classes) ? tap_mask_classes(max(0, -y0), min(p.KH, p.H - y0), max(0, -x0), min(p.KW, p.W - x0), p.KH, p.KW)
                                                                      : tap_mask(max(0, -y0), min(p.KH, p.H - y0), max(0, -x0), min(p.KW, p.W - x0), p.KW);
      ri.mask_lo = (unsigned)m; ri.mask_hi = (unsigned)(m >> 32);
    }
  }
  return ri;
}

// ---- tap compaction (p.compact, block-uniform; every thread of the block calls it, at least BM of them) ----------------------
// Keep only the taps a row of this tile can see: tap tables and row masks in compact order.  Returns the tile's own tap count
// (its Kdim is that times Cp).  rows / tapA / tapB must be complete (a barrier behind their fill).
template <int BM>
__device__ __forceinline__ int compact_taps(const int ntaps, RowInfo* rows, int* tapA, int* tapB, const int tid) {
  __shared__ unsigned umask[2];
  if (tid < 2) umask[tid] = 0u;
  __syncthreads();
  if (tid < BM) {
    const RowInfo ri = rows[tid];
    if (ri.mask_lo) atomicOr(&umask[0], ri.mask_lo);
    if (ri.mask_hi) atomicOr(&umask[1], ri.mask_hi);
  }
  __syncthreads();
  const unsigned long long U = (unsigned long long)umask[0] | ((unsigned long long)umask[1] << 32);
  int ta = 0, tb = 0;
  const bool mine = tid < ntaps && ((U >> tid) & 1ull);
  if (mine) { ta = tapA[tid]; tb = tapB[tid]; }
  unsigned long long rm = 0ull;        // this row's mask over the compact taps
  if (tid < BM) {
    const RowInfo ri = rows[tid];
    const unsigned long long old = (unsigned long long)ri.mask_lo | ((unsigned long long)ri.mask_hi << 32);
    int pos = 0;
    for (int t = 0; t < ntaps; ++t)
      if ((U >> t) & 1ull) { rm |= ((old >> t) & 1ull) << pos; ++pos; }
  }
  __syncthreads();
  if (mine) { const int pos = __popcll(U & ((1ull << tid) - 1ull)); tapA[pos] = ta; tapB[pos] = tb; }
  if (tid < BM) { rows[tid].mask_lo = (unsigned)rm; rows[tid].mask_hi = (unsigned)(rm >> 32); }
  __syncthreads();
  return __popcll(U);
}

// ---- output side ---------------------------------------------------------------------------------------------------------
// index of the block's BatchNorm partials (ConvArgs::stats): they start at stats + stats_block * 2 * N
template <int MODE>
__device__ __forceinline__ long long stats_block(const ConvArgs& p, const int by, const int tm) {
  int g = 0, blk;
  if constexpr (MODE == MODE_DGRAD) { blk = by * p.stats_tpg + tm; } else { g = tm / p.stats_tpg; blk = tm - g * p.stats_tpg; }
  return (long long)g * p.stats_nblk + blk;
}

// Element (m, n) of the contraction lies at row_base(m) + col_off(n) of the output tensor or slab.
template <int MODE, class TR, bool COMPACT, bool LAYOUTS>
struct OutMap {
  const ConvArgs& p;
  TileGeom g;
  // column term of an element's offset: n, or in the quad slab layout (ConvArgs::slab_rows; float32 slabs only) the quad's
  // run of rows + n & 3
  bool quads;
  // rows addressed by their out_off: DGRAD (a stride class), and of FWD the merged input gradient (columns = 2 x 2 pixel,
  // channel) and pixel-major small maps
  bool by_rows;
  long long row_pitch;

  __device__ __forceinline__ long long col_off(const int n) const {
    if (MODE == MODE_FWD && LAYOUTS && p.shuf_c > 0) { const int cls = n / p.shuf_c; return (long long)((cls >> 1) * p.shuf_w + (cls & 1)) * p.shuf_pitch + (n - cls * p.shuf_c); }
    return quads ? (long long)(n >> 2) * p.slab_rows * 4 + (n & 3) : (long long)n;
  }
  // false: no such row - a pad channel of the weight gradient, whose rows are (tap, channel) with the channels padded to Cp
  __device__ __forceinline__ bool row_base(const int m, const RowInfo* rows, const int row, long long& base) const {
    if (by_rows) {
      base = rows[row].out_off;
    } else if constexpr (MODE == MODE_WGRAD) {
      const int t = div_fast(m, p.mg_cp, p.sh_cp), c = m - t * g.Cp;      // (Cp == Cs: c < Cs always)
      if (c >= g.Cs) return false;
      base = ((long long)t * g.Cs + c) * g.N;
    } else {
      base = (long long)m * row_pitch;
    }
    return true;
  }
};
template <int MODE, class TR, bool COMPACT, bool LAYOUTS = true>
__device__ __forceinline__ OutMap<MODE, TR, COMPACT, LAYOUTS> out_map(const ConvArgs& p, const TileGeom& g) {
  const bool quads = LAYOUTS && MODE != MODE_WGRAD && p.slab_rows > 0;
  const bool shuf = MODE == MODE_FWD && LAYOUTS && (p.shuf_c > 0 || (COMPACT && p.compact));
  return OutMap<MODE, TR, COMPACT, LAYOUTS>{p, g, quads, MODE == MODE_DGRAD || shuf, MODE == MODE_WGRAD ? g.N : (quads ? 4 : TR::y_pitch(p))};
}

// The accumulators of a block to memory.  C/D layout of the 32 x 32 MFMAs: col = lane & 31 (lrow), row = (reg & 3) + 8 * (reg >> 2)
// + 4 * (lane >> 5) (lk); the wave's sub-tile starts at (wm0, wn0).  HALF: the tensor may be bf16 - it is when to_bf16.
// Full tiles take a straight-line path - one base per 32 x 32 sub-tile, sixteen stores at row strides - instead of a bounds
// test, a branch and a 64-bit index multiply per element.  (The general loop below costs ~1600 instructions and ~190 branches
// per thread on a 128 x 128 tile: 4.8 us of an 8.7 us one-K-step launch, tools/fixed_cost_probe.py.)
// (rows full; a ragged last column tile - 3, 6, 25, 121 or 138 output channels - only masks lanes, once per 32-column sub-tile)
template <int MODE, int BM, int TA, int TB, bool HALF, class Acc, class Map>
__device__ __forceinline__ void store_tile(const Acc& acc, const Map& map, const RowInfo* rows, float* const outf, const bool to_bf16,
                                           const int wm0, const int wn0, const int lrow, const int lk) {
  const ConvArgs& p = map.p;
  const int M = map.g.M, N = map.g.N, m0 = map.g.m0, n0 = map.g.n0;
  __bf16* const outh = reinterpret_cast<__bf16*>(p.out);
  const bool acc_out = MODE == MODE_WGRAD && p.splits == 1 && p.accumulate != 0.f;
  const bool full = m0 + BM <= M && (MODE != MODE_WGRAD || (map.g.Cp == map.g.Cs && !acc_out));
  if (full) {
    auto store_rows = [&](auto* base, long long pitch, int a, int b) {
      using T = std::remove_pointer_t<decltype(base)>;
#pragma unroll
      for (int r = 0; r < 16; ++r) base[(long long)((r & 3) + 8 * (r >> 2)) * pitch] = (T)acc[a][b][r];
    };
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      if (n0 + wn0 + 32 * b + lrow < N) {
        const long long co = map.col_off(n0 + wn0 + 32 * b + lrow);
        if (map.by_rows) {
#pragma unroll
          for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const long long off = (long long)rows[wm0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lk].out_off + co;
              if constexpr (HALF) { if (to_bf16) outh[off] = (__bf16)acc[a][b][r]; else outf[off] = acc[a][b][r]; }
              else outf[off] = acc[a][b][r];
            }
        } else {
#pragma unroll
          for (int a = 0; a < TA; ++a) {
            const long long o = (long long)(m0 + wm0 + 32 * a + 4 * lk) * map.row_pitch + co;
            if constexpr (HALF) { if (to_bf16) store_rows(outh + o, map.row_pitch, a, b); else store_rows(outf + o, map.row_pitch, a, b); }
            else store_rows(outf + o, map.row_pitch, a, b);
          }
        }
      }
    }
    return;
  }
  // partial row tiles (the last tile of a weight gradient whose taps x channels is no multiple of the tile; tiny layers): per
  // ROW one validity test and one base index (the weight gradient's division by the padded channel count included), per
  // element only the column mask
#pragma unroll
  for (int a = 0; a < TA; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lk;
      const int m = m0 + row;
      if (m >= M) continue;
      long long base;
      if (!map.row_base(m, rows, row, base)) continue;
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        const int n = n0 + wn0 + 32 * b + lrow;
        if (n < N) {
          const long long o = base + map.col_off(n);
          float v = acc[a][b][r];
          if (HALF && to_bf16) {
            outh[o] = (__bf16)v;
          } else {
            if (acc_out) v += p.accumulate * outf[o];
            outf[o] = v;
          }
        }
      }
    }
}

// ---- host: the geometry fields of ConvArgs from a descriptor ------------------------------------------------------------------
// batch ... pl, Cx, Ky, Nv, the three magic dividers, compact, tap_classes, slab_rows.  `which`: ACG_CONV_*; bf16: the storage.
struct GeomFlags {
  int compact_max;      // small maps (ConvArgs::compact): at most this many pixels per image (DGRAD: per stride class); 0 = never
  bool tap_classes;     // strided forward convolutions walk their taps class by class (ConvArgs::tap_classes)
  bool quad_slabs;      // the slabs are written in the ACG_SLABS_QUADS layout (ConvArgs::slab_rows)
};
static inline void fill_geometry(ConvArgs& a, const acg_conv_desc& d, const int which, const bool bf16, const GeomFlags& f) {
  const int unit = bf16 ? 8 : 4;
  a.Cx = d.in_pitch > 0 ? d.in_pitch : d.in_c;
  a.Ky = d.out_pitch > 0 ? d.out_pitch : d.out_c;
  a.batch = d.batch; a.H = d.in_h; a.W = d.in_w; a.C = d.in_c; a.OH = d.out_h; a.OW = d.out_w; a.K = d.out_c;
  a.KH = d.kh; a.KW = d.kw; a.sh = d.stride_h; a.sw = d.stride_w; a.pt = d.pad_top; a.pl = d.pad_left;
  a.Nv = which == ACG_CONV_DGRAD ? d.dgrad_c : (which == ACG_CONV_FWD ? d.adj_dgrad_c : 0);
  a.tap_classes = (f.tap_classes && which == ACG_CONV_FWD && d.stride_h == 2 && d.stride_w == 2 && d.kh * d.kw > 1 && d.kh * d.kw <= 64) ? 1 : 0;
  // measured: compact pays only where more than half of the taps are dead (a 4 x 4 map under a 5 x 5 / stride-2 filter: d/conv5) -
  // from 16 pixels per class on, what the pixel-major order loses in gather reuse inside a tile eats the skipped K-steps
  const int hc = (d.in_h + d.stride_h - 1) / d.stride_h, wc = (d.in_w + d.stride_w - 1) / d.stride_w;
  const int px = which == ACG_CONV_DGRAD ? hc * wc : d.out_h * d.out_w;
  a.compact = (which != ACG_CONV_WGRAD && !bf16 && px <= f.compact_max && d.batch >= 8 && d.kh * d.kw > 1) ? 1 : 0;
  const long long orows = which == ACG_CONV_DGRAD ? (long long)d.batch * d.in_h * d.in_w : (long long)d.batch * d.out_h * d.out_w;
  a.slab_rows = f.quad_slabs ? (int)orows : 0;
  const FastDiv fw = fast_div(d.out_w), fh = fast_div(d.out_h);
  a.mg_ow = fw.magic; a.sh_ow = fw.shift; a.mg_oh = fh.magic; a.sh_oh = fh.shift;
  const FastDiv fc = fast_div(((which == ACG_CONV_DGRAD ? d.out_c : d.in_c) + unit - 1) & ~(unit - 1));
  a.mg_cp = fc.magic; a.sh_cp = fc.shift;
}

}  // namespace acgconv
