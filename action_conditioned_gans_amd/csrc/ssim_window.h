// The windowed-moments pass of SSIM, shared by the metric (metrics.hip) and the training loss (ssim_loss.hip): the 11 x 11
// Gaussian window (sigma 1.5, normalised to sum 1, VALID filtering) run over x, y, x^2, y^2 and (x - y)^2.
//
// One block = one frame x one strip of <= 64 output columns x one band of output rows, one wave per channel (lane = output
// column).  The band's input rows go through LDS in chunks of 11 (coalesced, 16-byte loads where the rows allow them); each
// lane runs the horizontal 11-tap pass of its column on the five quantities and adds the result into a ring of 11 vertical
// accumulators (row r feeds the outputs r-10..r), so the vertical pass needs no second LDS round trip; the output whose
// window ended at this row is handed to the caller's epilogue and the ring slot is reused.
//
// Contraction.  This header sets no `#pragma clang fp contract`: a template takes the mode in force where its text is included,
// not where it is instantiated.  ssim_loss.hip includes it under contract(off) (its three kinds of call must agree to the bit:
// every fused operation is an explicit fmaf), metrics.hip under hipcc's default, which fuses `h[0] += g * x` as it always has.
// Each entry keeps its bits only as long as that stays so.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "common.h"

namespace acg {
namespace ssim {

constexpr int kTaps = 11, kHalo = kTaps - 1;
constexpr int kStrip = 64;                  // output columns per block (one per lane)
constexpr int kCols = kStrip + kHalo;       // input columns a strip reads
constexpr int kLdsCols = kCols + 2;         // (row pitch in LDS)
constexpr int kMaxC = 4;

struct Window {
  float g[kTaps];
};

inline Window gaussian_window() {
  double g[kTaps], s = 0.0;
  for (int t = 0; t < kTaps; ++t) { const double u = t - kHalo / 2; g[t] = exp(-u * u / (2.0 * 1.5 * 1.5)); s += g[t]; }
  Window w;
  for (int t = 0; t < kTaps; ++t) w.g[t] = (float)(g[t] / s);
  return w;
}

inline bool aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

// Blocking of a rows x cols field of outputs, shared by the workspace queries and the launches: strips of 64 columns, bands of
// rows halved while the grid has fewer than min_blocks blocks and the band is longer than min_band rows.
struct Plan {
  int rows, cols, strips, band, bands;
  __host__ __device__ long long blocks_per_frame() const { return (long long)strips * bands; }
};

inline Plan plan_for(int n, int rows, int cols, int min_blocks, int min_band) {
  Plan p;
  p.rows = rows;
  p.cols = cols;
  p.strips = (cols + kStrip - 1) / kStrip;
  p.band = rows;
  while ((long long)n * p.strips * ((rows + p.band - 1) / p.band) < min_blocks && p.band > min_band) p.band = (p.band + 1) / 2;
  p.bands = (rows + p.band - 1) / p.band;
  return p;
}

// What a block (blockDim.x = 64 * C) works on: outputs [p0, p0 + rows_out) x [q0, q0 + 64) of frame n, read from the rows_in x
// cols_in inputs that start at the same (p0, q0) (the input field is 10 rows and 10 columns larger than the output field).
struct Tile {
  long long n;
  int strip, band, q0, p0, rows_out, rows_in, cols_in, c, lane;
};

__device__ __forceinline__ Tile tile_of(const Plan& pl) {
  Tile t;
  const long long bpf = pl.blocks_per_frame();
  t.n = blockIdx.x / bpf;
  const int b = (int)(blockIdx.x - t.n * bpf);
  t.strip = b % pl.strips;
  t.band = b / pl.strips;
  t.q0 = t.strip * kStrip;
  t.p0 = t.band * pl.band;
  t.rows_out = min(pl.band, pl.rows - t.p0);
  t.rows_in = t.rows_out + kHalo;
  t.cols_in = min(kCols, pl.cols + kHalo - t.q0);
  t.c = threadIdx.x >> 6;
  t.lane = threadIdx.x & 63;
  return t;
}

// Rows [row0, row0 + nr) x columns [q0, q0 + cols_in) of one frame of pred and truth into xs, ys, by the whole block.
// VEC: 16-byte (fp32) / 8-byte (bf16) loads; needs W * P a multiple of 4 and both frames aligned to a vector.
template <bool VEC, typename TA, typename TB>
__device__ __forceinline__ void stage_rows(const TA* __restrict__ pred, const TB* __restrict__ truth, float (&xs)[kMaxC][kTaps][kLdsCols],
                                           float (&ys)[kMaxC][kTaps][kLdsCols], size_t frame, size_t row_elems, int row0, int q0, int nr,
                                           int cols_in, int C, int P) {
  const int seg = cols_in * P;  // elements of one input row this block reads
  if constexpr (VEC) {
    const int seg4 = (seg + 3) >> 2;  // rows and q0 * P are multiples of 4 elements: a vector never crosses the row end
    for (int e = threadIdx.x; e < nr * seg4; e += blockDim.x) {
      const int i = e / seg4, e4 = (e - i * seg4) << 2;
      const size_t o = frame + (size_t)(row0 + i) * row_elems + (size_t)q0 * P + e4;
      float vx[4], vy[4];
      acg::ldv<4>(pred + o, vx);
      acg::ldv<4>(truth + o, vy);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int el = e4 + j, col = el / P, ch = el - col * P;
        if (col < cols_in && ch < C) { xs[ch][i][col] = vx[j]; ys[ch][i][col] = vy[j]; }
      }
    }
  } else {
    for (int e = threadIdx.x; e < nr * seg; e += blockDim.x) {
      const int i = e / seg, el = e - i * seg, col = el / P, ch = el - col * P;
      if (ch < C) {
        const size_t o = frame + (size_t)(row0 + i) * row_elems + (size_t)q0 * P + el;
        xs[ch][i][col] = (float)pred[o];
        ys[ch][i][col] = (float)truth[o];
      }
    }
  }
}

// The pass over one tile of [n][H][W][P] frames (P >= C: the channel pitch) whose outputs pl blocks.  xs, ys: the block's LDS.
// sx, sy: the constants this thread's channel is moved by before anything is squared.  The epilogue has two hooks, both called by
// the threads of a live channel (c < C) only:
//   ep.row(r, x, y)    - band row r is staged: x, y are its LDS rows of this channel (unshifted; column 0 is frame column q0);
//   ep.position(p, m)  - output row p >= 0 of the band, column q0 + lane < pl.cols, is complete: m = the window's means of
//                        x', y', x'^2, y'^2, (x' - y')^2 (x' = x - sx, y' = y - sy).
// Registers: ssim_partial_k sits just under 128 VGPRs (4 waves per SIMD), and hipcc goes past 160 when the epilogue is handed
// over by reference or when the loader's loops stand in this body.  So the epilogue goes in by value and comes back with what it
// summed, and the loader is a function of its own (profiles/ssim_loss/resource_usage.txt).
template <bool VEC, typename TA, typename TB, typename E>
__device__ __forceinline__ E moments_pass(const TA* __restrict__ pred, const TB* __restrict__ truth, float (&xs)[kMaxC][kTaps][kLdsCols],
                                          float (&ys)[kMaxC][kTaps][kLdsCols], const Tile& tl, const Plan& pl, int H, int W, int C, int P,
                                          const Window& win, float sx, float sy, E ep) {
  const int c = tl.c, lane = tl.lane, q0 = tl.q0, p0 = tl.p0, rows_in = tl.rows_in, cols_in = tl.cols_in;
  const size_t frame = (size_t)tl.n * H * W * P;
  const size_t row_elems = (size_t)W * P;
  const bool col_ok = q0 + lane < pl.cols;

  float acc[kTaps][5];
#pragma unroll
  for (int s = 0; s < kTaps; ++s)
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[s][k] = 0.f;

  for (int r0 = 0; r0 < rows_in; r0 += kTaps) {
    const int nr = min(kTaps, rows_in - r0);
    __syncthreads();  // the previous chunk has been read
    stage_rows<VEC>(pred, truth, xs, ys, frame, row_elems, p0 + r0, q0, nr, cols_in, C, P);
    __syncthreads();
    if (c < C) {
#pragma unroll
      for (int i = 0; i < kTaps; ++i) {
        if (i < nr) {
          const int r = r0 + i;
          ep.row(r, xs[c][i], ys[c][i]);
          // horizontal pass (columns past the frame's edge hold stale values: they only reach outputs with col_ok false)
          float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < kTaps; ++t) {
            const float x = xs[c][i][lane + t] - sx, y = ys[c][i][lane + t] - sy, d = x - y, g = win.g[t];
            const float gx = g * x, gy = g * y, gd = g * d;
            h[0] = h[0] + gx;
            h[1] = h[1] + gy;
            h[2] = fmaf(gx, x, h[2]);
            h[3] = fmaf(gy, y, h[3]);
            h[4] = fmaf(gd, d, h[4]);
          }
          // vertical pass: input row r feeds output row r - k with weight g[k]; the slot of output p is p mod 11 = (r - k) mod 11
          // and r = r0 + i with r0 a multiple of 11, so every slot index is a compile-time constant.  Outputs p < 0 land in
          // slots that are cleared below before their own first row.
#pragma unroll
          for (int k = 0; k < kTaps; ++k) {
            const int s = (i - k + kTaps) % kTaps;
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[s][q] = fmaf(win.g[k], h[q], acc[s][q]);
          }
          // output p = r - 10 is complete (slot (i + 1) mod 11)
          const int s = (i + 1) % kTaps;
          const int p = r - kHalo;
          if (p >= 0 && col_ok) ep.position(p, acc[s]);
#pragma unroll
          for (int q = 0; q < 5; ++q) acc[s][q] = 0.f;
        }
      }
    }
  }
  return ep;
}

}  // namespace ssim
}  // namespace acg
