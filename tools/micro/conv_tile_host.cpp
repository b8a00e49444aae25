// csrc/conv_tile.h - the header itself, not a restatement - compiled as plain C++ for the host against
// tools/micro/hip_host/hip/hip_runtime.h.  For one descriptor it runs what every block program of the convolution kernels runs
// around its K loop - fill_geometry, tile_geometry, fill_taps, row_info, compact_taps, out_map - for every block of the grid and
// writes out every address that comes of it; tests/test_conv_tile_host.py holds them against the definition of the convolution.
// Built with the host sanitizers (host code only, nothing for a GPU): rows, tapA and tapB are exact-size heap blocks.
//   hipcc -x c++ -std=c++17 -O1 -Xarch_host -fsanitize=address,undefined -Itools/micro/hip_host -pthread tools/micro/conv_tile_host.cpp -o conv_tile_host
//   conv_tile_host out.txt which unit BM BN compact_max tap_classes quad_slabs  batch in_h in_w in_c out_h out_w out_c kh kw stride_h
//                  stride_w pad_top pad_left in_pitch out_pitch dgrad_c adj_dgrad_c
//       which: 0 FWD, 1 DGRAD, 2 WGRAD; unit: 4 (float32 tensors) or 8 (bf16)
// Output, one line per item (all offsets in elements):
//   G gx gy N                                   the grid (x: tiles, y: stride classes) and the columns computed
//   B by bx empty m0 n0 M ntaps Kdim Cp Cs      a block; ntaps / Kdim after the tap compaction
//   R row out_off  {gather tapB c} x Kdim       a tile row (WGRAD: a pixel of the reduction): per K position k = (tap t, channel c) in
//                                               the tile's tap order, the gather offset base + tapA[t] + c or -1 = masked (tap_ok
//                                               false or c >= Cs), the tap's filter offset tapB[t], and c
//   O row n0 count  {offset} x count            the output offsets row_base + col_off(n) of the row's columns n0 .. n0 + count - 1
//   W m valid base                              WGRAD: output row m = (tap, padded channel) -> row_base
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
pthread_barrier_t emu_barrier;
double emu_exchange[1024];
#include "../../action_conditioned_gans_amd/csrc/conv_tile.h"

using namespace acgconv;

static FILE* out;

// compact_taps is a block-wide step with barriers: 256 real threads, as emu_launch runs a kernel's block
template <int BM>
static int run_compact(int ntaps, RowInfo* rows, int* tapA, int* tapB) {
  int result[256];
  pthread_barrier_init(&emu_barrier, nullptr, 256);
  std::vector<std::thread> ts;
  for (int t = 0; t < 256; ++t) ts.emplace_back([=, &result]() { result[t] = compact_taps<BM>(ntaps, rows, tapA, tapB, t); });
  for (auto& t : ts) t.join();
  pthread_barrier_destroy(&emu_barrier);
  for (int t = 1; t < 256; ++t)
    if (result[t] != result[0]) { fprintf(stderr, "compact_taps: the threads disagree\n"); exit(3); }
  return result[0];
}

static void print_row(const ConvArgs& p, const TileGeom& g, const RowInfo& ri, int row, const int* tapA, const int* tapB) {
  (void)p;
  fprintf(out, "R %d %d ", row, ri.out_off);
  for (int k = 0; k < g.Kdim; ++k) {
    const int t = k / g.Cp, c = k - t * g.Cp;
    const bool ok = tap_ok(ri, t) && c < g.Cs;
    fprintf(out, " %d %d %d", ok ? ri.base + tapA[t] + c : -1, tapB[t], c);
  }
  fputc('\n', out);
}

template <int MODE, class TR, bool COMPACT>
static int run(const ConvArgs& p, int BM, int BN) {
  const TileGeom g0 = tile_geometry<MODE, TR>(p, 0, 0, 1, BM, BN);      // class 0: the largest
  if (MODE == MODE_WGRAD) {
    // the weight gradient: row infos of every pixel of the reduction, as conv_body's wgrad_rows derives them; the output rows
    RowInfo* rows = (RowInfo*)aligned_alloc(16, sizeof(RowInfo) * (size_t)g0.Kdim);
    int* tapA = (int*)malloc(sizeof(int) * g0.ntaps);
    int* tapB = (int*)malloc(sizeof(int) * g0.ntaps);
    for (int tid = 0; tid < 256; ++tid) fill_taps<MODE, TR>(p, g0, tapA, tapB, tid);
    for (int r = 0; r < g0.Kdim; ++r) rows[r] = row_info<MODE, TR, false>(p, g0, r, g0.Kdim);
    fprintf(out, "G 1 1 %d\nB 0 0 0 0 0 %d %d %d %d %d\n", g0.N, g0.Kdim, g0.ntaps, g0.ntaps * g0.Cp, g0.Cp, g0.Cs);
    TileGeom gk = g0;
    gk.Kdim = g0.ntaps * g0.Cp;      // a pixel's gathers: every (tap, channel)
    for (int r = 0; r < g0.Kdim; ++r) print_row(p, gk, rows[r], r, tapA, tapB);
    const RowInfo beyond = row_info<MODE, TR, false>(p, g0, g0.Kdim, g0.Kdim);
    if (beyond.mask_lo || beyond.mask_hi) { fprintf(stderr, "a row beyond the limit carries a mask\n"); return 4; }
    const auto map = out_map<MODE, TR, false>(p, g0);
    for (int m = 0; m < g0.M; ++m) {
      long long base = -1;
      const bool ok = map.row_base(m, rows, 0, base);
      fprintf(out, "W %d %d %lld\n", m, ok ? 1 : 0, ok ? base : -1ll);
      if (ok) {
        fprintf(out, "O %d 0 %d ", m, g0.N);
        for (int n = 0; n < g0.N; ++n) fprintf(out, " %lld", base + map.col_off(n));
        fputc('\n', out);
      }
    }
    free(rows); free(tapA); free(tapB);
    return 0;
  }
  const int gy = MODE == MODE_DGRAD ? p.sh * p.sw : 1;
  const int gx = ((g0.M + BM - 1) / BM) * ((g0.N + BN - 1) / BN);
  fprintf(out, "G %d %d %d\n", gx, gy, g0.N);
  for (int by = 0; by < gy; ++by)
    for (int bx = 0; bx < gx; ++bx) {
      TileGeom g = tile_geometry<MODE, TR>(p, bx, by, gx, BM, BN);
      if (g.empty) { fprintf(out, "B %d %d 1 %d %d %d 0 0 %d %d\n", by, bx, g.m0, g.n0, g.M, g.Cp, g.Cs); continue; }
      RowInfo* rows = (RowInfo*)aligned_alloc(16, sizeof(RowInfo) * (size_t)BM);
      int* tapA = (int*)malloc(sizeof(int) * (g.ntaps > 0 ? g.ntaps : 1));
      int* tapB = (int*)malloc(sizeof(int) * (g.ntaps > 0 ? g.ntaps : 1));
      for (int tid = 0; tid < 256; ++tid) {      // the block's threads in turn: nothing here waits for another thread
        fill_taps<MODE, TR>(p, g, tapA, tapB, tid);
        for (int r = tid; r < BM; r += 256) rows[r] = row_info<MODE, TR, COMPACT>(p, g, g.m0 + r, g.M);
      }
      if (COMPACT && p.compact) {
        g.ntaps = BM == 64 ? run_compact<64>(g.ntaps, rows, tapA, tapB) : BM == 128 ? run_compact<128>(g.ntaps, rows, tapA, tapB) : run_compact<256>(g.ntaps, rows, tapA, tapB);
        g.Kdim = g.ntaps * g.Cp;
      }
      fprintf(out, "B %d %d 0 %d %d %d %d %d %d %d\n", by, bx, g.m0, g.n0, g.M, g.ntaps, g.Kdim, g.Cp, g.Cs);
      const auto map = out_map<MODE, TR, COMPACT>(p, g);
      for (int row = 0; row < BM; ++row) {
        print_row(p, g, rows[row], row, tapA, tapB);
        const int m = g.m0 + row;
        long long base = -1;
        if (m >= g.M || !map.row_base(m, rows, row, base)) continue;
        const int cnt = min(BN, g.N - g.n0);
        fprintf(out, "O %d %d %d ", row, g.n0, cnt);
        for (int n = g.n0; n < g.n0 + cnt; ++n) fprintf(out, " %lld", base + map.col_off(n));
        fputc('\n', out);
      }
      free(rows); free(tapA); free(tapB);
    }
  return 0;
}

template <class TR, bool COMPACT>
static int run_mode(int which, const ConvArgs& p, int BM, int BN) {
  if (which == ACG_CONV_FWD) return run<MODE_FWD, TR, COMPACT>(p, BM, BN);
  if (which == ACG_CONV_DGRAD) return run<MODE_DGRAD, TR, COMPACT>(p, BM, BN);
  return run<MODE_WGRAD, TR, false>(p, BM, BN);
}

int main(int argc, char** argv) {
  if (argc != 26) { fprintf(stderr, "conv_tile_host: 25 arguments, see the head of the source\n"); return 1; }
  int v[24];
  for (int i = 0; i < 24; ++i) v[i] = atoi(argv[2 + i]);
  const int which = v[0], unit = v[1], BM = v[2], BN = v[3];
  if ((unit != 4 && unit != 8) || (BM != 64 && BM != 128 && BM != 256) || BN < 32 || BN % 32 || which < 0 || which > 2) return 1;
  const GeomFlags flags{v[4], v[5] != 0, v[6] != 0};
  acg_conv_desc d;
  memset(&d, 0, sizeof d);
  d.batch = v[7]; d.in_h = v[8]; d.in_w = v[9]; d.in_c = v[10]; d.out_h = v[11]; d.out_w = v[12]; d.out_c = v[13]; d.kh = v[14]; d.kw = v[15];
  d.stride_h = v[16]; d.stride_w = v[17]; d.pad_top = v[18]; d.pad_left = v[19]; d.in_pitch = v[20]; d.out_pitch = v[21]; d.dgrad_c = v[22];
  d.adj_dgrad_c = v[23];
  ConvArgs p;
  memset(&p, 0, sizeof p);
  p.splits = 1;
  fill_geometry(p, d, which, unit == 8, flags);      // the library's own code (conv_f32.hip prepare)
  out = fopen(argv[1], "w");
  if (!out) return 2;
  fprintf(out, "A %d %d %d %d\n", p.compact, p.tap_classes, p.slab_rows, p.Nv);
  // the float32 forward / input-gradient kernels are the ones compiled with the small-map path (conv_f32_kernel.h: COMPACT)
  const int rc = unit == 4 ? run_mode<F32Tensors, true>(which, p, BM, BN) : run_mode<Bf16Tensors<>, false>(which, p, BM, BN);
  fclose(out);
  return rc;
}
