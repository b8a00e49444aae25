// The row table of the weight gradient's UW loaders on the host: conv_tile.h's straight-line forms - bit_range, tap_mask_closed,
// wgrad_row - against the looped forms they replace and against a bit-by-bit enumeration.  Integer code only; compiled with the
// host sanitizers by tests/test_conv_wgrad_row_host.py, like conv_tile_host.cpp.
//
//   wgrad_row_host masks                       every filter KH x KW of at most 64 taps, every (lo, hi) pair of both ranges
//   wgrad_row_host rows B H W KH KW SH SW PT PL OH OW CX EXTRA
//                                              every pixel row of the shape, and EXTRA rows beyond it, against row_info
// Prints "checked N" and exits 0, or prints the first mismatches and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hip/hip_runtime.h"
#include "../../action_conditioned_gans_amd/csrc/conv_tile.h"

using namespace acgconv;

// bits (a * nb + b), a in [lo_a, hi_a), b in [lo_b, hi_b): the definition
static unsigned long long mask_by_bits(int lo_a, int hi_a, int lo_b, int hi_b, int nb) {
  unsigned long long m = 0ull;
  for (int a = lo_a; a < hi_a; ++a)
    for (int b = lo_b; b < hi_b; ++b) m |= 1ull << (a * nb + b);
  return m;
}

static int masks() {
  long n = 0, bad = 0;
  for (int lo = 0; lo <= 64; ++lo)
    for (int hi = -1; hi <= 64; ++hi) {
      unsigned long long want = 0ull;
      for (int b = lo; b < hi; ++b) want |= 1ull << b;
      ++n;
      if (bit_range(lo, hi) != want && bad++ < 8) printf("bit_range(%d, %d)\n", lo, hi);
    }
  for (int KH = 1; KH <= 64; ++KH)
    for (int KW = 1; KH * KW <= 64; ++KW) {
      const unsigned long long rep = tap_rep(KH, KW);
      for (int la = 0; la <= KH; ++la)
        for (int ha = -1; ha <= KH; ++ha)
          for (int lb = 0; lb <= KW; ++lb)
            for (int hb = -1; hb <= KW; ++hb) {
              const unsigned long long got = tap_mask_closed(la, ha, lb, hb, KW, rep);
              ++n;
              if (got != mask_by_bits(la, ha, lb, hb, KW) && bad++ < 8) printf("closed form: %d x %d rows [%d, %d) columns [%d, %d)\n", KH, KW, la, ha, lb, hb);
              // the looped form shifts by the range's width: defined below 64 columns
              if (hb - lb < 64 && got != tap_mask(la, ha, lb, hb, KW) && bad++ < 8) printf("tap_mask: %d x %d rows [%d, %d) columns [%d, %d)\n", KH, KW, la, ha, lb, hb);
            }
    }
  printf("checked %ld\n", n);
  return bad != 0;
}

static int rows(char** v) {
  ConvArgs p{};
  p.batch = atoi(v[0]); p.H = atoi(v[1]); p.W = atoi(v[2]); p.KH = atoi(v[3]); p.KW = atoi(v[4]); p.sh = atoi(v[5]); p.sw = atoi(v[6]);
  p.pt = atoi(v[7]); p.pl = atoi(v[8]); p.OH = atoi(v[9]); p.OW = atoi(v[10]); p.Cx = atoi(v[11]); p.C = p.Cx; p.K = p.Ky = 4;
  const int extra = atoi(v[12]);
  const FastDiv fw = fast_div(p.OW), fh = fast_div(p.OH);
  p.mg_ow = fw.magic; p.sh_ow = fw.shift; p.mg_oh = fh.magic; p.sh_oh = fh.shift;
  TileGeom g{};
  const int Kdim = p.batch * p.OH * p.OW, shift = (p.pt * p.W + p.pl) * p.Cx;
  const unsigned long long rep = tap_rep(p.KH, p.KW);
  long n = 0, bad = 0;
  for (int r = 0; r < Kdim + extra; ++r) {
    const RowInfo ri = row_info<MODE_WGRAD, F32Tensors, false>(p, g, r, Kdim);
    const WgradRow w = wgrad_row<F32Tensors>(p, r, Kdim, shift, rep);
    // in range: the same masks, complemented; the byte offset from the padding corner, never negative.  Beyond: all dead, offset 0.
    const bool ok = w.inv_lo == ~ri.mask_lo && w.inv_hi == ~ri.mask_hi &&
                    (r >= Kdim ? (w.off == 0u && w.inv_lo == ~0u && w.inv_hi == ~0u) : (ri.base + shift >= 0 && w.off == (unsigned)(ri.base + shift) * 4u));
    ++n;
    if (!ok && bad++ < 8) printf("row %d: off %u inv %08x %08x against base %d masks %08x %08x\n", r, w.off, w.inv_lo, w.inv_hi, ri.base, ri.mask_lo, ri.mask_hi);
  }
  printf("checked %ld\n", n);
  return bad != 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "masks")) return masks();
  if (argc == 15 && !strcmp(argv[1], "rows")) return rows(argv + 2);
  fprintf(stderr, "usage: wgrad_row_host masks | rows B H W KH KW SH SW PT PL OH OW CX EXTRA\n");
  return 2;
}
