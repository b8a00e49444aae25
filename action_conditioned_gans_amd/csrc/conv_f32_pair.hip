// Instantiates the paired launches (input gradient + weight gradient of one layer in one grid), see conv_f32_kernel.h.
#include "conv_f32_kernel.h"

namespace acgconv {

namespace {
template <int MODE_A, int BMA, int BNA, int WMA, int WNA, bool RAGGED, bool LIN_A, bool UK_A, bool UW_B>
void launch_b(const Plan& pb, const ConvArgs& a, const ConvArgs& b, const PairGeom& g, unsigned blocks, hipStream_t st) {
  // A 64x64 weight gradient beside a 128x32 A keeps the generic loaders: that launch holds three blocks per CU either way (A's
  // 43528 B of LDS) and measured 1.7 % slower with UW in three traces out of three (profiles/wgrad_uniform/README.md).
  constexpr bool UW64 = UW_B && BMA == 64;
  if (pb.cfg == 2) ACG_LAUNCH((conv_pair_f32<MODE_A, BMA, BNA, WMA, WNA, 128, 32, 4, 1, RAGGED, LIN_A, UK_A, UW_B>), dim3(blocks), dim3(256), 0, st, a, b, g);
  else ACG_LAUNCH((conv_pair_f32<MODE_A, BMA, BNA, WMA, WNA, 64, 64, 2, 2, RAGGED, LIN_A, UK_A, UW64>), dim3(blocks), dim3(256), 0, st, a, b, g);
}
// (the weight gradient B takes its UW variant by its own rule, whatever A runs; a ragged pair never does)
template <int MODE_A, bool RAGGED, bool LIN_A = false, bool UK_A = false>
void launch_a(const Plan& pa, const Plan& pb, const ConvArgs& a, const ConvArgs& b, const PairGeom& g, unsigned blocks, hipStream_t st) {
  if constexpr (!RAGGED) {
    if (uniform_w_variant(MODE_WGRAD, pb, b)) {
      if (pa.cfg == 2) launch_b<MODE_A, 128, 32, 4, 1, RAGGED, LIN_A, UK_A, true>(pb, a, b, g, blocks, st);
      else launch_b<MODE_A, 64, 64, 2, 2, RAGGED, LIN_A, UK_A, true>(pb, a, b, g, blocks, st);
      return;
    }
  }
  if (pa.cfg == 2) launch_b<MODE_A, 128, 32, 4, 1, RAGGED, LIN_A, UK_A, false>(pb, a, b, g, blocks, st);
  else launch_b<MODE_A, 64, 64, 2, 2, RAGGED, LIN_A, UK_A, false>(pb, a, b, g, blocks, st);
}
}  // namespace

int launch_pair(int modeA, const Plan& pa, const ConvArgs& a, const Plan& pb, const ConvArgs& b, hipStream_t st) {
  PairGeom g;
  g.gxA = (int)(acg::ceil_div(pa.M, pa.bm) * acg::ceil_div(pa.N, pa.bn));
  g.gyA = pa.classes;
  g.nA = g.gxA * g.gyA * pa.splits;
  g.gxB = (int)(acg::ceil_div(pb.M, pb.bm) * acg::ceil_div(pb.N, pb.bn));
  const unsigned blocks = (unsigned)(g.nA + g.gxB * pb.splits);
  if (modeA == MODE_FWD) {
    // (pair_supported: the dense operands are float4-able; gathered channels a multiple of 4 -> the LIN variant of A)
    if (pa.ragged) launch_a<MODE_FWD, true>(pa, pb, a, b, g, blocks, st);
    else if (uniform_k_variant(MODE_FWD, pa, a)) launch_a<MODE_FWD, false, true, true>(pa, pb, a, b, g, blocks, st);
    else if (lin_variant(MODE_FWD, pa, a)) launch_a<MODE_FWD, false, true>(pa, pb, a, b, g, blocks, st);
    else launch_a<MODE_FWD, false>(pa, pb, a, b, g, blocks, st);
  } else {
    if (pa.ragged) launch_a<MODE_DGRAD, true>(pa, pb, a, b, g, blocks, st);
    else if (uniform_k_variant(MODE_DGRAD, pa, a)) launch_a<MODE_DGRAD, false, false, true>(pa, pb, a, b, g, blocks, st);
    else launch_a<MODE_DGRAD, false>(pa, pb, a, b, g, blocks, st);
  }
  return acg::check_launch("conv_pair_f32");
}

}  // namespace acgconv
