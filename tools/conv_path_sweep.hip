// The conv planner of conv_f32.hip as a table, on the CPU: which kernel family, tile, split count, template switches and
// reduction a convolution call would launch - no GPU, no launch.  The sibling of bn_path_sweep.hip: it compiles the planner's own
// source with the launch functions stubbed out and answers through acg_conv2d_path / acg_conv2d_pair_path (acgan_conv_plan.h).
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/conv_path_sweep.hip -o /tmp/conv_path_sweep
//   PYTHONPATH=. python tests/conv_path_cases.py | /tmp/conv_path_sweep
//
// Queries come in on stdin, one per line, `desc` being the 17 int32 fields of acg_conv_desc in order:
//   path  <name> <which> <dtype> <as_pair_a> <desc>      -> acg_conv2d_path
//   pair  <name> <transposed> <dtype> <flags> <desc>     -> acg_conv2d_pair_path
//   epi   <name> <dtype> <desc>                          -> acg_deconv2d_fwd_bias_act_ok
//   stats <name> <which> <dtype> <groups> <desc>         -> acg_conv2d_stats_blocks
// tests/conv_path_cases.py prints its table in this form; tests/test_conv_paths_cpu.py holds the answers against the table's
// expectations, so the table can be composed and re-derived on a machine with no GPU.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../action_conditioned_gans_amd/csrc/conv_bf16_kernel.h"

namespace acgconv {      // defined below; declared before conv_f32.hip names them
template <> int launch_mode<MODE_FWD>(const Plan&, const ConvArgs&, hipStream_t);
template <> int launch_mode<MODE_DGRAD>(const Plan&, const ConvArgs&, hipStream_t);
template <> int launch_mode<MODE_WGRAD>(const Plan&, const ConvArgs&, hipStream_t);
template <> int launch_mode16<MODE_FWD>(const Plan&, const ConvArgs&, hipStream_t);
template <> int launch_mode16<MODE_DGRAD>(const Plan&, const ConvArgs&, hipStream_t);
template <> int launch_mode16<MODE_WGRAD>(const Plan&, const ConvArgs&, hipStream_t);
}  // namespace acgconv

#include "../action_conditioned_gans_amd/csrc/conv_f32.hip"

namespace acg {      // what elementwise.hip provides inside the library
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  return code;
}
int check_launch(const char*) { return ACG_OK; }
}  // namespace acg

namespace acgconv {      // the launch functions of the other conv sources: never reached from the queries
int launch_direct(int, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
int launch_direct_pair(const ConvArgs&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
int launch_pair(int, const Plan&, const ConvArgs&, const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
int launch_pair16(int, const Plan&, const ConvArgs&, const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
int launch_deconv_fwd_epi(const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
int launch_deconv_fwd_epi16(const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
template <> int launch_mode<MODE_FWD>(const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
template <> int launch_mode<MODE_DGRAD>(const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
template <> int launch_mode<MODE_WGRAD>(const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
template <> int launch_mode16<MODE_FWD>(const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
template <> int launch_mode16<MODE_DGRAD>(const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
template <> int launch_mode16<MODE_WGRAD>(const Plan&, const ConvArgs&, hipStream_t) { return ACG_ERR_LAUNCH; }
}  // namespace acgconv

static bool read_desc(char** tok, acg_conv_desc* d) {
  int32_t* f = &d->batch;
  for (int i = 0; i < 17; ++i) {
    if (tok[i] == nullptr) return false;
    f[i] = atoi(tok[i]);
  }
  return true;
}

int main() {
  static_assert(sizeof(acg_conv_desc) == 17 * sizeof(int32_t), "acg_conv_desc: 17 int32 fields");
  static const char* const fam[] = {"direct", "mfma_f32", "mfma_bf16", "glds_bf16"}, * const red[] = {"none", "plain", "bf16", "cols"};
  static const char* const pairs[] = {"refused", "direct_pair", "conv_pair_f32", "conv_pair_bf16", "two_launches", "merged"};
  static const char* const which[] = {"fwd", "dgrad", "wgrad"};
  char line[1024];
  int bad = 0;
  while (fgets(line, sizeof line, stdin)) {
    char* tok[32] = {};
    int n = 0;
    for (char* t = strtok(line, " \t\r\n"); t != nullptr && n < 31; t = strtok(nullptr, " \t\r\n")) tok[n++] = t;
    if (n == 0 || tok[0][0] == '#') continue;
    acg_conv_desc d{};
    if (!strcmp(tok[0], "path") && n == 5 + 17 && read_desc(tok + 5, &d)) {
      acg_conv_path p{};
      const int w = atoi(tok[2]);
      const int rc = acg_conv2d_path(&d, w, atoi(tok[3]), atoi(tok[4]), &p);
      if (rc != ACG_OK) { printf("path %s %s error=%d\n", tok[1], w >= 0 && w <= 2 ? which[w] : "?", rc); continue; }
      printf("path %s %s family=%s tile=%dx%d tiles=%d classes=%d nk=%d splits=%d ragged=%d nvec=%d lin=%d compact=%d merged=%d reduce=%s nb=%d uk=%d uw=%d\n",
             tok[1], which[w], fam[p.family], p.tile_rows, p.tile_cols, p.tiles, p.classes, p.nk, p.splits, p.ragged, p.nvec, p.lin, p.compact,
             p.merged, red[p.reduce], p.direct_nb, p.uniform_k, p.uniform_w);
    } else if (!strcmp(tok[0], "pair") && n == 5 + 17 && read_desc(tok + 5, &d)) {
      printf("pair %s flags=%d kind=%s\n", tok[1], atoi(tok[4]), pairs[acg_conv2d_pair_path(&d, atoi(tok[2]), atoi(tok[3]), atoi(tok[4]))]);
    } else if (!strcmp(tok[0], "epi") && n == 3 + 17 && read_desc(tok + 3, &d)) {
      printf("epi %s ok=%d\n", tok[1], acg_deconv2d_fwd_bias_act_ok(&d, atoi(tok[2])));
    } else if (!strcmp(tok[0], "stats") && n == 5 + 17 && read_desc(tok + 5, &d)) {
      printf("stats %s groups=%d blocks=%d\n", tok[1], atoi(tok[4]), acg_conv2d_stats_blocks(&d, atoi(tok[2]), atoi(tok[3]), atoi(tok[4])));
    } else {
      fprintf(stderr, "conv_path_sweep: cannot read the query '%s' (%d fields)\n", tok[0], n);
      ++bad;
    }
  }
  return bad ? 1 : 0;
}
