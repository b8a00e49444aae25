// The BatchNorm path rule of bn.hip (fwd_path / bwd_path / slabs_layout) as a table, on the CPU: which kernel family, which
// grid, which NR for a sweep of shapes - no GPU, no launch.  Built with the host sanitizers it also proves the rule free of
// overflow and undefined behaviour at the sizes where the kernels change:
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/bn_path_sweep.hip -o /tmp/bn_path_sweep && /tmp/bn_path_sweep > table.txt
//
// Two builds that print the same table choose the same kernels (profiles/bn_host/README.md: the dispatcher rewrite against
// the rule it replaced).  The CU count is an argument of the rule here: BnCall::ncu.
#include <stdarg.h>
#include <stdio.h>

#ifndef BN_SWEEP_SOURCE      // -DBN_SWEEP_SOURCE='"file"': another source of BnCall / fwd_path / bwd_path / slabs_layout / slabs_family,
#define BN_SWEEP_SOURCE "../action_conditioned_gans_amd/csrc/bn.hip"      // e.g. an older rule written out for comparison
#endif
#include BN_SWEEP_SOURCE

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

static void show(const char* dir, const BnPath& p) {
  static const char* const names[] = {"none", "resident", "grid", "two_launch"};
  printf(" %s=%s", dir, names[p.family]);
  if (p.family == kResident) printf(":nr%d", p.nr);
  if (p.family == kGrid) printf(":%dx%d:%ux%ux%u", p.f.nt, p.f.U, p.f.grid.x, p.f.grid.y, p.f.grid.z);
}

int main() {
  const long long rows[] = {1, 255, 256, 257, 2047, 2048, 2049, 65537, 262145};
  const int chans[] = {4, 7, 8, 40, 1024}, ncus[] = {0, 256, 304};
  static const float probe = 0.f;
  for (int ncu : ncus)
    for (long long R : rows)
      for (int C : chans)
        for (int groups = 1; groups <= 3; ++groups)
          for (int no_grid = 0; no_grid < 2; ++no_grid) {
            for (int slabs = 0; slabs < 3; ++slabs) {      // none, rows, quads
              BnCall c{};
              c.R = R; c.C = C; c.groups = groups; c.v4 = C % 4 == 0; c.no_grid = no_grid != 0; c.ncu = ncu;
              c.sl = slabs ? Slabs{&probe, 2, R * groups * C, slabs == 2 ? R * groups : 0} : Slabs{nullptr, 0, 0, 0};
              printf("ncu=%d R=%lld C=%d groups=%d no_grid=%d slabs=%s", ncu, R, C, groups, no_grid, slabs == 0 ? "none" : slabs == 1 ? "rows" : "quads");
              show("fwd", fwd_path(c));
              show("bwd", bwd_path(c));
              printf("\n");
            }
            printf("ncu=%d R=%lld C=%d groups=%d no_grid=%d layout fwd=%d bwd=%d slabs_ok=%d\n", ncu, R, C, groups, no_grid,
                   slabs_layout(R, C, groups, C % 4 == 0, no_grid != 0, false, ncu), slabs_layout(R, C, groups, C % 4 == 0, no_grid != 0, true, ncu),
                   slabs_family(R, 4, groups, false, true, true, true, ncu) == kResident);
          }
  return 0;
}
