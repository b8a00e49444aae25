// acg_grad_clip_norm of csrc/grad_norm.hip - the kernel source itself, not a restatement - compiled as plain C++ for the host
// against tools/micro/hip_host/hip/hip_runtime.h: blocks run one after another, the threads of a block as real threads meeting
// at a barrier.  Built with the host sanitizers (the line below: host code only, nothing for a GPU) it checks every access to
// the gradient buffer, stats and the workspace for bounds - exact-size heap blocks - which no GPU run does
// (tests/test_clip_norm_host.py):
//   hipcc -x c++ -std=c++17 -O1 -Xarch_host -fsanitize=address,undefined -Itools/micro/hip_host -pthread tools/micro/grad_norm_host.cpp -o grad_norm_host
//   grad_norm_host in.bin out.bin pre_scale max_norm off0 len0 [off1 len1 ...]
//       in: the float32 buffer (its size is n);  out: the buffer after the call, then stats [2 + count];  max_norm "inf" measures
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
pthread_barrier_t emu_barrier;
double emu_exchange[1024];
#include "../../action_conditioned_gans_amd/csrc/grad_norm.hip"
namespace acg {
int fail(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); return code; }
int check_launch(const char*) { return 0; }
}
int main(int argc, char** argv) {
  if (argc < 7 || (argc - 5) % 2 != 0) return 1;
  acg_norm_segments segs;
  memset(&segs, 0, sizeof segs);
  const int count = (argc - 5) / 2;
  segs.count = count;
  for (int i = 0; i < count && i < ACG_NORM_SEGMENTS_MAX; ++i) {
    segs.offset[i] = atoll(argv[5 + 2 * i]);
    segs.length[i] = atoll(argv[6 + 2 * i]);
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / 4;
  fseek(f, 0, SEEK_SET);
  // exact-size heap buffers: AddressSanitizer sees any access outside them
  float* grad = (float*)aligned_alloc(16, (n * 4 + 15) / 16 * 16);
  if (fread(grad, 4, n, f) != n) return 2;
  fclose(f);
  const size_t nb = acg_grad_clip_norm_workspace_bytes((int64_t)n, &segs);
  void* ws = aligned_alloc(16, (nb + 15) / 16 * 16 + 16);
  memset(ws, 0xA5, nb);
  float* stats = (float*)malloc((2 + count) * 4);
  for (int i = 0; i < 2 + count; ++i) stats[i] = NAN;
  const int rc = acg_grad_clip_norm(grad, (int64_t)n, &segs, (float)atof(argv[3]), (float)atof(argv[4]), stats, ws, nb, nullptr);
  if (rc) return 10 + rc;
  f = fopen(argv[2], "wb");
  fwrite(grad, 4, n, f);
  fwrite(stats, 4, 2 + count, f);
  fclose(f);
  return 0;
}
