// acg_ssim_loss of csrc/ssim_loss.hip - the kernel source itself, not a restatement - compiled as plain C++ for the host
// against tools/micro/hip_host/hip/hip_runtime.h: blocks run one after another, the threads of a block as real threads meeting
// at a barrier.  Built with the host sanitizers (the line below: host code only, nothing for a GPU) it checks every global, LDS and workspace access of a shape for
// bounds, which no GPU run does (tests/test_ssim_loss_host.py):
//   hipcc -x c++ -std=c++17 -O1 -Xarch_host -fsanitize=address,undefined -Itools/micro/hip_host -pthread tools/micro/ssim_loss_host.cpp -o ssim_loss_host
//   ssim_loss_host n h w c mode in.bin out.bin     in: pred then truth (float32); out: value (1 float) then dpred;
//                                                  mode 0: value and gradient, 1: gradient only, 2: value only
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
pthread_barrier_t emu_barrier;
double emu_exchange[1024];
#include "../../action_conditioned_gans_amd/csrc/ssim_loss.hip"
namespace acg {
int fail(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); return code; }
int check_launch(const char*) { return 0; }
}
int main(int argc, char** argv) {
  if (argc != 8) return 1;
  const int n = atoi(argv[1]), h = atoi(argv[2]), w = atoi(argv[3]), c = atoi(argv[4]), mode = atoi(argv[5]);
  const size_t numel = (size_t)n * h * w * c;
  // exact-size heap buffers: AddressSanitizer sees any access outside them
  float* pred = (float*)aligned_alloc(16, (numel * 4 + 15) / 16 * 16);
  float* truth = (float*)aligned_alloc(16, (numel * 4 + 15) / 16 * 16);
  float* dp = (float*)aligned_alloc(16, (numel * 4 + 15) / 16 * 16);
  FILE* f = fopen(argv[6], "rb");
  if (fread(pred, 4, numel, f) != numel || fread(truth, 4, numel, f) != numel) return 2;
  fclose(f);
  const size_t nb = acg_ssim_loss_workspace_bytes(n, h, w, c);
  void* ws = aligned_alloc(16, (nb + 15) / 16 * 16);
  memset(ws, 0xA5, nb);
  for (size_t i = 0; i < numel; ++i) dp[i] = NAN;
  float value = NAN;
  const int rc = acg_ssim_loss(pred, truth, mode == 1 ? nullptr : &value, mode == 2 ? nullptr : dp, 1.0f, n, h, w, c, 2.0f, 0.01f, 0.03f, ws, nb, nullptr);
  if (rc) return 10 + rc;
  f = fopen(argv[7], "wb");
  fwrite(&value, 4, 1, f);
  fwrite(dp, 4, numel, f);
  fclose(f);
  return 0;
}
