// acg_d_augment_draw / _fwd / _bwd of csrc/d_augment.hip - the kernel source itself, not a restatement - compiled as plain C++ for
// the host against tools/micro/hip_host/hip/hip_runtime.h: blocks run one after another, the threads of a block as real threads
// meeting at a barrier.  Built with the host sanitizers (the line below: host code only, nothing for a GPU) it checks every access
// to the input, the output, the parameters and the workspace for bounds - exact-size heap blocks - which no GPU run does
// (tests/test_d_augment_host.py):
//   hipcc -x c++ -std=c++17 -O1 -Xarch_host -fsanitize=address,undefined -Itools/micro/hip_host -pthread tools/micro/d_augment_host.cpp -o d_augment_host
//   d_augment_host fwd|bwd in.bin params.bin out.bin rows h w pitch frames cf off
//       in: float32 [rows, h, w, pitch];  params: float32 [rows, 8];  out: what the call left in a buffer prefilled with NaN;
//       off: 0 or 1 - both tensor bases that many floats behind a 16-byte boundary (1: the element path)
//   d_augment_host draw out.bin seed counter stream_id rows h w policy
//       out: float32 params [rows, 8], then the state's two uint64 after the call
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hip/hip_runtime.h"
struct uint4 { uint32_t x, y, z, w; } __attribute__((aligned(16)));
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
pthread_barrier_t emu_barrier;
double emu_exchange[1024];
#include "../../action_conditioned_gans_amd/csrc/d_augment.hip"
namespace acg {
int fail(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); return code; }
int check_launch(const char*) { return 0; }
}

// an exact-size heap block whose first used byte is `off` floats behind a 16-byte boundary: AddressSanitizer sees any access past
// its end (and before its start when off == 0)
static float* block(size_t floats, int off) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, (floats + off) * 4) != 0) exit(3);
  return (float*)p + off;
}

static bool read_all(const char* path, float* dst, size_t n) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const bool ok = fread(dst, 4, n, f) == n;
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc == 10 && !strcmp(argv[1], "draw")) {
    const int rows = atoi(argv[6]), h = atoi(argv[7]), w = atoi(argv[8]), policy = atoi(argv[9]);
    uint64_t* state = (uint64_t*)malloc(16);
    state[0] = strtoull(argv[3], nullptr, 10);
    state[1] = strtoull(argv[4], nullptr, 10);
    float* params = block((size_t)(rows > 0 ? rows : 1) * 8, 0);
    const int rc = acg_d_augment_draw(state, params, rows, h, w, policy, atoi(argv[5]), nullptr);
    if (rc) return 10 + rc;
    FILE* f = fopen(argv[2], "wb");
    fwrite(params, 4, (size_t)rows * 8, f);
    fwrite(state, 8, 2, f);
    fclose(f);
    return 0;
  }
  if (argc != 12) return 1;
  const bool bwd = !strcmp(argv[1], "bwd");
  const int rows = atoi(argv[5]), h = atoi(argv[6]), w = atoi(argv[7]), pitch = atoi(argv[8]), frames = atoi(argv[9]), cf = atoi(argv[10]);
  const int off = atoi(argv[11]);
  const size_t n = (size_t)rows * h * w * pitch;
  float* in = block(n, off);
  float* out = block(n, off);
  float* params = block((size_t)rows * 8, 0);
  if (!read_all(argv[2], in, n) || !read_all(argv[3], params, (size_t)rows * 8)) return 2;
  for (size_t i = 0; i < n; ++i) out[i] = NAN;
  const int64_t nb = acg_d_augment_workspace_bytes(rows, h, w, frames, cf);
  void* ws = nullptr;
  if (posix_memalign(&ws, 16, (size_t)(nb > 0 ? nb : 8)) != 0) return 3;
  memset(ws, 0xA5, (size_t)(nb > 0 ? nb : 8));
  const int rc = bwd ? acg_d_augment_bwd(in, params, out, rows, h, w, pitch, frames, cf, ws, nb, nullptr)
                     : acg_d_augment_fwd(in, params, out, rows, h, w, pitch, frames, cf, ws, nb, nullptr);
  if (rc) return 10 + rc;
  FILE* f = fopen(argv[4], "wb");
  fwrite(out, 4, n, f);
  fclose(f);
  return 0;
}
