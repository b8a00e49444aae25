// Host stand-in for <hip/hip_runtime.h>: runs a kernel's blocks one after another, the threads of a block as real threads
// that meet at a barrier for __syncthreads().  Only what csrc/ssim_loss.hip, csrc/ssim_window.h, csrc/grad_norm.hip,
// csrc/conv_tile.h and csrc/common.h use.
#pragma once
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
#define __align__(n) __attribute__((aligned(n)))

struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct float4 { float x, y, z, w; } __attribute__((aligned(16)));
static inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
typedef void* hipStream_t;
typedef int hipError_t;
static inline hipError_t hipGetLastError() { return 0; }

extern thread_local dim3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;
extern pthread_barrier_t emu_barrier;
extern double emu_exchange[1024];
static inline void __syncthreads() { pthread_barrier_wait(&emu_barrier); }
using std::min;
using std::max;
// (csrc/conv_tile.h: compact_taps)
static inline unsigned atomicOr(unsigned* p, unsigned v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }

// called by every thread of the block at the same place (block_sum): exchange through memory
template <typename T>
static inline T __shfl_down(T v, int off, int width) {
  emu_exchange[threadIdx.x] = (double)v;
  __syncthreads();
  const unsigned src = threadIdx.x + off;
  const T r = ((threadIdx.x & 63) + off < 64 && src < blockDim.x) ? (T)emu_exchange[src] : v;
  __syncthreads();
  return r;
}

template <typename K, typename... A>
static inline void emu_launch(K kernel, dim3 grid, dim3 block, A... args) {
  blockDim = block;
  gridDim = grid;
  for (unsigned b = 0; b < grid.x; ++b) {
    pthread_barrier_init(&emu_barrier, nullptr, block.x);
    std::vector<std::thread> ts;
    for (unsigned t = 0; t < block.x; ++t)
      ts.emplace_back([=]() { threadIdx = dim3(t); blockIdx = dim3(b); kernel(args...); });
    for (auto& t : ts) t.join();
    pthread_barrier_destroy(&emu_barrier);
  }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
