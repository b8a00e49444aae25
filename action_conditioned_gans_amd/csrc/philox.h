// Philox4x32-10, the uniform and the normals it is turned into, and the counter protocol of the device-side draws of
// include/acgan_rollout.h: the generator's noise input (noise.hip), the scheduled-sampling coins (sched_sample.hip) and the planner's
// candidates (plan.hip).  Each is ONE block that draws from a {seed, counter} pair in device memory with the counter words
// (lo32(counter), hi32(counter), block, stream word) and the key (lo32(seed), hi32(seed)): every thread reads the pair
// (load_draw_state), thread i takes the Philox blocks i, i + blockDim.x, ... (draw_block; the tail of the last block is dropped by
// the kernel's own element loop), and advance_draw_state closes the launch.  No atomics: a draw is a pure function of
// (seed, counter, stream word, element index).  The instance noise on the discriminator's inputs (d_noise.hip) is the one
// multi-block draw: its blocks call draw_block on a {seed, counter} SNAPSHOT that a one-thread launch took and advanced before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acg {

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key (k0, k1) -> c[4]
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += W0;
    k1 += W1;
  }
}

// the top 23 bits of x, centred in their cell: exact in float32, inside (0, 1)
__device__ __forceinline__ float unit(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

struct DrawState {
  unsigned long long seed, counter;
};

__device__ __forceinline__ DrawState load_draw_state(const unsigned long long* __restrict__ state) { return {state[0], state[1]}; }

// c[4] = Philox block `block` of the draw that `s` and the stream word name
__device__ __forceinline__ void draw_block(const DrawState& s, uint32_t block, uint32_t stream_word, uint32_t (&c)[4]) {
  c[0] = (uint32_t)s.counter;
  c[1] = (uint32_t)(s.counter >> 32);
  c[2] = block;
  c[3] = stream_word;
  philox4x32_10(c, (uint32_t)s.seed, (uint32_t)(s.seed >> 32));
}

// z[4] ~ N(0, 1): the four words of a Philox block by Box-Muller, two pairs
__device__ __forceinline__ void normals(const uint32_t (&c)[4], float (&z)[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float r = sqrtf(-2.f * logf(unit(c[2 * h]))), t = 6.283185307179586f * unit(c[2 * h + 1]);
    z[2 * h] = r * cosf(t);
    z[2 * h + 1] = r * sinf(t);
  }
}

// the end of a draw kernel: a barrier - every thread has read the counter - and thread 0 stores counter + 1
__device__ __forceinline__ void advance_draw_state(unsigned long long* __restrict__ state, const DrawState& s) {
  __syncthreads();
  if (threadIdx.x == 0) state[1] = s.counter + 1;
}

}  // namespace acg
