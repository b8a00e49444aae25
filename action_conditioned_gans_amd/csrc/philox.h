// Philox4x32-10 and the uniform it is turned into, shared by the device-side draws of include/acgan_rollout.h: the generator's noise
// input (noise.hip) and the scheduled-sampling coins (sched_sample.hip).  Both draw from a {seed, counter} pair in device memory
// with the counter words (lo32(counter), hi32(counter), block, stream word) and the key (lo32(seed), hi32(seed)).
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

}  // namespace acg
