// The weight average's per-element update, its coefficient prologue and its in-launch counter advance (include/acgan_ema.h),
// shared by the stand-alone kernel (ema.hip) and the optimizer kernels that carry the update (optim.hip); the counter advance
// (retire) is also what the scheduled optimizer entries advance their update counter with (include/acgan_rollout.h).
#pragma once
#include <hip/hip_runtime.h>

namespace acg_ema {

struct Coef {
  float omd;   // (float)(1 - min(decay, (1 + k) / (10 + k)))
  int seed;    // k == 0: the shadow takes the parameter
};

// ONE thread per block: a dependent read of the counter and a double-precision division - callers issue their loads first.
__device__ __forceinline__ Coef coef(const long long* num_updates, float decay, long long* k_out) {
  const long long k = *num_updates;
  const double d = fmin((double)decay, (1.0 + (double)k) / (10.0 + (double)k));
  *k_out = k;
  return Coef{(float)(1.0 - d), k == 0 ? 1 : 0};
}

// Three separately rounded operations, no FMA: the same bits whichever kernel inlines it, and a float32 restatement on the host
// reproduces it.  The pragma over plain operators is what guarantees it: hipcc's __fmul_rn / __fsub_rn are inline functions around
// a plain `*` and `-` compiled under the default -ffp-contract=fast-honor-pragmas, and the product and the subtraction behind it
// came out as one v_fma_f32 (seen in the ISA, and as a last-bit difference from the restatement on the device).
__device__ __forceinline__ float ema1(float s, float p, float omd, int seed) {
#pragma clang fp contract(off)
  const float diff = s - p;
  const float prod = omd * diff;
  return seed ? p : s - prod;
}

// ema1 over the four elements of a 16-byte access
__device__ __forceinline__ void ema4(float4& s, const float4& p, float omd, int seed) {
  s.x = ema1(s.x, p.x, omd, seed); s.y = ema1(s.y, p.y, omd, seed);
  s.z = ema1(s.z, p.z, omd, seed); s.w = ema1(s.w, p.w, omd, seed);
}

// A device counter that the launch which read it advances: called by the ONE thread of each block that read the counter (coef()
// above for the average's num_updates; the learning-rate schedule's update counter in optim.hip), behind a block barrier that
// follows the read.  `done` is the counter's own state word: one word belongs to one counter, a launch that advances two
// counters calls this twice with two words.  The last block of the grid to get here writes the counter and resets the word;
// nobody waits on either.  Relaxed is enough: this thread's read of the counter has RETURNED (its value went through shared
// memory in front of the barrier), so it was performed before this add, and the one store to the counter comes after the add
// that saw every other block's - after every read of this launch.  The next launch (or graph node) on the stream sees counter
// and word through the kernel boundary.
__device__ __forceinline__ void retire(long long* counter, unsigned* done, long long k) {
  const unsigned total = gridDim.x * gridDim.y * gridDim.z;
  const unsigned prev = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (prev + 1u == total) {
    __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *counter = k + 1;
  }
}

}  // namespace acg_ema
