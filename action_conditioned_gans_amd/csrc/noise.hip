// The generator's noise input (include/acgan_rollout.h, acg_noise_concat): out[b] = [actions[b], scale * z[b]] with z drawn
// on the device by Philox4x32-10 + Box-Muller from a {seed, counter} pair in device memory that the kernel itself advances - a
// captured program draws a fresh z at every replay with no host in the loop.
//
// One block: at most 8192 normals (2048 Philox blocks, 8 per thread) and 8192 * 64 copied action values - the call is launch-latency
// bound like the one-block loss heads of loss.hip, and one block needs no handshake for the counter: every thread reads it, a
// barrier, thread 0 stores counter + 1.  No atomics; the draw is a pure function of (seed, counter, stream_id, element index).
#include <hip/hip_runtime.h>
#include "../../include/acgan_rollout.h"
#include "common.h"
#include "philox.h"

namespace {

constexpr int NTH = 256;

__global__ __launch_bounds__(NTH) void noise_concat_kernel(const float* __restrict__ actions, unsigned long long* __restrict__ state,
                                                           const float* __restrict__ scale, float* __restrict__ out, int B, int A, int Z,
                                                           uint32_t stream_id) {
  const int tid = threadIdx.x, P = A + Z, n = B * Z;
  const acg::DrawState draw = acg::load_draw_state(state);
  const float sc = scale[0];
  for (int idx = tid; idx < B * A; idx += NTH) {
    const int b = idx / A;
    out[b * P + idx - b * A] = actions[idx];
  }
  for (int i = tid; i * 4 < n; i += NTH) {
    uint32_t c[4];
    float z[4];
    acg::draw_block(draw, (uint32_t)i, stream_id, c);
    acg::normals(c, z);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int e = i * 4 + l;                 // the tail of the last Philox block is dropped
      if (e < n) {
        const int b = e / Z;
        out[b * P + A + e - b * Z] = sc == 0.f ? 0.f : sc * z[l];
      }
    }
  }
  acg::advance_draw_state(state, draw);
}

}  // namespace

extern "C" int32_t acg_noise_concat(const float* actions, uint64_t* state, const float* scale, float* out, int32_t batch,
                                    int32_t action_dim, int32_t noise_dim, int32_t stream_id, acg_stream_t stream) {
  ACG_REQUIRE(actions && state && scale && out, ACG_ERR_INVALID_ARG, "noise_concat: null pointer");
  ACG_REQUIRE(batch >= 1, ACG_ERR_INVALID_ARG, "noise_concat: batch %d", batch);
  ACG_REQUIRE(action_dim >= 1 && action_dim <= ACG_NOISE_DIM_MAX, ACG_ERR_INVALID_ARG, "noise_concat: action_dim %d outside 1..%d",
              action_dim, ACG_NOISE_DIM_MAX);
  ACG_REQUIRE(noise_dim >= 1 && noise_dim <= ACG_NOISE_DIM_MAX, ACG_ERR_INVALID_ARG, "noise_concat: noise_dim %d outside 1..%d",
              noise_dim, ACG_NOISE_DIM_MAX);
  ACG_REQUIRE((int64_t)batch * noise_dim <= ACG_NOISE_VALUES_MAX, ACG_ERR_UNSUPPORTED, "noise_concat: %d x %d values, at most %d", batch,
              noise_dim, ACG_NOISE_VALUES_MAX);
  ACG_LAUNCH(noise_concat_kernel, dim3(1), dim3(NTH), 0, acg::to_stream(stream), actions, (unsigned long long*)state, scale, out,
             (int)batch, (int)action_dim, (int)noise_dim, (uint32_t)stream_id);
  return acg::check_launch("noise_concat");
}
