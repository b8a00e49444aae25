// The learned latent posterior of the generator's noise input (include/acgan_rollout.h): acg_latent_fwd is noise.hip's draw with
// the reparameterisation z = mu + scale * exp(logvar / 2) * eps and the KL term in the same launch, acg_latent_bwd the one launch
// that carries the generator's gradient and the KL gradient back into (mu, logvar).
//
// One block each, the limits of acg_noise_concat: at most 8192 latent values, so both calls are launch-latency bound and the KL
// sum - double terms, a fixed order - needs no workspace and no atomics.  The counter protocol is philox.h's.
#include <hip/hip_runtime.h>
#include "../../include/acgan_rollout.h"
#include "common.h"
#include "philox.h"

namespace {

constexpr int NTH = 256;

__global__ __launch_bounds__(NTH) void latent_fwd_kernel(const float* __restrict__ actions, const float* __restrict__ stats,
                                                         unsigned long long* __restrict__ state, const float* __restrict__ mode,
                                                         float* __restrict__ out, float* __restrict__ kl, int B, int A, int Z,
                                                         uint32_t stream_id) {
  __shared__ double scratch[16];
  const int tid = threadIdx.x, P = A + Z, n = B * Z;
  const acg::DrawState draw = acg::load_draw_state(state);
  const float sc = mode[0];
  const bool posterior = mode[1] != 0.f;
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
        const int b = e / Z, j = e - b * Z;
        float v;
        if (posterior) {
          const float mu = stats[b * 2 * Z + j], lv = stats[b * 2 * Z + Z + j];
          v = sc == 0.f ? mu : fmaf(sc * expf(0.5f * lv), z[l], mu);
        } else {
          v = sc == 0.f ? 0.f : sc * z[l];
        }
        out[b * P + A + j] = v;
      }
    }
  }
  if (kl != nullptr) {                         // (a kernel argument: the whole block takes the branch, the barriers inside are uniform)
    double part = 0.0;
    for (int e = tid; e < n; e += NTH) {
      const int b = e / Z, j = e - b * Z;
      const double mu = (double)stats[b * 2 * Z + j], lv = (double)stats[b * 2 * Z + Z + j];
      part += mu * mu + exp(lv) - lv - 1.0;
    }
    const double total = acg::block_sum(part, scratch);
    if (tid == 0) kl[0] = (float)(0.5 * total);
  }
  acg::advance_draw_state(state, draw);
}

__global__ __launch_bounds__(NTH) void latent_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                         const float* __restrict__ stats, const float* __restrict__ mode, float klw,
                                                         float* __restrict__ dstats, float* __restrict__ dactions, int B, int A, int Z) {
  const int tid = threadIdx.x, P = A + Z, n = B * Z;
  const bool posterior = mode[1] != 0.f;
  for (int e = tid; e < n; e += NTH) {
    const int b = e / Z, j = e - b * Z;
    const float mu = stats[b * 2 * Z + j], lv = stats[b * 2 * Z + Z + j];
    float gm = 0.f, gl = 0.f;
    if (posterior && dout != nullptr) {
      const float dz = dout[b * P + A + j];
      gm = dz;
      gl = 0.5f * (out[b * P + A + j] - mu) * dz;
    }
    if (klw != 0.f) {
      gm = fmaf(klw, mu, gm);
      gl = fmaf(0.5f * klw, expm1f(lv), gl);
    }
    dstats[b * 2 * Z + j] = gm;
    dstats[b * 2 * Z + Z + j] = gl;
  }
  if (dactions != nullptr)
    for (int idx = tid; idx < B * A; idx += NTH) {
      const int b = idx / A;
      dactions[idx] = dout != nullptr ? dout[b * P + idx - b * A] : 0.f;
    }
}

}  // namespace

#define ACG_LATENT_DIMS(who)                                                                                                          \
  ACG_REQUIRE(batch >= 1, ACG_ERR_INVALID_ARG, who ": batch %d", batch);                                                              \
  ACG_REQUIRE(action_dim >= 1 && action_dim <= ACG_NOISE_DIM_MAX, ACG_ERR_INVALID_ARG, who ": action_dim %d outside 1..%d", action_dim, \
              ACG_NOISE_DIM_MAX);                                                                                                     \
  ACG_REQUIRE(latent_dim >= 1 && latent_dim <= ACG_NOISE_DIM_MAX, ACG_ERR_INVALID_ARG, who ": latent_dim %d outside 1..%d", latent_dim, \
              ACG_NOISE_DIM_MAX);                                                                                                     \
  ACG_REQUIRE((int64_t)batch * latent_dim <= ACG_NOISE_VALUES_MAX, ACG_ERR_UNSUPPORTED, who ": %d x %d values, at most %d", batch,      \
              latent_dim, ACG_NOISE_VALUES_MAX)

extern "C" int32_t acg_latent_fwd(const float* actions, const float* stats, uint64_t* state, const float* mode, float* out, float* kl,
                                  int32_t batch, int32_t action_dim, int32_t latent_dim, int32_t stream_id, acg_stream_t stream) {
  ACG_REQUIRE(actions && stats && state && mode && out, ACG_ERR_INVALID_ARG, "latent_fwd: null pointer");
  ACG_LATENT_DIMS("latent_fwd");
  ACG_LAUNCH(latent_fwd_kernel, dim3(1), dim3(NTH), 0, acg::to_stream(stream), actions, stats, (unsigned long long*)state, mode, out, kl,
             (int)batch, (int)action_dim, (int)latent_dim, (uint32_t)stream_id);
  return acg::check_launch("latent_fwd");
}

extern "C" int32_t acg_latent_bwd(const float* dout, const float* out, const float* stats, const float* mode, float kl_weight,
                                  float* dstats, float* dactions, int32_t batch, int32_t action_dim, int32_t latent_dim,
                                  acg_stream_t stream) {
  ACG_REQUIRE(out && stats && mode && dstats, ACG_ERR_INVALID_ARG, "latent_bwd: null pointer");
  ACG_LATENT_DIMS("latent_bwd");
  ACG_LAUNCH(latent_bwd_kernel, dim3(1), dim3(NTH), 0, acg::to_stream(stream), dout, out, stats, mode, kl_weight, dstats, dactions,
             (int)batch, (int)action_dim, (int)latent_dim);
  return acg::check_launch("latent_bwd");
}
