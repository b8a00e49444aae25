// The generator's weight average (include/acgan_ema.h): the stand-alone update over a flat buffer and the in-place exchange of
// two flat buffers.  Pure streaming, 16 B per lane.  The optimizer kernels that carry the same update live in optim.hip,
// beside the update formulas they share; the per-element function and the counter advance are ema_common.h's.
#include <hip/hip_runtime.h>

#include "../../include/acgan_ema.h"
#include "common.h"
#include "ema_common.h"

namespace {

__global__ __launch_bounds__(256) void ema_update_k(float* __restrict__ shadow, const float* __restrict__ p, long long n,
                                                    float decay, long long* num_updates, unsigned* done) {
  __shared__ acg_ema::Coef s_c;
  const long long stride = (long long)gridDim.x * 256;
  const bool al = ((reinterpret_cast<uintptr_t>(shadow) | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
  const long long n4 = al ? n / 4 : 0;
  // the first float4 of every thread (the grid is sized so that it is nearly the only one) is loaded BEFORE the coefficient
  // prologue - a dependent read of the counter and a double-precision division on one thread - as adam_k does
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool have = i0 < n4;
  float4 ss, pp;
  auto load = [&](long long i) { ss = reinterpret_cast<float4*>(shadow)[i]; pp = reinterpret_cast<const float4*>(p)[i]; };
  if (have) load(i0);
  long long k = 0;
  if (threadIdx.x == 0) s_c = acg_ema::coef(num_updates, decay, &k);
  __syncthreads();
  const float omd = s_c.omd;
  const int seed = s_c.seed;
  auto update = [&](long long i) { acg_ema::ema4(ss, pp, omd, seed); reinterpret_cast<float4*>(shadow)[i] = ss; };
  if (have) update(i0);
  for (long long i = i0 + stride; i < n4; i += stride) { load(i); update(i); }
  for (long long i = n4 * 4 + i0; i < n; i += stride) shadow[i] = acg_ema::ema1(shadow[i], p[i], omd, seed);
  if (threadIdx.x == 0) acg_ema::retire(num_updates, done, k);
}

__global__ __launch_bounds__(256) void swap_k(float* __restrict__ a, float* __restrict__ b, long long n) {
  const long long stride = (long long)gridDim.x * 256;
  const bool al = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
  const long long n4 = al ? n / 4 : 0;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
  for (long long i = i0; i < n4; i += stride) {
    const float4 x = reinterpret_cast<float4*>(a)[i], y = reinterpret_cast<float4*>(b)[i];
    reinterpret_cast<float4*>(a)[i] = y; reinterpret_cast<float4*>(b)[i] = x;
  }
  for (long long i = n4 * 4 + i0; i < n; i += stride) {
    const float x = a[i], y = b[i];
    a[i] = y; b[i] = x;
  }
}

}  // namespace

extern "C" {

int32_t acg_ema_update(float* shadow, const float* param, int64_t n, float decay, int64_t* num_updates, uint32_t* state,
                       acg_stream_t stream) {
  ACG_REQUIRE(n > 0 && shadow && param && num_updates && state, ACG_ERR_INVALID_ARG, "ema_update: null pointer / n <= 0");
  ACG_REQUIRE(decay > 0.f && decay < 1.f, ACG_ERR_INVALID_ARG, "ema_update: decay %g is not in (0, 1)", (double)decay);
  ACG_REQUIRE((reinterpret_cast<uintptr_t>(num_updates) & 7) == 0 && (reinterpret_cast<uintptr_t>(state) & 3) == 0, ACG_ERR_INVALID_ARG,
              "ema_update: the counter must be 8-byte and the state word 4-byte aligned");
  ACG_LAUNCH(ema_update_k, dim3(acg::grid_for(n / 4 + 1)), dim3(256), 0, acg::to_stream(stream), shadow, param, (long long)n, decay,
             reinterpret_cast<long long*>(num_updates), reinterpret_cast<unsigned*>(state));
  return acg::check_launch("ema_update");
}

int32_t acg_swap_f32(float* a, float* b, int64_t n, acg_stream_t stream) {
  ACG_REQUIRE(n > 0 && a && b, ACG_ERR_INVALID_ARG, "swap_f32: null pointer / n <= 0");
  ACG_REQUIRE(a + n <= b || b + n <= a, ACG_ERR_INVALID_ARG, "swap_f32: the buffers overlap");
  ACG_LAUNCH(swap_k, dim3(acg::grid_for(n / 4 + 1)), dim3(256), 0, acg::to_stream(stream), a, b, (long long)n);
  return acg::check_launch("swap_f32");
}

}  // extern "C"
