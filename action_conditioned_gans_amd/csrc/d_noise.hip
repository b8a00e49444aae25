// Instance noise on the discriminator's inputs (include/acgan_rollout.h: acg_inst_noise_prepare / acg_inst_noise_add) and the
// statistics of its logits (acg_logit_stats).
//
// Prepare / add.  The draws of noise.hip, sched_sample.hip and plan.hip are ONE block each, so the block that draws can also
// advance the counter behind a barrier.  This draw covers every pixel D judges (2 B S S at config 2: 262 144 Philox blocks), a
// multi-block launch, and no block of such a launch may advance a counter the others still have to read.  So the counter
// protocol is a launch of its own: acg_inst_noise_prepare - one thread - evaluates sigma at the schedule position it finds,
// copies {seed, counter} into a key snapshot and advances both; acg_inst_noise_add only READS that snapshot and sigma, so it is
// a pure function of its inputs: no atomics, no workspace, the same bits on every run.
//
// Add: one thread per pixel, grid-strided.  The pixel index is the Philox block, the judged frame's channels are its lanes (at
// most 4), so a thread runs Philox once and Box-Muller twice for the up to 32 bytes it moves: 8.4 MB in and 8.4 MB out at
// config 2, HBM-bound.  A pixel moves as 16-byte vectors where pitch * element size is a multiple of 16 and both bases are
// aligned (pitch 8: two per float32 pixel, one per bf16 pixel; consecutive lanes then cover consecutive 32 / 16 bytes), and
// element by element otherwise - the same bits either way.  Untouched channels and the pad channels are moved as bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/acgan_rollout.h"
#include "common.h"
#include "philox.h"

namespace {

constexpr int NTH = 256;
constexpr int MAX_BLOCKS = 2048;      // 256 CUs x 8 blocks: longer tensors loop

// sigma at schedule position k, in double with every operation rounded on its own (the float64 restatement of the tests rounds
// each one too)
__device__ __forceinline__ double sigma_at(unsigned long long k, float start, float final, long long offset, long long decay_steps) {
#pragma clang fp contract(off)
  const double s = (double)start, f = (double)final;
  if (decay_steps == 0) return s;
  const unsigned long long off = (unsigned long long)offset;
  const double j = (double)(k > off ? k - off : 0ull);
  const double t = fmin(j / (double)decay_steps, 1.0);
  return s + (f - s) * t;
}

__global__ __launch_bounds__(64) void inst_noise_prepare_kernel(unsigned long long* __restrict__ state,
                                                                unsigned long long* __restrict__ updates,
                                                                unsigned long long* __restrict__ key_out, float* __restrict__ sigma_out,
                                                                float start, float final, long long offset, long long decay_steps,
                                                                int advance_schedule) {
  if (threadIdx.x != 0) return;       // ordinary stores of one thread: nobody else reads or writes these words in this launch
  const unsigned long long seed = state[0], counter = state[1], k = updates[0];
  sigma_out[0] = (float)sigma_at(k, start, final, offset, decay_steps);
  key_out[0] = seed;
  key_out[1] = counter;
  state[1] = counter + 1;
  if (advance_schedule) updates[0] = k + 1;
}

// lane l (0..3) of z without a runtime-indexed register array
__device__ __forceinline__ float pick(const float (&z)[4], int l) { return l == 0 ? z[0] : l == 1 ? z[1] : l == 2 ? z[2] : z[3]; }

__device__ __forceinline__ uint32_t noisy_bits(uint32_t bits, float sg, float z, float*) { return __float_as_uint(fmaf(sg, z, __uint_as_float(bits))); }
__device__ __forceinline__ uint16_t noisy_bits(uint16_t bits, float sg, float z, __bf16*) {
  const __bf16 r = (__bf16)fmaf(sg, z, __uint_as_float((uint32_t)bits << 16));      // round to nearest even, once
  return __builtin_bit_cast(uint16_t, r);
}

// T: the storage type, U: its bits.  VEC: the pixel moves as 16-byte vectors.
template <typename T, typename U, bool VEC>
__global__ __launch_bounds__(NTH) void inst_noise_add_kernel(const U* __restrict__ in, U* __restrict__ out,
                                                             const unsigned long long* __restrict__ key, const float* __restrict__ sigma,
                                                             long long pixels, int pitch, int c0, int cn, uint32_t stream_word) {
  constexpr int EPV = 16 / (int)sizeof(U);      // elements per 16-byte vector
  const acg::DrawState draw = {key[0], key[1]};
  const float sg = sigma[0];
  const bool quiet = sg == 0.f;                 // uniform: a bitwise copy of every channel (-0.0 stays -0.0)
  for (long long p = (long long)blockIdx.x * NTH + threadIdx.x; p < pixels; p += (long long)gridDim.x * NTH) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!quiet) {
      uint32_t c[4];
      acg::draw_block(draw, (uint32_t)p, stream_word, c);
      acg::normals(c, z);
    }
    const long long base = p * pitch;
    if (VEC) {
      const uint4* __restrict__ src = reinterpret_cast<const uint4*>(in + base);
      uint4* __restrict__ dst = reinterpret_cast<uint4*>(out + base);
      const int nvec = pitch / EPV;
      for (int v = 0; v < nvec; ++v) {
        uint4 w = src[v];
        const int ch0 = v * EPV;
        if (!quiet && ch0 < c0 + cn && ch0 + EPV > c0) {
          uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int e = 0; e < EPV; ++e) {
            const int l = ch0 + e - c0;
            if (l >= 0 && l < cn) {
              if constexpr (sizeof(U) == 4) {
                words[e] = noisy_bits(words[e], sg, pick(z, l), (T*)nullptr);
              } else {
                const int sh = (e & 1) * 16;
                const uint16_t r = noisy_bits((uint16_t)(words[e >> 1] >> sh), sg, pick(z, l), (T*)nullptr);
                words[e >> 1] = (words[e >> 1] & ~(0xFFFFu << sh)) | ((uint32_t)r << sh);
              }
            }
          }
          w = make_uint4(words[0], words[1], words[2], words[3]);
        }
        dst[v] = w;
      }
    } else {
      for (int ch = 0; ch < pitch; ++ch) {
        U bits = in[base + ch];
        const int l = ch - c0;
        if (!quiet && l >= 0 && l < cn) bits = noisy_bits(bits, sg, pick(z, l), (T*)nullptr);
        out[base + ch] = bits;
      }
    }
  }
}

template <typename T, typename U>
void launch_add(const void* in, void* out, const uint64_t* key, const float* sigma, int64_t pixels, int pitch, int c0, int cn,
                uint32_t stream_word, hipStream_t stream) {
  const bool vec = ((int64_t)pitch * (int64_t)sizeof(U)) % 16 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int64_t nb = acg::ceil_div(pixels, NTH);
  const dim3 grid((unsigned)(nb < MAX_BLOCKS ? nb : MAX_BLOCKS));
  if (vec)
    ACG_LAUNCH((inst_noise_add_kernel<T, U, true>), grid, dim3(NTH), 0, stream, (const U*)in, (U*)out, (const unsigned long long*)key, sigma,
               (long long)pixels, pitch, c0, cn, stream_word);
  else
    ACG_LAUNCH((inst_noise_add_kernel<T, U, false>), grid, dim3(NTH), 0, stream, (const U*)in, (U*)out, (const unsigned long long*)key, sigma,
               (long long)pixels, pitch, c0, cn, stream_word);
}

// out4 = {mean fake, mean real, share of fake < 0, share of real > 0}: per-thread double partials over a strided share, the
// lanes of a wave by shuffles, the waves in order - a fixed order, no atomics
__global__ __launch_bounds__(NTH) void logit_stats_kernel(const float* __restrict__ fake, const float* __restrict__ real, int n,
                                                          float* __restrict__ out4) {
  __shared__ double scratch[16];
  double sf = 0.0, sr = 0.0, nf = 0.0, nr = 0.0;
  for (int i = threadIdx.x; i < n; i += NTH) {
    const float f = fake[i], r = real[i];
    sf += (double)f;
    sr += (double)r;
    nf += f < 0.f ? 1.0 : 0.0;
    nr += r > 0.f ? 1.0 : 0.0;
  }
  sf = acg::block_sum(sf, scratch);
  sr = acg::block_sum(sr, scratch);
  nf = acg::block_sum(nf, scratch);
  nr = acg::block_sum(nr, scratch);
  if (threadIdx.x == 0) {
    const double d = (double)n;
    out4[0] = (float)(sf / d);
    out4[1] = (float)(sr / d);
    out4[2] = (float)(nf / d);
    out4[3] = (float)(nr / d);
  }
}

}  // namespace

extern "C" {

int32_t acg_inst_noise_prepare(uint64_t* state, uint64_t* updates, uint64_t* key_out, float* sigma_out, float sigma_start,
                               float sigma_final, int64_t offset, int64_t decay_steps, int32_t advance_schedule, acg_stream_t stream) {
  ACG_REQUIRE(state && updates && key_out && sigma_out, ACG_ERR_INVALID_ARG, "inst_noise_prepare: null pointer");
  ACG_REQUIRE(isfinite(sigma_start) && sigma_start >= 0.f && isfinite(sigma_final) && sigma_final >= 0.f, ACG_ERR_INVALID_ARG,
              "inst_noise_prepare: sigma_start %g / sigma_final %g must be finite and >= 0", (double)sigma_start, (double)sigma_final);
  ACG_REQUIRE(offset >= 0, ACG_ERR_INVALID_ARG, "inst_noise_prepare: offset %lld", (long long)offset);
  ACG_REQUIRE(decay_steps >= 0, ACG_ERR_INVALID_ARG, "inst_noise_prepare: decay_steps %lld", (long long)decay_steps);
  ACG_LAUNCH(inst_noise_prepare_kernel, dim3(1), dim3(64), 0, acg::to_stream(stream), (unsigned long long*)state,
             (unsigned long long*)updates, (unsigned long long*)key_out, sigma_out, sigma_start, sigma_final, (long long)offset,
             (long long)decay_steps, (int)advance_schedule);
  return acg::check_launch("inst_noise_prepare");
}

int32_t acg_inst_noise_add(const void* in, void* out, const uint64_t* key, const float* sigma, int64_t pixels, int32_t c, int32_t pitch,
                           int32_t c0, int32_t cn, int32_t dtype, int32_t stream_id, acg_stream_t stream) {
  ACG_REQUIRE(in && out && key && sigma, ACG_ERR_INVALID_ARG, "inst_noise_add: null pointer");
  ACG_REQUIRE(in != out, ACG_ERR_INVALID_ARG, "inst_noise_add: in and out are the same buffer (the add is not in place)");
  ACG_REQUIRE(dtype == ACG_F32 || dtype == ACG_BF16, ACG_ERR_UNSUPPORTED, "inst_noise_add: dtype %d (ACG_F32 or ACG_BF16)", dtype);
  ACG_REQUIRE(pixels >= 1, ACG_ERR_INVALID_ARG, "inst_noise_add: pixels %lld", (long long)pixels);
  ACG_REQUIRE(pixels < (int64_t)1 << 32, ACG_ERR_UNSUPPORTED, "inst_noise_add: %lld pixels, the Philox block index holds fewer than 2^32",
              (long long)pixels);
  ACG_REQUIRE(c >= 1 && c <= pitch, ACG_ERR_INVALID_ARG, "inst_noise_add: %d channels at a pitch of %d", c, pitch);
  ACG_REQUIRE(cn >= 1 && c0 >= 0, ACG_ERR_INVALID_ARG, "inst_noise_add: channels [%d, %d + %d)", c0, c0, cn);
  ACG_REQUIRE(cn <= 4, ACG_ERR_UNSUPPORTED, "inst_noise_add: %d noisy channels, a Philox block has 4 lanes", cn);
  ACG_REQUIRE((int64_t)c0 + cn <= c, ACG_ERR_INVALID_ARG, "inst_noise_add: channels [%d, %d + %d) of %d", c0, c0, cn, c);
  const uint32_t word = (uint32_t)stream_id ^ ACG_DN_STREAM_TAG;
  if (dtype == ACG_F32)
    launch_add<float, uint32_t>(in, out, key, sigma, pixels, pitch, c0, cn, word, acg::to_stream(stream));
  else
    launch_add<__bf16, uint16_t>(in, out, key, sigma, pixels, pitch, c0, cn, word, acg::to_stream(stream));
  return acg::check_launch("inst_noise_add");
}

int32_t acg_logit_stats(const float* fake, const float* real, int32_t n, float* out4, acg_stream_t stream) {
  ACG_REQUIRE(fake && real && out4, ACG_ERR_INVALID_ARG, "logit_stats: null pointer");
  ACG_REQUIRE(n >= 1, ACG_ERR_INVALID_ARG, "logit_stats: n %d", n);
  ACG_LAUNCH(logit_stats_kernel, dim3(1), dim3(NTH), 0, acg::to_stream(stream), fake, real, (int)n, out4);
  return acg::check_launch("logit_stats");
}

}  // extern "C"
