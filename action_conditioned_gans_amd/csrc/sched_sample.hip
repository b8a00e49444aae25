// Scheduled sampling for the K-step rollout trainer (include/acgan_rollout.h): the coins, the row select and its adjoint.
//
// Draw.  One block, as the noise draw (noise.hip): the coins of all K-1 fed-back positions of a program in one launch, at most
// 8192 of them (2048 Philox blocks, 8 per thread).  The probability of truth is the schedule's value at the counter the launch
// finds, evaluated in double by every thread (the same value in all of them); every thread reads the counter, a barrier, thread 0
// stores counter + 1.  No atomics: mask and probability are a pure function of (seed, counter, stream_id, schedule).
//
// Select / adjoint.  One sample per blockIdx.y, so the coin is uniform in a block and only the chosen source row is read; the
// frame rows move as 16-byte vectors where the row length and the pointers allow, the few state values ride in block x = 0 of the
// same launch.  3 MB at 64x64x3 and batch 32: launch-latency bound, so one launch per fed-back step and direction is the point.
#include <hip/hip_runtime.h>
#include "../../include/acgan_rollout.h"
#include "common.h"
#include "philox.h"

namespace {

constexpr int NTH = 256;
constexpr int VPT = 4;            // 16-byte vectors per thread and block of the select kernels
constexpr int MAX_BX = 1024;      // blocks per sample at most: longer rows loop

struct Sched {
  int kind;
  long long offset, decay_steps;
  float start, final;
};

// the schedule at update k, in double with every operation rounded on its own (no contraction: the float64 restatement of the
// tests rounds each one too)
__device__ __forceinline__ double probability(const Sched& sc, unsigned long long k) {
#pragma clang fp contract(off)
  const double s = (double)sc.start, f = (double)sc.final;
  if (sc.kind == ACG_SS_CONSTANT) return s;
  const unsigned long long off = (unsigned long long)sc.offset;
  const double j = (double)(k > off ? k - off : 0ull), d = (double)sc.decay_steps;
  if (sc.kind == ACG_SS_LINEAR) {
    const double t = fmin(j / d, 1.0);
    return s + (f - s) * t;
  }
  const double e = exp(j / d);                 // +inf for a long finished decay: d / (d + inf) = 0, p = final
  return f + (s - f) * (d / (d + e));
}

__global__ __launch_bounds__(NTH) void sched_sample_draw_kernel(unsigned long long* __restrict__ state, const Sched sc,
                                                                float* __restrict__ mask, float* __restrict__ prob_out, int n,
                                                                uint32_t stream_word) {
  const int tid = threadIdx.x;
  const acg::DrawState draw = acg::load_draw_state(state);
  const float p = (float)probability(sc, draw.counter);
  if (tid == 0) prob_out[0] = p;
  for (int i = tid; i * 4 < n; i += NTH) {
    uint32_t c[4];
    acg::draw_block(draw, (uint32_t)i, stream_word, c);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int e = i * 4 + l;                 // the tail of the last Philox block is dropped
      if (e < n) mask[e] = acg::unit(c[l]) < p ? 1.f : 0.f;
    }
  }
  acg::advance_draw_state(state, draw);
}

// dst[b, :] = src[b, :] for the rows of this block's sample, or +0 when src == nullptr.  VEC: 16-byte moves (n % 4 == 0, aligned)
template <bool VEC>
__device__ __forceinline__ void move_row(const float* __restrict__ src, float* __restrict__ dst, long long n) {
  if (VEC) {
    const long long nv = n >> 2;
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
    for (long long v0 = (long long)blockIdx.x * (NTH * VPT); v0 < nv; v0 += (long long)gridDim.x * (NTH * VPT)) {
#pragma unroll
      for (int u = 0; u < VPT; ++u) {
        const long long v = v0 + u * NTH + threadIdx.x;
        if (v < nv) d4[v] = src ? s4[v] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  } else {
    for (long long e = (long long)blockIdx.x * NTH + threadIdx.x; e < n; e += (long long)gridDim.x * NTH) dst[e] = src ? src[e] : 0.f;
  }
}

// out[b] = mask[b] != 0 ? truth[b] : pred[b]; a NULL `out` (frame or state) skips that half
template <bool VEC>
__global__ __launch_bounds__(NTH) void sched_sample_fwd_kernel(const float* __restrict__ mask, const float* __restrict__ pred,
                                                               const float* __restrict__ truth, float* __restrict__ out,
                                                               long long per_sample, const float* __restrict__ pred_state,
                                                               const float* __restrict__ true_state, float* __restrict__ out_state,
                                                               int state_dim) {
  const int b = blockIdx.y;
  const bool take_truth = mask[b] != 0.f;       // uniform in the block: only the chosen source is read
  if (out) move_row<VEC>((take_truth ? truth : pred) + (long long)b * per_sample, out + (long long)b * per_sample, per_sample);
  if (out_state && blockIdx.x == 0) {
    const float* src = (take_truth ? true_state : pred_state) + (long long)b * state_dim;
    for (int e = threadIdx.x; e < state_dim; e += NTH) out_state[(long long)b * state_dim + e] = src[e];
  }
}

// dpred[b] = mask[b] != 0 ? +0 : dout[b]
template <bool VEC>
__global__ __launch_bounds__(NTH) void sched_sample_bwd_kernel(const float* __restrict__ mask, const float* __restrict__ dout,
                                                               float* __restrict__ dpred, long long per_sample,
                                                               const float* __restrict__ dout_state, float* __restrict__ dpred_state,
                                                               int state_dim) {
  const int b = blockIdx.y;
  const bool take_truth = mask[b] != 0.f;
  if (dpred) move_row<VEC>(take_truth ? nullptr : dout + (long long)b * per_sample, dpred + (long long)b * per_sample, per_sample);
  if (dpred_state && blockIdx.x == 0) {
    for (int e = threadIdx.x; e < state_dim; e += NTH)
      dpred_state[(long long)b * state_dim + e] = take_truth ? 0.f : dout_state[(long long)b * state_dim + e];
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// blocks per sample: one per NTH * VPT vectors (NTH scalars) of the frame row, one when only the state moves
unsigned blocks_x(bool frame, bool vec, int64_t per_sample) {
  if (!frame) return 1;
  const int64_t per_block = vec ? (int64_t)NTH * VPT * 4 : NTH;
  const int64_t nb = (per_sample + per_block - 1) / per_block;
  return (unsigned)(nb < MAX_BX ? nb : MAX_BX);
}

}  // namespace

extern "C" {

int32_t acg_sched_sample_draw(uint64_t* state, const acg_ss_schedule* sched, float* mask, float* prob_out, int32_t steps,
                              int32_t batch, int32_t stream_id, acg_stream_t stream) {
  ACG_REQUIRE(state && sched && mask && prob_out, ACG_ERR_INVALID_ARG, "sched_sample_draw: null pointer");
  ACG_REQUIRE(sched->kind == ACG_SS_CONSTANT || sched->kind == ACG_SS_LINEAR || sched->kind == ACG_SS_INVERSE_SIGMOID,
              ACG_ERR_INVALID_ARG, "sched_sample_draw: schedule kind %d", sched->kind);
  ACG_REQUIRE(sched->start >= 0.f && sched->start <= 1.f && sched->final >= 0.f && sched->final <= 1.f, ACG_ERR_INVALID_ARG,
              "sched_sample_draw: start %g / final %g outside [0, 1]", (double)sched->start, (double)sched->final);
  ACG_REQUIRE(sched->offset >= 0, ACG_ERR_INVALID_ARG, "sched_sample_draw: offset %lld", (long long)sched->offset);
  ACG_REQUIRE(sched->kind == ACG_SS_CONSTANT || sched->decay_steps >= 1, ACG_ERR_INVALID_ARG,
              "sched_sample_draw: decay_steps %lld (>= 1 for a decaying schedule)", (long long)sched->decay_steps);
  ACG_REQUIRE(steps >= 1 && batch >= 1 && (int64_t)steps * batch <= ACG_NOISE_VALUES_MAX, ACG_ERR_INVALID_ARG,
              "sched_sample_draw: %d x %d coins outside 1..%d", steps, batch, ACG_NOISE_VALUES_MAX);
  const Sched sc{sched->kind, (long long)sched->offset, (long long)sched->decay_steps, sched->start, sched->final};
  ACG_LAUNCH(sched_sample_draw_kernel, dim3(1), dim3(NTH), 0, acg::to_stream(stream), (unsigned long long*)state, sc, mask, prob_out,
             (int)(steps * batch), (uint32_t)stream_id ^ ACG_SS_STREAM_TAG);
  return acg::check_launch("sched_sample_draw");
}

int32_t acg_sched_sample_fwd(const float* mask, const float* pred, const float* truth, float* out, int64_t per_sample,
                             const float* pred_state, const float* true_state, float* out_state, int32_t state_dim, int32_t batch,
                             acg_stream_t stream) {
  const bool frame = pred || truth || out, st = pred_state || true_state || out_state;
  ACG_REQUIRE(mask, ACG_ERR_INVALID_ARG, "sched_sample_fwd: null mask");
  ACG_REQUIRE(frame || st, ACG_ERR_INVALID_ARG, "sched_sample_fwd: neither a frame nor a state to select");
  ACG_REQUIRE(!frame || (pred && truth && out && per_sample >= 1), ACG_ERR_INVALID_ARG,
              "sched_sample_fwd: the frame needs pred, truth, out and per_sample >= 1 (got %lld)", (long long)per_sample);
  ACG_REQUIRE(!st || (pred_state && true_state && out_state && state_dim >= 1), ACG_ERR_INVALID_ARG,
              "sched_sample_fwd: the state needs pred_state, true_state, out_state and state_dim >= 1 (got %d)", state_dim);
  ACG_REQUIRE(batch >= 1 && batch <= 65535, ACG_ERR_INVALID_ARG, "sched_sample_fwd: batch %d outside 1..65535", batch);
  const bool vec = frame && per_sample % 4 == 0 && aligned16(pred) && aligned16(truth) && aligned16(out);
  const dim3 grid(blocks_x(frame, vec, per_sample), batch);
  if (vec)
    ACG_LAUNCH(sched_sample_fwd_kernel<true>, grid, dim3(NTH), 0, acg::to_stream(stream), mask, pred, truth, out, (long long)per_sample,
               pred_state, true_state, out_state, (int)state_dim);
  else
    ACG_LAUNCH(sched_sample_fwd_kernel<false>, grid, dim3(NTH), 0, acg::to_stream(stream), mask, pred, truth, out, (long long)per_sample,
               pred_state, true_state, out_state, (int)state_dim);
  return acg::check_launch("sched_sample_fwd");
}

int32_t acg_sched_sample_bwd(const float* mask, const float* dout, float* dpred, int64_t per_sample, const float* dout_state,
                             float* dpred_state, int32_t state_dim, int32_t batch, acg_stream_t stream) {
  const bool frame = dout || dpred, st = dout_state || dpred_state;
  ACG_REQUIRE(mask, ACG_ERR_INVALID_ARG, "sched_sample_bwd: null mask");
  ACG_REQUIRE(frame || st, ACG_ERR_INVALID_ARG, "sched_sample_bwd: neither a frame nor a state gradient");
  ACG_REQUIRE(!frame || (dout && dpred && per_sample >= 1), ACG_ERR_INVALID_ARG,
              "sched_sample_bwd: the frame needs dout, dpred and per_sample >= 1 (got %lld)", (long long)per_sample);
  ACG_REQUIRE(!st || (dout_state && dpred_state && state_dim >= 1), ACG_ERR_INVALID_ARG,
              "sched_sample_bwd: the state needs dout_state, dpred_state and state_dim >= 1 (got %d)", state_dim);
  ACG_REQUIRE(batch >= 1 && batch <= 65535, ACG_ERR_INVALID_ARG, "sched_sample_bwd: batch %d outside 1..65535", batch);
  const bool vec = frame && per_sample % 4 == 0 && aligned16(dout) && aligned16(dpred);
  const dim3 grid(blocks_x(frame, vec, per_sample), batch);
  if (vec)
    ACG_LAUNCH(sched_sample_bwd_kernel<true>, grid, dim3(NTH), 0, acg::to_stream(stream), mask, dout, dpred, (long long)per_sample, dout_state,
               dpred_state, (int)state_dim);
  else
    ACG_LAUNCH(sched_sample_bwd_kernel<false>, grid, dim3(NTH), 0, acg::to_stream(stream), mask, dout, dpred, (long long)per_sample, dout_state,
               dpred_state, (int)state_dim);
  return acg::check_launch("sched_sample_bwd");
}

}  // extern "C"
