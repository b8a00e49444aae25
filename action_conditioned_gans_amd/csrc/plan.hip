// Planning with the generator by the cross-entropy method (include/acgan_rollout.h): the three launches that sit around the N
// generator forwards of an iteration - draw N candidate action sequences, score the predicted frames against a goal, refit the
// sampling distribution to the best E - so that nothing of the optimiser runs on the host and nothing but the final plan leaves
// the device.  No float atomics and a fixed summation order in all three: the same inputs give the same bits.
//
// Sample.  One block, as the noise draw (noise.hip), of as many waves as there are Philox blocks to draw, up to 16: at most
// 131 072 normals = 32 768 Philox blocks, 32 per thread; the call is launch-latency bound beside N generator forwards, and one
// block needs no handshake for the counter: every thread reads it, a barrier, thread 0 stores counter + 1 (a second block,
// starting late, would read the advanced counter).
//
// Cost.  One block per candidate: 256 threads stride over the frame with 16-byte loads where the layout allows (a dense frame is
// read flat, a pitch-4 frame pixel by pixel), each thread sums its squares in float32, the 64 lanes of a wave by shuffles, the four
// waves through LDS in wave order.  49 KB per candidate at 64 x 64 x 3; N blocks fill the part from N = 256 on.
//
// Pixel cost.  The cost kernel's shape on d <= 4 probability maps [h, w, d] instead of a frame: 4 d sums per candidate (mass, mass x
// distance to the goal, mass x y, mass x x) in one pass, then the same block divides the maps it has just read by their mass.
// 16 KB per candidate and map at 64 x 64: read once from memory, re-read from cache, written once.
//
// Refit.  One block of up to 1024 threads.  The keys (cost, NaN as +inf) go to LDS; thread n counts the keys that come before its
// own - every lane of a wave reads the same 16 bytes of LDS in the same cycle, a broadcast, so the O(N^2) loop has no bank
// conflict and costs N / 4 ds_read_b128 per thread.  The E best are scattered to LDS by rank; thread (t, a) then sums its
// column over them in rank order, twice (mean, then squared deviations).  At most 2 x 1024 coalesced row reads of <= 512 bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/acgan_rollout.h"
#include "common.h"
#include "philox.h"

namespace {

constexpr int NTH = 256;                                 // the cost kernel's block
constexpr int SAMPLE_MAX = 1024;                         // the sample kernel's block at most
constexpr int REFIT_MAX = ACG_PLAN_CANDIDATES_MAX;       // one thread per candidate
constexpr int HA_MAX = ACG_PLAN_HORIZON_MAX * ACG_PLAN_ACTION_DIM_MAX;

// ---- sample -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAMPLE_MAX) void plan_sample_kernel(const float* __restrict__ mean, const float* __restrict__ std,
                                                                 const float* __restrict__ lo, const float* __restrict__ hi,
                                                                 unsigned long long* __restrict__ state, float* __restrict__ actions,
                                                                 int n, int HA, int A, int keep_mean, uint32_t stream_word) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const acg::DrawState draw = acg::load_draw_state(state);
  for (int i = tid; i * 4 < n; i += nth) {
    uint32_t c[4];
    float z[4];
    acg::draw_block(draw, (uint32_t)i, stream_word, c);
    acg::normals(c, z);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int e = i * 4 + l;                 // the tail of the last Philox block is dropped
      if (e < n) {
        const int ta = e % HA, a = ta % A;
        const float m = mean[ta];
        const float v = (keep_mean && e < HA) ? m : fmaf(std[ta], z[l], m);      // row 0: the mean itself, no noise
        actions[e] = fminf(fmaxf(v, lo[a]), hi[a]);
      }
    }
  }
  acg::advance_draw_state(state, draw);
}

// ---- cost ---------------------------------------------------------------------------------------------------------------------
enum { SCALAR = 0, DENSE4 = 1, PITCH4 = 2 };

// sum over this thread's share of (frame - goal)^2, channels c < C of every pixel
template <typename T, int MODE>
__device__ __forceinline__ float sq_partial(const T* __restrict__ f, const float* __restrict__ goal, int pixels, int C, int pitch) {
  float acc = 0.f;
  if constexpr (MODE == DENSE4) {              // pitch == C: frame and goal are the same flat array, 4 values per load
    const int nv = (pixels * C) >> 2;
    for (int v = threadIdx.x; v < nv; v += NTH) {
      float x[4], g[4];
      acg::ldv<4>(f + 4 * v, x);
      acg::ldv<4>(goal + 4 * v, g);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = x[k] - g[k];
        acc = fmaf(d, d, acc);
      }
    }
  } else if constexpr (MODE == PITCH4) {       // one 4-channel pixel per load; the pad channels are loaded and not used
    for (int p = threadIdx.x; p < pixels; p += NTH) {
      float x[4];
      acg::ldv<4>(f + 4 * p, x);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < C) {
          const float d = x[k] - goal[p * C + k];
          acc = fmaf(d, d, acc);
        }
    }
  } else {
    for (int p = threadIdx.x; p < pixels; p += NTH)
      for (int k = 0; k < C; ++k) {
        const float d = acg::ldf(f + (long long)p * pitch + k) - goal[p * C + k];
        acc = fmaf(d, d, acc);
      }
  }
  return acc;
}

template <typename T, int MODE>
__global__ __launch_bounds__(NTH) void plan_cost_kernel(const T* __restrict__ frames, const float* __restrict__ goal,
                                                        const float* __restrict__ states, const float* __restrict__ goal_state,
                                                        float frame_weight, float state_weight, float* __restrict__ cost,
                                                        int accumulate, int pixels, int C, int pitch, int S) {
  __shared__ float scratch[16];
  const int n = blockIdx.x;
  const float part = sq_partial<T, MODE>(frames + (long long)n * pixels * pitch, goal, pixels, C, pitch);
  const float fs = acg::block_sum(part, scratch);      // lanes by shuffles, then the waves in order: thread 0 holds the sum
  if (threadIdx.x == 0) {
    float ss = 0.f;
    if (states)
      for (int s = 0; s < S; ++s) {
        const float d = states[n * S + s] - goal_state[s];
        ss = fmaf(d, d, ss);
      }
    const float c = frame_weight * fs + state_weight * ss;
    cost[n] = accumulate ? cost[n] + c : c;            // accumulate == 0: the old value is not read
  }
}

template <typename T>
void launch_cost(int mode, hipStream_t st, int N, const void* frames, const float* goal, const float* states, const float* goal_state,
                 float fw, float sw, float* cost, int accumulate, int pixels, int C, int pitch, int S) {
  const T* f = static_cast<const T*>(frames);
  if (mode == DENSE4)
    ACG_LAUNCH((plan_cost_kernel<T, DENSE4>), dim3(N), dim3(NTH), 0, st, f, goal, states, goal_state, fw, sw, cost, accumulate, pixels, C, pitch, S);
  else if (mode == PITCH4)
    ACG_LAUNCH((plan_cost_kernel<T, PITCH4>), dim3(N), dim3(NTH), 0, st, f, goal, states, goal_state, fw, sw, cost, accumulate, pixels, C, pitch, S);
  else
    ACG_LAUNCH((plan_cost_kernel<T, SCALAR>), dim3(N), dim3(NTH), 0, st, f, goal, states, goal_state, fw, sw, cost, accumulate, pixels, C, pitch, S);
}

// ---- pixel cost ---------------------------------------------------------------------------------------------------------------
// one pixel of D interleaved maps; VEC: one 8- or 16-byte access (D = 2, 4 and an aligned base), else D scalar ones
template <int D, bool VEC>
__device__ __forceinline__ void ld_px(const float* p, float (&v)[D]) {
  if constexpr (VEC && D == 4) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  else if constexpr (VEC && D == 2) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; }
  else {
#pragma unroll
    for (int j = 0; j < D; ++j) v[j] = p[j];
  }
}
template <int D, bool VEC>
__device__ __forceinline__ void st_px(float* p, const float (&v)[D]) {
  if constexpr (VEC && D == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else if constexpr (VEC && D == 2) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  else {
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] = v[j];
  }
}

// One block per candidate.  Pass 1: thread t sums mass, mass x distance, mass x y and mass x x of the pixels t, t + 256, ... of every
// map; the 4 D partials go through the lanes by shuffles and through LDS in wave order, and EVERY thread adds the four wave sums
// itself, so all of them hold the same totals without a broadcast.  Pass 2: the thread divides the pixels it read - nobody else's -
// by the mass, out of the cache lines it has just pulled in.  A frame smaller than the block leaves threads without a pixel: their
// partials are 0 and they take part in the shuffles and the barrier like everybody else.
template <int D, bool VEC>
__global__ __launch_bounds__(NTH) void plan_pixel_cost_kernel(float* __restrict__ maps, const float* __restrict__ goals, float pixel_weight,
                                                              float* __restrict__ cost, int accumulate, float* __restrict__ expected,
                                                              float* __restrict__ mass, int pixels, int W) {
  __shared__ float part[4 * D][NTH / acg::kWave];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* P = maps + (long long)n * pixels * D;
  float gy[D], gx[D], acc[4 * D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    gy[j] = goals[2 * j];
    gx[j] = goals[2 * j + 1];
    acc[4 * j] = acc[4 * j + 1] = acc[4 * j + 2] = acc[4 * j + 3] = 0.f;
  }
  for (int p = tid; p < pixels; p += NTH) {
    const int yi = p / W;
    const float y = (float)yi, x = (float)(p - yi * W);
    float v[D];
    ld_px<D, VEC>(P + p * D, v);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float dy = y - gy[j], dx = x - gx[j];
      const float dist = sqrtf(fmaf(dy, dy, dx * dx));
      acc[4 * j] += v[j];
      acc[4 * j + 1] = fmaf(v[j], dist, acc[4 * j + 1]);
      acc[4 * j + 2] = fmaf(v[j], y, acc[4 * j + 2]);
      acc[4 * j + 3] = fmaf(v[j], x, acc[4 * j + 3]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4 * D; ++q) {
    const float s = acg::wave_sum(acc[q]);
    if (lane == 0) part[q][wave] = s;
  }
  __syncthreads();
  float m0[D];
  bool ok[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    m0[j] = ((part[4 * j][0] + part[4 * j][1]) + part[4 * j][2]) + part[4 * j][3];
    ok[j] = m0[j] > 0.f && m0[j] < INFINITY;           // (a NaN fails both)
  }
  if (tid == 0) {
    float sum = 0.f;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float m1 = ((part[4 * j + 1][0] + part[4 * j + 1][1]) + part[4 * j + 1][2]) + part[4 * j + 1][3];
      const float ey = ((part[4 * j + 2][0] + part[4 * j + 2][1]) + part[4 * j + 2][2]) + part[4 * j + 2][3];
      const float ex = ((part[4 * j + 3][0] + part[4 * j + 3][1]) + part[4 * j + 3][2]) + part[4 * j + 3][3];
      if (ok[j]) sum += m1 / m0[j];
      else bad = true;
      if (expected) {
        expected[(n * D + j) * 2] = ok[j] ? ey / m0[j] : NAN;
        expected[(n * D + j) * 2 + 1] = ok[j] ? ex / m0[j] : NAN;
      }
      if (mass) mass[n * D + j] = m0[j];
    }
    const float c = bad ? INFINITY : pixel_weight * sum;   // a map without mass: +inf whatever the weight (0 * inf would be a NaN)
    cost[n] = accumulate ? cost[n] + c : c;                // accumulate == 0: the old value is not read
  }
  bool any = false;
#pragma unroll
  for (int j = 0; j < D; ++j) any = any || ok[j];
  if (!any) return;                                        // nothing to scale (uniform in the block)
  for (int p = tid; p < pixels; p += NTH) {
    float v[D];
    ld_px<D, VEC>(P + p * D, v);
#pragma unroll
    for (int j = 0; j < D; ++j)
      if (ok[j]) v[j] = v[j] / m0[j];
    st_px<D, VEC>(P + p * D, v);
  }
}

template <int D>
void launch_pixel_cost(bool vec, hipStream_t st, int N, float* maps, const float* goals, float pw, float* cost, int accumulate,
                       float* expected, float* mass, int pixels, int W) {
  if constexpr (D == 2 || D == 4) {                      // (D = 1 is a scalar access anyway, D = 3 has no vector form)
    if (vec) {
      ACG_LAUNCH((plan_pixel_cost_kernel<D, true>), dim3(N), dim3(NTH), 0, st, maps, goals, pw, cost, accumulate, expected, mass, pixels, W);
      return;
    }
  }
  ACG_LAUNCH((plan_pixel_cost_kernel<D, false>), dim3(N), dim3(NTH), 0, st, maps, goals, pw, cost, accumulate, expected, mass, pixels, W);
}

// ---- refit --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(REFIT_MAX) void plan_refit_kernel(const float* __restrict__ cost, const float* __restrict__ actions,
                                                               float* __restrict__ mean, float* __restrict__ std,
                                                               float* __restrict__ best_cost, float* __restrict__ best_actions,
                                                               int* __restrict__ elite_idx, float* __restrict__ history, int N, int HA,
                                                               int E, float alpha, float min_std) {
  __shared__ __attribute__((aligned(16))) float key[REFIT_MAX];
  __shared__ int elite[REFIT_MAX];
  const int tid = threadIdx.x;
  const float old_best = best_cost[0];                 // read by every thread before anything is written (barriers below)
  const int Np = (N + 3) & ~3;
  float mine = INFINITY;
  if (tid < Np) {
    if (tid < N) {
      const float c = cost[tid];
      mine = c != c ? INFINITY : c;                    // NaN ranks with +inf: last, by index
    }
    key[tid] = mine;                                   // (the pad keys [N, Np) are +inf at an index >= N: they precede nobody)
  }
  __syncthreads();
  if (tid < N) {
    int rank = 0;
    for (int m = 0; m < Np; m += 4) {                  // one 16-byte LDS read per 4 keys, the same address in every lane: a broadcast
      const float4 k = *reinterpret_cast<const float4*>(key + m);
      rank += (k.x < mine || (k.x == mine && m < tid)) + (k.y < mine || (k.y == mine && m + 1 < tid))
              + (k.z < mine || (k.z == mine && m + 2 < tid)) + (k.w < mine || (k.w == mine && m + 3 < tid));
    }
    if (rank < E) elite[rank] = tid;                   // the order is total: every rank below N is taken exactly once
  }
  __syncthreads();
  if (tid < E) elite_idx[tid] = elite[tid];
  const int first = elite[0];
  const float first_key = key[first];
  const bool improved = first_key < old_best;          // strict: an equal cost keeps the earlier plan; uniform in the block
  if (tid < HA) {
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < E; ++r) s += actions[elite[r] * HA + tid];           // rank order, sequential
    const float mean_e = s / (float)E;
    float q = 0.f;
#pragma unroll 8
    for (int r = 0; r < E; ++r) {
      const float d = actions[elite[r] * HA + tid] - mean_e;
      q = fmaf(d, d, q);
    }
    const float std_e = sqrtf(q / (float)E);           // population standard deviation
    mean[tid] = alpha * mean[tid] + (1.f - alpha) * mean_e;
    std[tid] = fmaxf(alpha * std[tid] + (1.f - alpha) * std_e, min_std);
    if (improved) best_actions[tid] = actions[first * HA + tid];
  }
  if (tid == 0) {
    if (improved) best_cost[0] = first_key;
    if (history) history[0] = improved ? first_key : old_best;
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int32_t check_shape(const char* who, int32_t N, int32_t H, int32_t A) {
  ACG_REQUIRE(N >= 1 && H >= 1 && A >= 1, ACG_ERR_INVALID_ARG, "%s: candidates %d, horizon %d, action_dim %d (all >= 1)", who, N, H, A);
  ACG_REQUIRE(N <= ACG_PLAN_CANDIDATES_MAX && H <= ACG_PLAN_HORIZON_MAX && A <= ACG_PLAN_ACTION_DIM_MAX, ACG_ERR_UNSUPPORTED,
              "%s: candidates %d, horizon %d, action_dim %d above %d, %d, %d", who, N, H, A, ACG_PLAN_CANDIDATES_MAX, ACG_PLAN_HORIZON_MAX,
              ACG_PLAN_ACTION_DIM_MAX);
  return ACG_OK;
}

}  // namespace

extern "C" {

int32_t acg_plan_sample(const float* mean, const float* std, const float* lo, const float* hi, uint64_t* state, float* actions,
                        int32_t candidates, int32_t horizon, int32_t action_dim, int32_t keep_mean, int32_t stream_id,
                        acg_stream_t stream) {
  ACG_REQUIRE(mean && std && lo && hi && state && actions, ACG_ERR_INVALID_ARG, "plan_sample: null pointer");
  if (int32_t rc = check_shape("plan_sample", candidates, horizon, action_dim)) return rc;
  const int n = candidates * horizon * action_dim, blocks4 = (n + 3) / 4;
  const int threads = blocks4 >= SAMPLE_MAX ? SAMPLE_MAX : (blocks4 + 63) & ~63;       // whole waves, one Philox block per thread and pass
  ACG_LAUNCH(plan_sample_kernel, dim3(1), dim3(threads), 0, acg::to_stream(stream), mean, std, lo, hi, (unsigned long long*)state, actions,
             n, (int)(horizon * action_dim), (int)action_dim, (int)keep_mean,
             (uint32_t)stream_id ^ ACG_PLAN_STREAM_TAG);
  return acg::check_launch("plan_sample");
}

int32_t acg_plan_cost(const void* frames, const float* goal, const float* states, const float* goal_state, float frame_weight,
                      float state_weight, float* cost, int32_t accumulate, int32_t candidates, int32_t h, int32_t w, int32_t c,
                      int32_t pitch, int32_t state_dim, int32_t dtype, acg_stream_t stream) {
  ACG_REQUIRE(frames && goal && cost, ACG_ERR_INVALID_ARG, "plan_cost: null pointer");
  ACG_REQUIRE((states == nullptr) == (goal_state == nullptr), ACG_ERR_INVALID_ARG, "plan_cost: states and goal_state go together");
  ACG_REQUIRE(states ? (state_dim >= 1 && state_dim <= ACG_PLAN_STATE_DIM_MAX) : state_dim == 0, ACG_ERR_INVALID_ARG,
              "plan_cost: state_dim %d (1..%d with states, 0 without)", state_dim, ACG_PLAN_STATE_DIM_MAX);
  ACG_REQUIRE(candidates >= 1 && h >= 1 && w >= 1, ACG_ERR_INVALID_ARG, "plan_cost: candidates %d, frame %d x %d (all >= 1)", candidates, h, w);
  ACG_REQUIRE(candidates <= ACG_PLAN_CANDIDATES_MAX, ACG_ERR_UNSUPPORTED, "plan_cost: %d candidates, at most %d", candidates,
              ACG_PLAN_CANDIDATES_MAX);
  ACG_REQUIRE(c >= 1 && c <= pitch && pitch <= 64, ACG_ERR_INVALID_ARG, "plan_cost: %d channels at a pitch of %d", c, pitch);
  ACG_REQUIRE((int64_t)h * w * pitch < (1LL << 31), ACG_ERR_UNSUPPORTED, "plan_cost: a frame of %d x %d x %d", h, w, pitch);
  ACG_REQUIRE(dtype == ACG_F32 || dtype == ACG_BF16, ACG_ERR_UNSUPPORTED, "plan_cost: dtype %d (ACG_F32 or ACG_BF16 frames)", dtype);
  const int pixels = h * w, esz = acg::dt_size(dtype);
  // 16-byte loads (8 for bf16) need every candidate's frame aligned: the base, and a frame length that is a multiple of 4 values
  int mode = SCALAR;
  if (pitch == c && (pixels * c) % 4 == 0 && aligned(frames, 4 * esz) && aligned(goal, 16)) mode = DENSE4;
  else if (pitch == 4 && c < 4 && aligned(frames, 4 * esz)) mode = PITCH4;
  const hipStream_t st = acg::to_stream(stream);
  if (dtype == ACG_F32)
    launch_cost<float>(mode, st, candidates, frames, goal, states, goal_state, frame_weight, state_weight, cost, accumulate, pixels, c, pitch,
                       state_dim);
  else
    launch_cost<__bf16>(mode, st, candidates, frames, goal, states, goal_state, frame_weight, state_weight, cost, accumulate, pixels, c, pitch,
                        state_dim);
  return acg::check_launch("plan_cost");
}

int32_t acg_plan_pixel_cost(float* maps, const float* goals, float pixel_weight, float* cost, int32_t accumulate, float* expected,
                            float* mass, int32_t candidates, int32_t h, int32_t w, int32_t d, acg_stream_t stream) {
  ACG_REQUIRE(maps && goals && cost, ACG_ERR_INVALID_ARG, "plan_pixel_cost: null pointer");
  ACG_REQUIRE(candidates >= 1 && h >= 1 && w >= 1 && d >= 1, ACG_ERR_INVALID_ARG,
              "plan_pixel_cost: candidates %d, maps %d x %d x %d (all >= 1)", candidates, h, w, d);
  ACG_REQUIRE(pixel_weight >= 0.f && pixel_weight < INFINITY, ACG_ERR_INVALID_ARG, "plan_pixel_cost: pixel_weight %g (finite, >= 0)",
              (double)pixel_weight);
  ACG_REQUIRE(candidates <= ACG_PLAN_CANDIDATES_MAX && d <= ACG_PLAN_PIXEL_MAPS_MAX && h <= ACG_PLAN_MAP_SIDE_MAX && w <= ACG_PLAN_MAP_SIDE_MAX,
              ACG_ERR_UNSUPPORTED, "plan_pixel_cost: candidates %d, maps %d x %d x %d above %d, %d x %d x %d", candidates, h, w, d,
              ACG_PLAN_CANDIDATES_MAX, ACG_PLAN_MAP_SIDE_MAX, ACG_PLAN_MAP_SIDE_MAX, ACG_PLAN_PIXEL_MAPS_MAX);
  const int pixels = h * w;                              // <= 2^20, and pixels * d <= 2^22: the kernel's int indices
  const bool vec = aligned(maps, 4 * d);                 // (every candidate's maps then are: pixels * d * 4 bytes apart)
  const hipStream_t st = acg::to_stream(stream);
  switch (d) {
    case 1: launch_pixel_cost<1>(vec, st, candidates, maps, goals, pixel_weight, cost, accumulate, expected, mass, pixels, w); break;
    case 2: launch_pixel_cost<2>(vec, st, candidates, maps, goals, pixel_weight, cost, accumulate, expected, mass, pixels, w); break;
    case 3: launch_pixel_cost<3>(vec, st, candidates, maps, goals, pixel_weight, cost, accumulate, expected, mass, pixels, w); break;
    default: launch_pixel_cost<4>(vec, st, candidates, maps, goals, pixel_weight, cost, accumulate, expected, mass, pixels, w); break;
  }
  return acg::check_launch("plan_pixel_cost");
}

int32_t acg_plan_refit(const float* cost, const float* actions, float* mean, float* std, float* best_cost, float* best_actions,
                       int32_t* elite_idx, float* history, int32_t candidates, int32_t horizon, int32_t action_dim, int32_t elites,
                       float alpha, float min_std, acg_stream_t stream) {
  ACG_REQUIRE(cost && actions && mean && std && best_cost && best_actions && elite_idx, ACG_ERR_INVALID_ARG, "plan_refit: null pointer");
  if (int32_t rc = check_shape("plan_refit", candidates, horizon, action_dim)) return rc;
  ACG_REQUIRE(elites >= 1 && elites <= candidates, ACG_ERR_INVALID_ARG, "plan_refit: %d elites of %d candidates", elites, candidates);
  ACG_REQUIRE(alpha >= 0.f && alpha <= 1.f, ACG_ERR_INVALID_ARG, "plan_refit: alpha %g outside [0, 1]", (double)alpha);
  ACG_REQUIRE(min_std >= 0.f && min_std < INFINITY, ACG_ERR_INVALID_ARG, "plan_refit: min_std %g (finite, >= 0)", (double)min_std);
  const int HA = horizon * action_dim;
  static_assert(HA_MAX <= REFIT_MAX, "one thread per (t, a)");
  const int need = candidates > HA ? candidates : HA;
  const int threads = (need + 63) & ~63;               // whole waves: candidates, (t, a) columns and elites each get a thread
  ACG_LAUNCH(plan_refit_kernel, dim3(1), dim3(threads), 0, acg::to_stream(stream), cost, actions, mean, std, best_cost, best_actions,
             (int*)elite_idx, history, (int)candidates, HA, (int)elites, alpha, min_std);
  return acg::check_launch("plan_refit");
}

}  // extern "C"
