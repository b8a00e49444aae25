// TensorFlow-1.0 Adam / RMSProp over FLAT float32 buffers (train.py:91-102) with the discriminator
// weight clip of train.py:89,140-143 fused after the update (defect D6 resolved as update -> clip).
// All variables of one scope are views into one flat buffer, so a whole network updates in ONE launch:
// pure streaming, 16 B per lane, read p/g/slots + write p/slots once.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/acgan_ema.h"
#include "../../include/acgan_rollout.h"
#include "common.h"
#include "ema_common.h"

namespace {

__device__ __forceinline__ float clipf(float v, int use, float lo, float hi) { return use ? fminf(fmaxf(v, lo), hi) : v; }

// (explicitly rounded operations: the same sequence whichever kernel inlines it - hipcc otherwise contracts multiplies and adds
// into FMAs differently in different contexts, and the flat kernels and opt_prepare_k below must agree bit for bit)
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float lr_t, float b1, float b2, float eps,
                                      float gs, int use_clip, float lo, float hi) {
  g = __fmul_rn(g, gs);
  m = __fmaf_rn(b1, m, __fmul_rn(1.f - b1, g));
  v = __fmaf_rn(b2, v, __fmul_rn(__fmul_rn(1.f - b2, g), g));
  p = clipf(__fsub_rn(p, __fdiv_rn(__fmul_rn(lr_t, m), __fadd_rn(sqrtf(v), eps))), use_clip, lo, hi);
}

__device__ __forceinline__ void rms1(float& p, float g, float& ms, float lr, float decay, float eps, float gs, int use_clip,
                                     float lo, float hi) {
  g = __fmul_rn(g, gs);
  ms = __fmaf_rn(decay, ms, __fmul_rn(__fmul_rn(1.f - decay, g), g));
  p = clipf(__fsub_rn(p, __fdiv_rn(__fmul_rn(lr, g), sqrtf(__fadd_rn(ms, eps)))), use_clip, lo, hi);
}

struct OptScalars {
  float lr, b1, b2, eps, gs, lo, hi;      // b1: Adam's beta1, RMSProp's decay
  int use_clip;
};

// ---- the learning-rate schedule of the *_step_lr entries (include/acgan_rollout.h acg_lr_schedule) -------------------------------
// The launch's own view of the schedule: the shape as the host read it, the update counter the launch advances, that counter's
// state word, and where block 0 leaves the rate it used.
struct LrArgs {
  int kind;
  long long warmup, decay_steps;
  float final_factor;
  long long* updates;
  unsigned* done;
  float* out;
};

// lr_k, the rate of update k: all of it in double, one rounding to float32 at the end (the header states the formulas).  ONE
// thread per block evaluates it, in the prologue that holds Adam's two pow calls anyway.
__device__ __forceinline__ float lr_at(float lr, const LrArgs& s, long long k) {
  const double F = (double)s.final_factor;
  const double w = (s.warmup > 0 && k < s.warmup) ? (double)(k + 1) / (double)s.warmup : 1.0;
  double f = 1.0;
  if (s.kind != ACG_LR_CONSTANT) {
    const double j = (double)(k > s.warmup ? k - s.warmup : 0);
    const double t = fmin(j / (double)s.decay_steps, 1.0);
    if (s.kind == ACG_LR_LINEAR) f = 1.0 - (1.0 - F) * t;
    else if (s.kind == ACG_LR_COSINE) f = F + (1.0 - F) * 0.5 * (1.0 + cos(3.14159265358979323846 * t));
    else f = pow(F, j / (double)s.decay_steps);
  }
  return (float)((double)lr * w * f);
}

// ---- the update rules: what a kernel below is instantiated with -----------------------------------------------------------------
// kSlots: the slot buffers the rule reads and writes (a one-slot rule never touches s2); kPrologue: `rate` must be derived by
// one thread of the block before any element is updated; one(): the update of one element, given that rate.  `lr`: the base
// rate of this launch - the argument, or what the schedule makes of it.
struct Adam {
  static constexpr int kSlots = 2;
  static constexpr bool kPrologue = true;
  // lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)   (SURVEY A.6); fp64 pow keeps the tiny 1-b^t differences exact.  ONE thread per
  // block evaluates it: a dependent read of the step counter and two double-precision pow calls, several hundred
  // instructions (~1 us) - more than the whole update of the one or two float4 a thread owns.
  static __device__ __forceinline__ float rate(float lr, const OptScalars& a, const int* step) {
    const int t = *step;
    return (float)((double)lr * sqrt(1.0 - pow((double)a.b2, (double)t)) / (1.0 - pow((double)a.b1, (double)t)));
  }
  static __device__ __forceinline__ void one(float& p, float g, float& m, float& v, float lr_t, const OptScalars& a) {
    adam1(p, g, m, v, lr_t, a.b1, a.b2, a.eps, a.gs, a.use_clip, a.lo, a.hi);
  }
};
struct RmsProp {
  static constexpr int kSlots = 1;
  static constexpr bool kPrologue = false;
  static __device__ __forceinline__ float rate(float lr, const OptScalars&, const int*) { return lr; }
  static __device__ __forceinline__ void one(float& p, float g, float& ms, float&, float lr, const OptScalars& a) {
    rms1(p, g, ms, lr, a.b1, a.eps, a.gs, a.use_clip, a.lo, a.hi);
  }
};

template <class R>
__device__ __forceinline__ void four(float4& p, const float4& g, float4& s1, float4& s2, float rate, const OptScalars& a) {
  R::one(p.x, g.x, s1.x, s2.x, rate, a);
  R::one(p.y, g.y, s1.y, s2.y, rate, a);
  R::one(p.z, g.z, s1.z, s2.z, rate, a);
  R::one(p.w, g.w, s1.w, s2.w, rate, a);
}

// ---- the update over flat float32 buffers: the body of adam_k, rmsprop_k and of the two kernels that carry the weight average ----
// EMA: the shadow element (include/acgan_ema.h) is updated from the new parameter while it is still in a register - one launch
// instead of two, and the average costs a read and a write of the shadow instead of those plus a second read of the parameters;
// parameters and slots come out as without it, the shadow as ema_update_k behind the plain kernel leaves it.  The prologue
// thread then also derives the average's coefficient, and retires the launch's count of it at the end.
// SCHED: the base rate is the schedule's (lr_at) at the update counter `lr.updates`, which the prologue thread reads in front of
// the rule's own rate() and retires at the end as the average's is; block 0 leaves the rate in lr.out.  A rule without a
// prologue gets one.  Every block reads the counter before the last one to retire stores it, so all use the same rate.
template <class R, bool EMA, bool SCHED = false>
__device__ __forceinline__ void flat_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                            float* __restrict__ s2, const int* __restrict__ step, long long n, const OptScalars& a,
                                            float* __restrict__ sh, float ema_decay, long long* num_updates, unsigned* done,
                                            const LrArgs& lr = LrArgs{}) {
  constexpr bool kTwo = R::kSlots == 2, kRate = R::kPrologue || SCHED, kPrologue = kRate || EMA;
  __shared__ float s_rate;
  __shared__ acg_ema::Coef s_c;
  const long long stride = (long long)gridDim.x * 256;
  const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(s1) |
                    (kTwo ? reinterpret_cast<uintptr_t>(s2) : 0) | (EMA ? reinterpret_cast<uintptr_t>(sh) : 0)) & 15) == 0;
  const long long n4 = al ? n / 4 : 0;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
  float rate = a.lr, omd = 0.f;
  int seed = 0;
  long long k = 0, lr_k = 0;
  float4 pp, gg, aa, bb, ss;
  auto load = [&](long long i) {
    pp = reinterpret_cast<float4*>(p)[i]; aa = reinterpret_cast<float4*>(s1)[i];
    if constexpr (kTwo) bb = reinterpret_cast<float4*>(s2)[i];
    gg = reinterpret_cast<const float4*>(g)[i];
    if constexpr (EMA) ss = reinterpret_cast<float4*>(sh)[i];
  };
  auto update = [&](long long i) {
    four<R>(pp, gg, aa, bb, rate, a);
    reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(s1)[i] = aa;
    if constexpr (kTwo) reinterpret_cast<float4*>(s2)[i] = bb;
    if constexpr (EMA) { acg_ema::ema4(ss, pp, omd, seed); reinterpret_cast<float4*>(sh)[i] = ss; }
  };
  long long i = i0;
  if constexpr (kPrologue) {
    // Round 5: the first float4 of every thread (the grid is sized so that it is nearly the only one) is loaded BEFORE the
    // prologue, during which the whole chip used to wait with nothing in flight (19.4 us for 133 MB in situ, 3.2 TB/s).
    // A kernel without a prologue has nothing to hide the load behind and keeps its plain loop (rmsprop_k; the scheduled
    // RMSProp has one and takes this path).  A scheduled launch runs fewer blocks (flat_step) and hides the first of its loads.
    const bool have = i0 < n4;
    if (have) load(i0);
    if (threadIdx.x == 0) {
      float base = a.lr;
      if constexpr (SCHED) {
        lr_k = *lr.updates;
        base = lr_at(a.lr, lr, lr_k);
        if (blockIdx.x == 0) *lr.out = base;
      }
      if constexpr (kRate) s_rate = R::rate(base, a, step);
      if constexpr (EMA) s_c = acg_ema::coef(num_updates, ema_decay, &k);
    }
    __syncthreads();
    if constexpr (kRate) rate = s_rate;
    if constexpr (EMA) { omd = s_c.omd; seed = s_c.seed; }
    if (have) update(i0);
    i += stride;
  }
  for (; i < n4; i += stride) { load(i); update(i); }
  for (i = n4 * 4 + i0; i < n; i += stride) {
    float none;
    R::one(p[i], g[i], s1[i], kTwo ? s2[i] : none, rate, a);
    if constexpr (EMA) sh[i] = acg_ema::ema1(sh[i], p[i], omd, seed);
  }
  if constexpr (EMA) if (threadIdx.x == 0) acg_ema::retire(num_updates, done, k);
  if constexpr (SCHED) if (threadIdx.x == 0) acg_ema::retire(lr.updates, lr.done, lr_k);
}

// (the kernels keep their names: tools/insitu_times.py, tools/gap_analysis.py and the committed traces find them by name)
__global__ __launch_bounds__(256) void adam_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, const int* __restrict__ step, long long n, float lr,
                                              float b1, float b2, float eps, float gs, int use_clip, float lo, float hi) {
  flat_update<Adam, false>(p, g, m, v, step, n, OptScalars{lr, b1, b2, eps, gs, lo, hi, use_clip}, nullptr, 0.f, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void rmsprop_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
                                                 long long n, float lr, float decay, float eps, float gs, int use_clip,
                                                 float lo, float hi) {
  flat_update<RmsProp, false>(p, g, ms, nullptr, nullptr, n, OptScalars{lr, decay, 0.f, eps, gs, lo, hi, use_clip}, nullptr, 0.f, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void adam_ema_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, const int* __restrict__ step, long long n, float lr,
                                                  float b1, float b2, float eps, float gs, int use_clip, float lo, float hi,
                                                  float* __restrict__ sh, float ema_decay, long long* num_updates, unsigned* done) {
  flat_update<Adam, true>(p, g, m, v, step, n, OptScalars{lr, b1, b2, eps, gs, lo, hi, use_clip}, sh, ema_decay, num_updates, done);
}

__global__ __launch_bounds__(256) void rmsprop_ema_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
                                                     long long n, float lr, float decay, float eps, float gs, int use_clip,
                                                     float lo, float hi, float* __restrict__ sh, float ema_decay,
                                                     long long* num_updates, unsigned* done) {
  flat_update<RmsProp, true>(p, g, ms, nullptr, nullptr, n, OptScalars{lr, decay, 0.f, eps, gs, lo, hi, use_clip}, sh, ema_decay, num_updates, done);
}

// The scheduled entries (acg_adam_step_lr / acg_rmsprop_step_lr): the same body, with or without the average.  RMSProp
// passes no second slot and no step counter.
template <class R, bool EMA>
__global__ __launch_bounds__(256) void step_lr_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                 float* __restrict__ s2, const int* __restrict__ step, long long n, const OptScalars a,
                                                 const LrArgs lr, float* __restrict__ sh, float ema_decay, long long* num_updates,
                                                 unsigned* done) {
  flat_update<R, EMA, true>(p, g, s1, s2, step, n, a, sh, ema_decay, num_updates, done, lr);
}

__global__ __launch_bounds__(256) void clip_k(float* __restrict__ p, long long n, float lo, float hi) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) p[i] = fminf(fmaxf(p[i], lo), hi);
}

__global__ void step_inc_k(int* step) { *step += 1; }

// ---- bf16 pipeline: optimizer update + refresh of the bf16 filter copies in ONE launch (acg_opt_step_prepare_bf16) ------------
// The conv kernels of a bf16 network read two bf16 copies of every filter [taps][A][B] - rm [taps][A][round8(B)] and the
// transpose tr [taps][B][round8(A)] (acg_weights_prepare_bf16) - which have to follow the float32 master weights after every
// update: a second launch over the whole scope right behind the optimizer's (round 3: 14 of the 37.5 us of D's update).
// Here a block owns one 32 (a) x 32 (b) tile of one tap of one filter: it updates the tile's elements (the same adam1 / rms1
// as the flat kernels: bit-identical parameters and slots), stores the rm run as it goes and the tr run through an LDS
// transpose; what lies between the filters in the flat buffer (beta, biases, alignment gaps) goes to one block per gap.
struct OptPrepList {
  long long off[ACG_PREP_MAX];            // element offset of filter e in the flat buffers
  __bf16* rm[ACG_PREP_MAX];
  __bf16* tr[ACG_PREP_MAX];
  int taps[ACG_PREP_MAX], A[ACG_PREP_MAX], B[ACG_PREP_MAX];
  int first_block[ACG_PREP_MAX + 1];      // tile blocks of entry e: [first_block[e], first_block[e + 1])
  long long gap_lo[ACG_PREP_MAX + 1], gap_len[ACG_PREP_MAX + 1];      // gap j is block first_block[count] + j
};

template <class R>       // Adam / RmsProp
__global__ __launch_bounds__(256) void opt_prepare_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                     float* __restrict__ s2, const int* __restrict__ step, const OptScalars a,
                                                     const OptPrepList l, int count) {
  __shared__ float tile[32][33];
  __shared__ float s_lr_t;
  float lr_t = a.lr;
  // Adam's bias-corrected learning rate: one thread derives it (a dependent read of the step counter + double-precision pow,
  // ~1-2 us); the block picks it up with `sync_lr()` - in the float4 path AFTER its loads are in flight (round 5)
  constexpr bool kTwo = R::kSlots == 2;
  if (R::kPrologue && threadIdx.x == 0) s_lr_t = R::rate(a.lr, a, step);
  auto sync_lr = [&]() { if (R::kPrologue) { __syncthreads(); lr_t = s_lr_t; } };     // block-uniform call sites only
  auto upd = [&](long long i) -> float {
    float none;
    R::one(p[i], g[i], s1[i], kTwo ? s2[i] : none, lr_t, a);
    return p[i];
  };
  const int blk = (int)blockIdx.x;
  if (blk >= l.first_block[count]) {             // a run between two filters: beta / bias vectors, alignment gaps
    const int j = blk - l.first_block[count];
    sync_lr();
    for (long long i = threadIdx.x; i < l.gap_len[j]; i += 256) upd(l.gap_lo[j] + i);
    return;
  }
  int e = 0;
  while (e + 1 < count && blk >= l.first_block[e + 1]) ++e;
  const int A = l.A[e], B = l.B[e], A8 = (A + 7) & ~7, B8 = (B + 7) & ~7;
  const int ta_n = (A8 + 31) >> 5, tb_n = (B8 + 31) >> 5;
  int t = blk - l.first_block[e];
  const int tb = t % tb_n; t /= tb_n;
  const int ta = t % ta_n, tap = t / ta_n;
  const int a0 = ta * 32, b0 = tb * 32;
  const int r = threadIdx.x >> 3, q = threadIdx.x & 7;
  if ((B & 3) == 0) {
    // rows are 16-byte aligned: thread -> (a = a0 + r, b run 4q .. 4q + 3), float4 accesses, the rm run as one 8-byte store
    const int ar = a0 + r, bq = b0 + 4 * q;
    float nv[4] = {0.f, 0.f, 0.f, 0.f};
    const bool have = ar < A && bq < B;
    const long long i0 = l.off[e] + ((long long)tap * A + ar) * B + bq;
    float4 pp, mm, gg, vv;
    if (have) {
      pp = *reinterpret_cast<float4*>(p + i0); mm = *reinterpret_cast<float4*>(s1 + i0);
      gg = *reinterpret_cast<const float4*>(g + i0);
      if (kTwo) vv = *reinterpret_cast<float4*>(s2 + i0);
    }
    sync_lr();
    if (have) {
      four<R>(pp, gg, mm, vv, lr_t, a);
      if (kTwo) *reinterpret_cast<float4*>(s2 + i0) = vv;
      *reinterpret_cast<float4*>(p + i0) = pp; *reinterpret_cast<float4*>(s1 + i0) = mm;
      nv[0] = pp.x; nv[1] = pp.y; nv[2] = pp.z; nv[3] = pp.w;
    }
    // rm [taps][A][B8]: the row's run of four (pad columns b in [B, B8) are zeros)
    if (ar < A && bq < B8)
      *reinterpret_cast<acg::bf16x4*>(l.rm[e] + ((long long)tap * A + ar) * B8 + bq) = acg::bf16x4{(__bf16)nv[0], (__bf16)nv[1], (__bf16)nv[2], (__bf16)nv[3]};
#pragma unroll
    for (int u = 0; u < 4; ++u) tile[r][4 * q + u] = nv[u];
  } else {
    // rows at any 4-byte offset (266 gathered channels, 1 or 5 output channels): thread -> (a = a0 + t / 32 + 8u, b = b0 + t % 32),
    // a wave instruction = two rows of 32 consecutive floats
    const int bl = threadIdx.x & 31, bb = b0 + bl;
    sync_lr();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int al = (threadIdx.x >> 5) + 8 * u, aa = a0 + al;
      float v = 0.f;
      if (aa < A && bb < B) v = upd(l.off[e] + ((long long)tap * A + aa) * B + bb);
      if (aa < A && bb < B8) l.rm[e][((long long)tap * A + aa) * B8 + bb] = (__bf16)v;
      tile[al][bl] = v;
    }
  }
  __syncthreads();
  // tr [taps][B][A8]: thread -> (b = b0 + r, a run 4q .. 4q + 3); pad rows a in [A, A8) come out as the zeros of invalid elements
  const int bt = b0 + r, at = a0 + 4 * q;
  if (bt < B && at < A8)
    *reinterpret_cast<acg::bf16x4*>(l.tr[e] + ((long long)tap * B + bt) * A8 + at) =
        acg::bf16x4{(__bf16)tile[4 * q][r], (__bf16)tile[4 * q + 1][r], (__bf16)tile[4 * q + 2][r], (__bf16)tile[4 * q + 3][r]};
}

// The four flat entries: one argument check, one launch.  `e`: the weight average the launch carries, or null.
struct EmaArgs {
  float* shadow;
  float decay;
  int64_t* num_updates;
  uint32_t* state;
};

// `lr`: the schedule the launch evaluates (the *_step_lr entries), or null.
int32_t flat_step(const char* who, bool adam, float* p, const float* g, float* s1, float* s2, const int32_t* step, int64_t n,
                  const OptScalars& a, const EmaArgs* e, acg_stream_t stream, const LrArgs* lr = nullptr) {
  ACG_REQUIRE(n > 0 && p && g && s1 && (!adam || (s2 && step)), ACG_ERR_INVALID_ARG, "%s: bad argument", who);
  if (e) {
    ACG_REQUIRE(e->shadow && e->num_updates && e->state, ACG_ERR_INVALID_ARG, "%s: null shadow / counter / state word", who);
    ACG_REQUIRE(e->decay > 0.f && e->decay < 1.f, ACG_ERR_INVALID_ARG, "%s: decay %g is not in (0, 1)", who, (double)e->decay);
    ACG_REQUIRE((reinterpret_cast<uintptr_t>(e->num_updates) & 7) == 0 && (reinterpret_cast<uintptr_t>(e->state) & 3) == 0,
                ACG_ERR_INVALID_ARG, "%s: the counter must be 8-byte and the state word 4-byte aligned", who);
  }
  // A scheduled launch retires its update counter with one atomic per block, all on one word, and they drain one after the other
  // once the streaming is over: ~9 ns each, 26 us behind the 13 us update of config 2's generator at the plain kernels' 2804
  // blocks (measured, profiles/lr_schedule/).  So it runs at most kLrGrid blocks - one per compute unit - and lets the
  // grid-stride loop do the rest: ~4 us over adam_k there.  The plain and the _ema launches keep the grid they have.
  constexpr int kLrGrid = 256;
  const dim3 grid(lr ? std::min(acg::grid_for(n / 4 + 1), kLrGrid) : acg::grid_for(n / 4 + 1)), block(256);
  hipStream_t st = acg::to_stream(stream);
  long long* count = e ? reinterpret_cast<long long*>(e->num_updates) : nullptr;
  unsigned* done = e ? reinterpret_cast<unsigned*>(e->state) : nullptr;
  if (lr) {
    float* sh = e ? e->shadow : nullptr;
    const float decay = e ? e->decay : 0.f;
    const int* st_dev = reinterpret_cast<const int*>(step);
    if (adam && e) ACG_LAUNCH((step_lr_k<Adam, true>), grid, block, 0, st, p, g, s1, s2, st_dev, (long long)n, a, *lr, sh, decay, count, done);
    else if (adam) ACG_LAUNCH((step_lr_k<Adam, false>), grid, block, 0, st, p, g, s1, s2, st_dev, (long long)n, a, *lr, sh, decay, count, done);
    else if (e) ACG_LAUNCH((step_lr_k<RmsProp, true>), grid, block, 0, st, p, g, s1, s2, st_dev, (long long)n, a, *lr, sh, decay, count, done);
    else ACG_LAUNCH((step_lr_k<RmsProp, false>), grid, block, 0, st, p, g, s1, s2, st_dev, (long long)n, a, *lr, sh, decay, count, done);
    return acg::check_launch(who);
  }
  if (adam && e)
    ACG_LAUNCH(adam_ema_k, grid, block, 0, st, p, g, s1, s2, step, (long long)n, a.lr, a.b1, a.b2, a.eps, a.gs, a.use_clip, a.lo, a.hi,
               e->shadow, e->decay, count, done);
  else if (adam)
    ACG_LAUNCH(adam_k, grid, block, 0, st, p, g, s1, s2, step, (long long)n, a.lr, a.b1, a.b2, a.eps, a.gs, a.use_clip, a.lo, a.hi);
  else if (e)
    ACG_LAUNCH(rmsprop_ema_k, grid, block, 0, st, p, g, s1, (long long)n, a.lr, a.b1, a.eps, a.gs, a.use_clip, a.lo, a.hi, e->shadow,
               e->decay, count, done);
  else
    ACG_LAUNCH(rmsprop_k, grid, block, 0, st, p, g, s1, (long long)n, a.lr, a.b1, a.eps, a.gs, a.use_clip, a.lo, a.hi);
  return acg::check_launch(who);
}

// The two scheduled entries: the schedule's own argument check, then flat_step with it (and with the average when `shadow` is
// not null).
int32_t flat_step_lr(const char* who, bool adam, float* p, const float* g, float* s1, float* s2, const int32_t* step, int64_t n,
                     const OptScalars& a, const acg_lr_schedule* sched, int64_t* lr_updates, uint32_t* lr_state, float* lr_out,
                     const EmaArgs& e, acg_stream_t stream) {
  ACG_REQUIRE(sched && lr_updates && lr_state && lr_out, ACG_ERR_INVALID_ARG, "%s: null schedule / update counter / state word / lr_out", who);
  ACG_REQUIRE((reinterpret_cast<uintptr_t>(lr_updates) & 7) == 0 && (reinterpret_cast<uintptr_t>(lr_state) & 3) == 0 &&
              (reinterpret_cast<uintptr_t>(lr_out) & 3) == 0, ACG_ERR_INVALID_ARG,
              "%s: the update counter must be 8-byte, its state word and lr_out 4-byte aligned", who);
  ACG_REQUIRE(a.lr > 0.f && a.lr <= 3.402823466e38f, ACG_ERR_INVALID_ARG, "%s: lr %g is not finite and > 0", who, (double)a.lr);
  ACG_REQUIRE(sched->kind >= ACG_LR_CONSTANT && sched->kind <= ACG_LR_EXPONENTIAL, ACG_ERR_INVALID_ARG,
              "%s: schedule kind %d (0 constant, 1 linear, 2 cosine, 3 exponential)", who, sched->kind);
  ACG_REQUIRE(sched->warmup >= 0, ACG_ERR_INVALID_ARG, "%s: warmup %lld < 0", who, (long long)sched->warmup);
  if (sched->kind != ACG_LR_CONSTANT) {
    const float F = sched->final_factor;
    ACG_REQUIRE(sched->decay_steps >= 1, ACG_ERR_INVALID_ARG, "%s: decay_steps %lld < 1", who, (long long)sched->decay_steps);
    ACG_REQUIRE(F <= 1.f && (sched->kind == ACG_LR_EXPONENTIAL ? F > 0.f : F >= 0.f), ACG_ERR_INVALID_ARG,
                "%s: final_factor %g is not in %s", who, (double)F, sched->kind == ACG_LR_EXPONENTIAL ? "(0, 1]" : "[0, 1]");
  }
  if (e.shadow)
    ACG_REQUIRE(lr_updates != e.num_updates && static_cast<void*>(lr_state) != static_cast<void*>(e.state), ACG_ERR_INVALID_ARG,
                "%s: the schedule and the average share a counter or a state word", who);
  const LrArgs lr{sched->kind, (long long)sched->warmup, (long long)sched->decay_steps, sched->final_factor,
                  reinterpret_cast<long long*>(lr_updates), reinterpret_cast<unsigned*>(lr_state), lr_out};
  return flat_step(who, adam, p, g, s1, s2, step, n, a, e.shadow ? &e : nullptr, stream, &lr);
}

}  // namespace

extern "C" {

int32_t acg_adam_step(float* param, const float* grad, float* m, float* v, const int32_t* step_dev, int64_t n, float lr,
                      float beta1, float beta2, float eps, float grad_scale, int32_t use_clip, float clip_lo, float clip_hi,
                      acg_stream_t stream) {
  return flat_step("adam_step", true, param, grad, m, v, step_dev, n, {lr, beta1, beta2, eps, grad_scale, clip_lo, clip_hi, use_clip},
                   nullptr, stream);
}

int32_t acg_rmsprop_step(float* param, const float* grad, float* ms, int64_t n, float lr, float decay, float eps,
                         float grad_scale, int32_t use_clip, float clip_lo, float clip_hi, acg_stream_t stream) {
  return flat_step("rmsprop_step", false, param, grad, ms, nullptr, nullptr, n, {lr, decay, 0.f, eps, grad_scale, clip_lo, clip_hi, use_clip},
                   nullptr, stream);
}

int32_t acg_adam_step_ema(float* param, const float* grad, float* m, float* v, const int32_t* step_dev, int64_t n, float lr,
                          float beta1, float beta2, float eps, float grad_scale, int32_t use_clip, float clip_lo, float clip_hi,
                          float* shadow, float ema_decay, int64_t* num_updates, uint32_t* state, acg_stream_t stream) {
  const EmaArgs e{shadow, ema_decay, num_updates, state};
  return flat_step("adam_step_ema", true, param, grad, m, v, step_dev, n, {lr, beta1, beta2, eps, grad_scale, clip_lo, clip_hi, use_clip},
                   &e, stream);
}

int32_t acg_rmsprop_step_ema(float* param, const float* grad, float* ms, int64_t n, float lr, float decay, float eps,
                             float grad_scale, int32_t use_clip, float clip_lo, float clip_hi, float* shadow, float ema_decay,
                             int64_t* num_updates, uint32_t* state, acg_stream_t stream) {
  const EmaArgs e{shadow, ema_decay, num_updates, state};
  return flat_step("rmsprop_step_ema", false, param, grad, ms, nullptr, nullptr, n,
                   {lr, decay, 0.f, eps, grad_scale, clip_lo, clip_hi, use_clip}, &e, stream);
}

int32_t acg_adam_step_lr(float* param, const float* grad, float* m, float* v, const int32_t* step_dev, int64_t n, float lr,
                         float beta1, float beta2, float eps, float grad_scale, int32_t use_clip, float clip_lo, float clip_hi,
                         const acg_lr_schedule* sched, int64_t* lr_updates, uint32_t* lr_state, float* lr_out, float* shadow,
                         float ema_decay, int64_t* num_updates, uint32_t* state, acg_stream_t stream) {
  return flat_step_lr("adam_step_lr", true, param, grad, m, v, step_dev, n, {lr, beta1, beta2, eps, grad_scale, clip_lo, clip_hi, use_clip},
                      sched, lr_updates, lr_state, lr_out, EmaArgs{shadow, ema_decay, num_updates, state}, stream);
}

int32_t acg_rmsprop_step_lr(float* param, const float* grad, float* ms, int64_t n, float lr, float decay, float eps,
                            float grad_scale, int32_t use_clip, float clip_lo, float clip_hi, const acg_lr_schedule* sched,
                            int64_t* lr_updates, uint32_t* lr_state, float* lr_out, float* shadow, float ema_decay,
                            int64_t* num_updates, uint32_t* state, acg_stream_t stream) {
  return flat_step_lr("rmsprop_step_lr", false, param, grad, ms, nullptr, nullptr, n,
                      {lr, decay, 0.f, eps, grad_scale, clip_lo, clip_hi, use_clip}, sched, lr_updates, lr_state, lr_out,
                      EmaArgs{shadow, ema_decay, num_updates, state}, stream);
}

int32_t acg_clip(float* param, int64_t n, float lo, float hi, acg_stream_t stream) {
  ACG_REQUIRE(n > 0 && param, ACG_ERR_INVALID_ARG, "clip: bad argument");
  ACG_LAUNCH(clip_k, dim3(acg::grid_for(n)), dim3(256), 0, acg::to_stream(stream), param, (long long)n, lo, hi);
  return acg::check_launch("clip");
}

int32_t acg_opt_step_prepare_bf16(float* param, const float* grad, float* slot1, float* slot2, const int32_t* step_dev, int64_t n,
                                  const acg_opt_args* args, const acg_prep_list* list, int32_t count, acg_stream_t stream) {
  ACG_REQUIRE(n > 0 && param && grad && slot1 && args && list, ACG_ERR_INVALID_ARG, "opt_step_prepare_bf16: null pointer / n <= 0");
  ACG_REQUIRE(count >= 1 && count <= ACG_PREP_MAX, ACG_ERR_INVALID_ARG, "opt_step_prepare_bf16: 1..%d filters", ACG_PREP_MAX);
  ACG_REQUIRE(args->kind == 0 || args->kind == 1, ACG_ERR_INVALID_ARG, "opt_step_prepare_bf16: kind %d (0 = Adam, 1 = RMSProp)", args->kind);
  ACG_REQUIRE(args->kind == 1 || (slot2 && step_dev), ACG_ERR_INVALID_ARG, "opt_step_prepare_bf16: Adam needs slot2 and the step counter");
  ACG_REQUIRE((reinterpret_cast<uintptr_t>(param) & 15) == 0 && (reinterpret_cast<uintptr_t>(grad) & 15) == 0 && (reinterpret_cast<uintptr_t>(slot1) & 15) == 0 &&
              (reinterpret_cast<uintptr_t>(slot2) & 15) == 0, ACG_ERR_INVALID_ARG, "opt_step_prepare_bf16: flat buffers must be 16-byte aligned");
  // the filters, in the order they lie in the flat buffer; what is left between them are the gaps
  int order[ACG_PREP_MAX];
  for (int i = 0; i < count; ++i) order[i] = i;
  std::sort(order, order + count, [&](int x, int y) { return list->src[x] < list->src[y]; });
  OptPrepList l;
  long long cursor = 0, blocks = 0;
  int ngaps = 0;
  for (int k = 0; k < count; ++k) {
    const int i = order[k];
    ACG_REQUIRE(list->src[i] && list->rm[i] && list->tr[i] && list->taps[i] > 0 && list->a[i] > 0 && list->b[i] > 0, ACG_ERR_INVALID_ARG,
                "opt_step_prepare_bf16: bad filter entry %d", i);
    const long long off = (const float*)list->src[i] - param, numel = (long long)list->taps[i] * list->a[i] * list->b[i];
    ACG_REQUIRE(off >= cursor && off + numel <= n && (off & 3) == 0, ACG_ERR_INVALID_ARG,
                "opt_step_prepare_bf16: filter %d does not lie inside the flat buffer (16-byte aligned, no overlap)", i);
    if (off > cursor) { l.gap_lo[ngaps] = cursor; l.gap_len[ngaps] = off - cursor; ++ngaps; }
    cursor = off + numel;
    l.off[k] = off; l.rm[k] = (__bf16*)list->rm[i]; l.tr[k] = (__bf16*)list->tr[i];
    l.taps[k] = list->taps[i]; l.A[k] = list->a[i]; l.B[k] = list->b[i];
    l.first_block[k] = (int)blocks;
    const int A8 = (list->a[i] + 7) & ~7, B8 = (list->b[i] + 7) & ~7;
    blocks += (long long)list->taps[i] * ((A8 + 31) / 32) * ((B8 + 31) / 32);
    ACG_REQUIRE(blocks < (1ll << 30), ACG_ERR_UNSUPPORTED, "opt_step_prepare_bf16: too many tiles");
  }
  if (n > cursor) { l.gap_lo[ngaps] = cursor; l.gap_len[ngaps] = n - cursor; ++ngaps; }
  l.first_block[count] = (int)blocks;
  const OptScalars a{args->lr, args->beta1_or_decay, args->beta2, args->eps, args->grad_scale, args->clip_lo, args->clip_hi, args->use_clip};
  hipStream_t st = acg::to_stream(stream);
  if (args->kind == 0) ACG_LAUNCH((opt_prepare_k<Adam>), dim3((unsigned)(blocks + ngaps)), dim3(256), 0, st, param, grad, slot1, slot2, (const int*)step_dev, a, l, (int)count);
  else ACG_LAUNCH((opt_prepare_k<RmsProp>), dim3((unsigned)(blocks + ngaps)), dim3(256), 0, st, param, grad, slot1, slot2, (const int*)step_dev, a, l, (int)count);
  return acg::check_launch("opt_step_prepare_bf16");
}

int32_t acg_step_inc(int32_t* step_dev, acg_stream_t stream) {
  ACG_REQUIRE(step_dev, ACG_ERR_INVALID_ARG, "step_inc: null counter");
  ACG_LAUNCH(step_inc_k, dim3(1), dim3(1), 0, acg::to_stream(stream), step_dev);
  return acg::check_launch("step_inc");
}

}  // extern "C"
