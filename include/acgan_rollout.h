/*
 * acgan_rollout.h - the two gradients that training through the generator's own K-step rollouts needs and the one-step
 * trainer never did: the DNA tail's gradient with respect to its image input (the image of step j >= 1 is the frame the
 * generator predicted at step j - 1) and the gradient of a tiled action vector (from step 1 on, the state half of the
 * vector is the state the generator predicted).
 *
 * An addition under ACG_ABI_VERSION 8: it changes no signature of acgan_hip.h, whose conventions it follows - device
 * pointers are borrowed (NHWC, float32), calls are asynchronous on `stream`, return ACG_OK or an ACG_ERR_* code with the
 * message in acg_last_error().  Neither entry uses atomics: the same call gives the same bits.  The Python binding keeps
 * these entries in a table of their own (_lib.ROLLOUT_SIGNATURES): the C oracle does not implement them.
 *
 * Back-propagation through K generator passes is the textbook case for exploding gradients, so the header also holds what bounds
 * them: acg_grad_clip_norm, the global-norm clip (and the norm measurement) of an optimizer's flat gradient buffer, with its
 * workspace query - same conventions, same table, no atomics either.
 *
 * The action vector on the device is this header's, so the generator's noise input - a latent drawn on the device and appended
 * to that vector, the last entry below - is declared here as well: same conventions, same table, no atomics.
 *
 * acg_grad_clip_norm is "what sits in front of the optimizer update", and so is the learning rate: the two optimizer steps whose
 * rate follows a schedule evaluated INSIDE their launch, from an update counter on the device that the launch advances itself
 * (acg_adam_step_lr / acg_rmsprop_step_lr, at the end of this header).  A rate passed by value is frozen into a captured graph of
 * the step; this one changes with every replay and no host in the loop.  Same conventions, same table; the only atomics are
 * those of the counter advance, which is the weight average's (include/acgan_ema.h).
 *
 * Scheduled sampling for the K-step rollout - the coins, drawn on the device by the noise input's generator from a state of their
 * own, the per-sample select between the true and the predicted frame and state, and its adjoint - closes the header: same
 * conventions, same table, no atomics.
 *
 * And what the action-conditioned rollout is for - choosing the actions that lead to a wanted frame - ends it: the three launches
 * of a cross-entropy-method planner around the generator forwards (acg_plan_sample / acg_plan_cost / acg_plan_refit), the draw by
 * the same generator from a state of its own.  Same conventions, same table, no atomics.  acg_plan_pixel_cost, the last entry,
 * is the planner's second cost: the expected distance of designated pixels' probability maps to their goal positions.
 *
 * The fourth draw of that generator is the one on the other network: instance noise on every frame the discriminator judges
 * (acg_inst_noise_prepare / acg_inst_noise_add), and, to choose its level by, the statistics of D's logits (acg_logit_stats).
 * Same conventions, same table, no atomics.
 *
 * The noise input's learned posterior (the VAE half of a VAE-GAN; SV2P, Babaeizadeh et al. 2018; SAVP, Lee et al. 2018) is the
 * last pair: acg_latent_fwd, acg_noise_concat's draw reparameterised as z = mu + exp(logvar / 2) * eps with
 * KL(N(mu, exp(logvar)) || N(0, 1)) summed in the same launch, and acg_latent_bwd, the one launch that carries the gradient of
 * both back into (mu, logvar).  They read acg_noise_concat's state and its limits, which is why they are declared here and not in
 * a header of their own.  Same conventions, same table, no atomics.
 */
#ifndef ACGAN_ROLLOUT_H
#define ACGAN_ROLLOUT_H

#include "acgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The exact adjoint of acg_dna_fwd with respect to its image (p = (k-1)/2, zero outside the image):
 *   g[b,y',x',c]  = dout[b,y',x',c] (+ dout2[b,y',x', dout2_offset + c] when dout2 is not NULL; pixels dout2_pitch apart,
 *                   storage dout2_dtype = ACG_F32 or ACG_BF16 - the frame's channels of d(discriminator input), as
 *                   acg_dna_bwd reads them);
 *   w[b,y',x',:]  = softmax(logits[b,y',x',:] + bias)       (bias float32 [k*k], may be NULL);
 *   dimage[b,y,x,c] = (accumulate != 0 ? accumulate * dimage[b,y,x,c] : 0)
 *                     + sum_{i,j} w[b,y',x'][i*k+j] * g[b,y',x',c],   y' = y+p-i, x' = x+p-j, over in-range (y', x').
 * A gather: every output element is written by one thread, no atomics.  logits [B,H,W,k*k] dense float32 (dtype ACG_F32);
 * dout and dimage [B,H,W,C] float32; 1 <= k <= 11, 1 <= C <= 4.  One launch. */
int32_t acg_dna_bwd_image(const void* logits, const float* bias, const float* dout, const void* dout2, int32_t dout2_pitch,
                          int32_t dout2_offset, int32_t dout2_dtype, float* dimage, float accumulate, int32_t batch, int32_t h,
                          int32_t w, int32_t c, int32_t ksize, int32_t dtype, acg_stream_t stream);

/* Gradient of a tiled action vector: the rows of dcat (float32, pixels `pitch` elements apart) took their action channels
 * [c_off, c_off + n) from row (r / div) % mod of a [mod, n] vector - the (div, mod) mapping of the host's feed copy
 * (tf.tile over an h x w map is div = h*w; one vector shared by the halves of a joined batch is mod = B) - so
 *   dact[q, a] = (accumulate != 0 ? accumulate * dact[q, a] : 0) + sum over rows r < rows with (r / div) % mod == q of
 *                dcat[r * pitch + c_off + a].
 * One block per q sums in a fixed order (no atomics).  dact is dense [mod, n]. */
int32_t acg_action_grad(const float* dcat, int64_t rows, int32_t pitch, int32_t c_off, int32_t n, int32_t div, int32_t mod,
                        float* dact, float accumulate, acg_stream_t stream);

/* Clip by global norm (tf.clip_by_global_norm) over the variables' windows of a flat float32 gradient buffer of n elements.
 * `segs` (read on the host during the call and copied into the kernel arguments: nothing of it is referenced afterwards, a
 * captured graph replays the call) lists 1..ACG_NORM_SEGMENTS_MAX windows [offset, offset + length) in elements: offsets are
 * multiples of 4 (16 bytes), lengths >= 1, inside [0, n), pairwise disjoint, in any order; `grad` is 16-byte aligned.
 *   ss_i   = sum of the squares of segment i, every square and every sum in double, in an order that depends on (n, segs) only:
 *            per ACG_NORM_CHUNK elements of a segment one partial (a double in `workspace`), the partials of a segment summed in
 *            a fixed order by one block, the segments in list order;
 *   norm_i = |pre_scale| * sqrt(ss_i),   norm = |pre_scale| * sqrt(sum_i ss_i);
 *   scale  = (float)(max_norm / norm) if norm is finite and norm > max_norm, else 1;
 *   grad[e] *= scale (one float32 multiply) for every element of every segment - only when scale != 1: a gradient that fits,
 *            a gradient with a NaN or an infinity in it, and max_norm = +inf (measure only) leave the buffer unwritten.  A
 *            non-finite gradient is passed on as it is and stats[0] says so.
 *   stats[0] = (float)norm, stats[1] = scale, stats[2 + i] = (float)norm_i          (device, float32 [2 + count]).
 * Elements between the segments (alignment gaps) are neither read nor written.  max_norm > 0 (+inf allowed), pre_scale finite:
 * with pre_scale = the optimizer's grad_scale, what the optimizer then sees is clip_by_global_norm of the averaged gradient.
 * Three launches (two for max_norm = +inf); workspace: acg_grad_clip_norm_workspace_bytes(n, segs) bytes, 8-byte aligned, its
 * content on entry is irrelevant (0 is returned for an invalid (n, segs); the call itself then reports the error). */
#define ACG_NORM_SEGMENTS_MAX 64
#define ACG_NORM_CHUNK 8192
typedef struct acg_norm_segments {
  int32_t count;
  int64_t offset[ACG_NORM_SEGMENTS_MAX];
  int64_t length[ACG_NORM_SEGMENTS_MAX];
} acg_norm_segments;
size_t acg_grad_clip_norm_workspace_bytes(int64_t n, const acg_norm_segments* segs);
int32_t acg_grad_clip_norm(float* grad, int64_t n, const acg_norm_segments* segs, float pre_scale, float max_norm, float* stats,
                           void* workspace, size_t workspace_bytes, acg_stream_t stream);

/* The generator's noise input.  This header owns the device-side action vector, so the latent that is appended to it lives here:
 *   out[b, :A]    = actions[b, :]                    (bit for bit),
 *   out[b, A + j] = scale[0] * z[b * Z + j]          (exactly 0 when scale[0] == 0),
 * actions [B, A], out [B, A + Z] dense float32, scale float32 [1] and state uint64 [2] = {seed, counter} in device memory, all
 * distinct.  z is a pure function of (seed, counter, stream_id, element index e): Philox4x32-10 on block i = e / 4 with the counter
 * words (lo32(counter), hi32(counter), i, stream_id) and the key (lo32(seed), hi32(seed)) - multipliers 0xD2511F53 / 0xCD9E8D57,
 * Weyl constants 0x9E3779B9 / 0xBB67AE85; each output word x gives u = ((x >> 9) + 0.5) * 2^-23 in (0, 1); Box-Muller on the pairs
 * (u0, u1), (u2, u3): r = sqrt(-2 ln u_even), z = r cos(2 pi u_odd), r sin(2 pi u_odd) in full float32 precision, |z| <= 5.77;
 * element e is lane e % 4 of block e / 4 and the tail of the last block is dropped.  After the draw the kernel stores
 * counter + 1 (also when scale[0] == 0): the same call draws fresh values each time it runs, a replayed graph included, with no
 * host in the loop.  stream_id separates concurrent streams of one seed (the data-parallel rank).  One launch of one block, no
 * atomics; 1 <= A, Z <= ACG_NOISE_DIM_MAX and B * Z <= ACG_NOISE_VALUES_MAX.  Calls that share a state must be stream-ordered. */
#define ACG_NOISE_DIM_MAX 64
#define ACG_NOISE_VALUES_MAX 8192
int32_t acg_noise_concat(const float* actions, uint64_t* state, const float* scale, float* out, int32_t batch, int32_t action_dim,
                         int32_t noise_dim, int32_t stream_id, acg_stream_t stream);

/* Optimizer steps with a learning-rate schedule.  acg_adam_step / acg_rmsprop_step (acgan_hip.h) with the base rate `lr` replaced
 * by lr_k, the schedule's rate at k = lr_updates[0] as the launch finds it; with `shadow` not NULL the launch also carries the
 * weight average, exactly as acg_adam_step_ema / acg_rmsprop_step_ema do (acgan_ema.h; shadow NULL: no average, ema_decay,
 * num_updates and state are ignored).  With F = (double)final_factor, everything in double:
 *   w = (warmup > 0 && k < warmup) ? (k + 1) / warmup : 1
 *   j = max(k - warmup, 0),   t = min(j / decay_steps, 1)
 *   ACG_LR_CONSTANT:     f = 1                                          (decay_steps and final_factor are not read)
 *   ACG_LR_LINEAR:       f = 1 - (1 - F) * t
 *   ACG_LR_COSINE:       f = F + (1 - F) * 0.5 * (1 + cos(pi * t))
 *   ACG_LR_EXPONENTIAL:  f = pow(F, j / decay_steps)                    (not clamped: tf.train.exponential_decay, no staircase)
 *   lr_k = (float)((double)lr * w * f)
 * and Adam's bias-corrected rate is (float)((double)lr_k * sqrt(1 - beta2^t) / (1 - beta1^t)) with its own step counter t, as
 * before.  Given the same rate the update is that of the plain entries bit for bit: parameters, slots and shadow come out as
 * acg_adam_step / acg_rmsprop_step (or their _ema forms) called with lr = lr_k leave them.
 * `sched` is read on the host during the call and copied into the kernel arguments: nothing of it is referenced afterwards, a
 * captured graph replays the call.  One launch: one thread of every block reads the counter and evaluates lr_k (every block the
 * same value), block 0 stores lr_out[0] = lr_k, and the last block to retire stores lr_updates[0] = k + 1 and resets lr_state[0]
 * - the rule of the average's counter (acgan_ema.h), each counter with a state word of its own: one state word belongs to one
 * counter.  lr_updates int64 [1] (8-byte aligned), lr_state uint32 [1] (0 before the first launch), lr_out float32 [1], all in
 * device memory and distinct from the average's.  Calls that share a counter must be stream-ordered.
 * Checked on the host before anything is launched: sched, lr_updates, lr_state, lr_out not NULL and aligned; lr finite and > 0;
 * kind one of the four; warmup >= 0; for every kind but constant decay_steps >= 1 and 0 <= final_factor <= 1 (exponential:
 * 0 < final_factor <= 1); the average's arguments as in acgan_ema.h. */
#define ACG_LR_CONSTANT 0
#define ACG_LR_LINEAR 1
#define ACG_LR_COSINE 2
#define ACG_LR_EXPONENTIAL 3
typedef struct acg_lr_schedule {
  int32_t kind;
  int64_t warmup;
  int64_t decay_steps;
  float final_factor;
} acg_lr_schedule;
int32_t acg_adam_step_lr(float* param, const float* grad, float* m, float* v, const int32_t* step_dev, int64_t n, float lr,
                         float beta1, float beta2, float eps, float grad_scale, int32_t use_clip, float clip_lo, float clip_hi,
                         const acg_lr_schedule* sched, int64_t* lr_updates, uint32_t* lr_state, float* lr_out, float* shadow,
                         float ema_decay, int64_t* num_updates, uint32_t* state, acg_stream_t stream);
int32_t acg_rmsprop_step_lr(float* param, const float* grad, float* ms, int64_t n, float lr, float decay, float eps,
                            float grad_scale, int32_t use_clip, float clip_lo, float clip_hi, const acg_lr_schedule* sched,
                            int64_t* lr_updates, uint32_t* lr_state, float* lr_out, float* shadow, float ema_decay,
                            int64_t* num_updates, uint32_t* state, acg_stream_t stream);

/* Scheduled sampling (Bengio et al. 2015) for the K-step rollout: at every fed-back position a coin per sample decides whether the
 * next step reads the true frame and state or the ones the generator predicted; the probability of truth follows a schedule over
 * the K-step updates.  Three entries - the coins, the row select, its adjoint - with this header's conventions; none uses atomics:
 * the same call on the same state gives the same bits.
 *
 * acg_sched_sample_draw: the coins of all `steps` fed-back positions of one program.  state uint64 [2] = {seed, counter} in device
 * memory (a state of its own, laid out as the noise state above).  With k = counter as the launch finds it, j = max(k - offset, 0)
 * and S = start, F = final, everything in double and every operation rounded on its own:
 *   ACG_SS_CONSTANT:         p = S                                              (offset, decay_steps and final are not read)
 *   ACG_SS_LINEAR:           p = S + (F - S) * min(j / decay_steps, 1)
 *   ACG_SS_INVERSE_SIGMOID:  p = F + (S - F) * (d / (d + exp(j / d))),  d = decay_steps   (Bengio's eps_i = k / (k + exp(i / k)))
 *   prob_out[0] = (float)p                                                      (device, float32 [1]).
 * The coin of element e = s * batch + b (step slot s in [0, steps), sample b) is lane e % 4 of Philox4x32-10 block e / 4 with the
 * counter words (lo32(k), hi32(k), e / 4, stream_id ^ ACG_SS_STREAM_TAG) and the key (lo32(seed), hi32(seed)) - the generator and
 * the uniform u = ((x >> 9) + 0.5) * 2^-23 of acg_noise_concat; the tag keeps this stream apart from the noise stream of the same
 * seed and stream id - and
 *   mask[e] = u < prob_out[0] ? 1.f : 0.f          (1: read the truth; mask float32 [steps, batch]).
 * u lies strictly inside (0, 1): p = 0 gives all zeros and p = 1 all ones, exactly.  After the draw the kernel stores counter + 1:
 * a replayed graph draws fresh coins and moves along the schedule with no host in the loop.  One launch of one block.  `sched` is
 * read on the host during the call and copied into the kernel arguments.  Checked on the host before anything is launched:
 * pointers not NULL; kind one of the three; 0 <= start, final <= 1; offset >= 0; decay_steps >= 1 for every kind but constant;
 * 1 <= steps * batch <= ACG_NOISE_VALUES_MAX.  Calls that share a state must be stream-ordered. */
#define ACG_SS_CONSTANT 0
#define ACG_SS_LINEAR 1
#define ACG_SS_INVERSE_SIGMOID 2
#define ACG_SS_STREAM_TAG 0x5353414Du
typedef struct acg_ss_schedule {
  int32_t kind;
  int64_t offset;
  int64_t decay_steps;
  float start;
  float final;
} acg_ss_schedule;
int32_t acg_sched_sample_draw(uint64_t* state, const acg_ss_schedule* sched, float* mask, float* prob_out, int32_t steps,
                              int32_t batch, int32_t stream_id, acg_stream_t stream);

/* The row select: out[b, :] = mask[b] != 0 ? truth[b, :] : pred[b, :], a copy of bits, for the frame (rows of per_sample float32)
 * and the state (rows of state_dim float32) under the same coin; `mask` points at one step slot's [batch] row.  Either the frame
 * triple (pred, truth, out) or the state triple may be NULL as a whole, not both.  One launch: one sample per blockIdx.y, so only
 * the selected source of a row is read (the other may hold anything); 16-byte moves when per_sample % 4 == 0 and pred, truth and
 * out are 16-byte aligned, a scalar path otherwise.  out must not overlap the inputs.  1 <= batch <= 65535. */
int32_t acg_sched_sample_fwd(const float* mask, const float* pred, const float* truth, float* out, int64_t per_sample,
                             const float* pred_state, const float* true_state, float* out_state, int32_t state_dim, int32_t batch,
                             acg_stream_t stream);

/* Its adjoint with respect to the predicted inputs: dpred[b, :] = mask[b] != 0 ? +0.f : dout[b, :] (dout of a truth row is not
 * read), the same for the state pair; the pair (dout, dpred) or (dout_state, dpred_state) may be NULL as a whole, not both.  The
 * launch shape and the limits of acg_sched_sample_fwd. */
int32_t acg_sched_sample_bwd(const float* mask, const float* dout, float* dpred, int64_t per_sample, const float* dout_state,
                             float* dpred_state, int32_t state_dim, int32_t batch, acg_stream_t stream);

/* Planning with the generator by the cross-entropy method (CEM): draw N candidate action sequences of H steps from a diagonal
 * Gaussian, roll each through the generator, score the predicted frames (and states) against a goal, refit the Gaussian to the E
 * best, repeat.  The three entries are what runs around the generator forwards, so that the optimiser has no host in its loop: a
 * replayed graph of an iteration draws fresh candidates.  This header's conventions; no float atomics, every sum in a fixed order:
 * the same call on the same inputs gives the same bits.  1 <= N <= ACG_PLAN_CANDIDATES_MAX, 1 <= H <= ACG_PLAN_HORIZON_MAX,
 * 1 <= A <= ACG_PLAN_ACTION_DIM_MAX, 1 <= E <= N; a value below 1 or a null pointer is ACG_ERR_INVALID_ARG, one above its limit
 * ACG_ERR_UNSUPPORTED, and nothing is launched.
 *
 * acg_plan_sample: actions[n, t, a] = min(max(mean[t, a] + std[t, a] * z[n, t, a], lo[a]), hi[a])   (one fused multiply-add),
 * mean and std float32 [H * A], lo and hi float32 [A], actions float32 [N, H, A] dense.  With keep_mean != 0 row n = 0 is
 * min(max(mean, lo), hi) with no noise: the best guess so far is always a candidate.  z is the normal of acg_noise_concat - the
 * same Philox4x32-10, uniform and Box-Muller pairing - for the element e = (n * H + t) * A + a: lane e % 4 of block e / 4 with the
 * counter words (lo32(counter), hi32(counter), e / 4, stream_id ^ ACG_PLAN_STREAM_TAG) and the key (lo32(seed), hi32(seed)); the
 * tag keeps the candidates apart from the noise and the scheduled-sampling coins of the same seed and stream id.  state uint64 [2]
 * = {seed, counter} in device memory; after the draw the kernel stores counter + 1.  One launch of one block.  Calls that share a
 * state must be stream-ordered.
 *
 * acg_plan_cost: cost[n] = (accumulate != 0 ? cost[n] : 0) + frame_weight * sum_{y, x, ch < c} (frames[n, y, x, ch] - goal[y, x, ch])^2
 *                          + state_weight * sum_{s < state_dim} (states[n, s] - goal_state[s])^2.
 * frames [N, h, w, pitch], storage dtype = ACG_F32 or ACG_BF16, channels ch < c <= pitch <= 64 are scored (the pad channels may hold
 * anything); goal float32 [h, w, c] dense, one goal for all candidates; states float32 [N, state_dim] and goal_state float32
 * [state_dim] are both NULL (state_dim = 0) or both given (1 <= state_dim <= ACG_PLAN_STATE_DIM_MAX); cost float32 [N].  With
 * accumulate == 0 the old cost is not read: whatever the buffer held, a NaN included, is gone.  A weight of 0 multiplies its sum,
 * it does not skip it.  One launch, one block per candidate: per-thread float32 partials over a strided share of the frame, the
 * lanes of a wave summed by shuffles, the waves in order; no workspace.  16-byte loads (8-byte for bf16) when pitch == c and
 * h * w * c % 4 == 0, or pitch == 4, and the pointers are aligned; a scalar path otherwise.
 *
 * acg_plan_refit: with key(n) = cost[n], a NaN read as +inf, the rank of candidate n is the number of m with key(m) < key(n), or
 * key(m) == key(n) and m < n - a total, stable order: NaN and +inf come last, by index.  elite_idx[r] (int32 [E]) = the candidate
 * of rank r < E.  For every (t, a), over the elites in rank order, two sequential float32 passes: mean_e = sum / E,
 * std_e = sqrt(sum (x - mean_e)^2 / E) (population); then
 *   mean[t, a] = alpha * mean[t, a] + (1 - alpha) * mean_e,   std[t, a] = max(alpha * std[t, a] + (1 - alpha) * std_e, min_std),
 * and if key(elite_idx[0]) < best_cost[0] - strictly: an equal cost keeps the earlier plan - best_cost[0] and best_actions
 * [H * A] take that candidate's key and actions (the host starts best_cost at +inf; with every cost NaN both stay untouched).
 * history, when not NULL, receives best_cost[0] after the update (float32 [1]: the caller points it at its slot).  0 <= alpha <= 1,
 * min_std finite and >= 0.  One launch of one block of up to 1024 threads (one per candidate; the ranks are counted out of LDS). */
#define ACG_PLAN_CANDIDATES_MAX 1024
#define ACG_PLAN_HORIZON_MAX 16
#define ACG_PLAN_ACTION_DIM_MAX 8
#define ACG_PLAN_STATE_DIM_MAX 16
#define ACG_PLAN_STREAM_TAG 0x504C414Eu
int32_t acg_plan_sample(const float* mean, const float* std, const float* lo, const float* hi, uint64_t* state, float* actions,
                        int32_t candidates, int32_t horizon, int32_t action_dim, int32_t keep_mean, int32_t stream_id,
                        acg_stream_t stream);
int32_t acg_plan_cost(const void* frames, const float* goal, const float* states, const float* goal_state, float frame_weight,
                      float state_weight, float* cost, int32_t accumulate, int32_t candidates, int32_t h, int32_t w, int32_t c,
                      int32_t pitch, int32_t state_dim, int32_t dtype, acg_stream_t stream);
int32_t acg_plan_refit(const float* cost, const float* actions, float* mean, float* std, float* best_cost, float* best_actions,
                       int32_t* elite_idx, float* history, int32_t candidates, int32_t horizon, int32_t action_dim, int32_t elites,
                       float alpha, float min_std, acg_stream_t stream);

/* The designated-pixel cost of visual MPC (Finn & Levine, "Deep Visual Foresight"): the user marks d pixels and says where each
 * should end up; the generator moves a probability map of every marked pixel with the per-pixel kernels it predicts for the frame
 * (acg_dna_fwd on the map, c = d), and the cost of a candidate is the expected distance of each map to its goal position.
 * maps float32 [N, h, w, d] dense, READ AND REWRITTEN in place; goals float32 [d, 2] as (y, x), may be fractional, one goal set for
 * all candidates.  For every candidate n and map j < d, with P = maps[n, :, :, j] and (gy, gx) = goals[j]:
 *   m0 = sum_{y, x} P[y, x]                                  (the mass: the DNA gather does not conserve it)
 *   m1 = sum_{y, x} P[y, x] * sqrt((y - gy)^2 + (x - gx)^2)
 *   ey = sum_{y, x} P[y, x] * y,   ex = sum_{y, x} P[y, x] * x
 *   cost[n] = (accumulate != 0 ? cost[n] : 0) + pixel_weight * sum_j m1_j / m0_j       (accumulate == 0: the old value is not read)
 *   P <- P / m0                                              (the published model renormalises every step; a long rollout
 *                                                             stays inside float32 range)
 *   expected[n, j] = (ey / m0, ex / m0),   mass[n, j] = m0   (float32 [N, d, 2] and [N, d]; either may be NULL)
 * A map whose m0 is not finite or not > 0 makes what is added to cost[n] +inf - whatever pixel_weight is; acg_plan_refit ranks
 * +inf last - is left unscaled, and its expected entries are NaN (its mass is m0 as it came out).
 * One launch, one block per candidate, as acg_plan_cost: per-thread float32 partials over a strided share of the pixels, the lanes
 * of a wave summed by shuffles, the waves in order; no atomics, no workspace, the same call gives the same bits.  The second pass,
 * the scale, re-reads what the block just read.  1 <= N <= ACG_PLAN_CANDIDATES_MAX, 1 <= d <= ACG_PLAN_PIXEL_MAPS_MAX,
 * 1 <= h, w <= ACG_PLAN_MAP_SIDE_MAX, pixel_weight finite and >= 0; a NULL maps / goals / cost or a value below 1 is
 * ACG_ERR_INVALID_ARG, one above its limit ACG_ERR_UNSUPPORTED, and nothing is launched. */
#define ACG_PLAN_PIXEL_MAPS_MAX 4
#define ACG_PLAN_MAP_SIDE_MAX 1024
int32_t acg_plan_pixel_cost(float* maps, const float* goals, float pixel_weight, float* cost, int32_t accumulate, float* expected,
                            float* mass, int32_t candidates, int32_t h, int32_t w, int32_t d, acg_stream_t stream);

/* Instance noise (Sonderby et al. 2016; Arjovsky & Bottou 2017): Gaussian noise of a decaying level sigma on every frame the
 * discriminator judges, real and generated.  The draws above are one block each and advance their own counter; this one covers
 * every pixel of D's input, a multi-block launch that cannot, so the counter protocol is a launch of its own.
 *
 * acg_inst_noise_prepare: one launch of one block.  state uint64 [2] = {seed, counter} (laid out as the noise state above),
 * updates uint64 [1] = the schedule position, key_out uint64 [2], sigma_out float32 [1], all in device memory and distinct.  With
 * k = updates[0] as the launch finds it, j = max(k - offset, 0), S = sigma_start, F = sigma_final, everything in double and every
 * operation rounded on its own:
 *   sigma = S + (F - S) * min(j / decay_steps, 1)        (decay_steps == 0: sigma = S)
 *   sigma_out[0] = (float)sigma
 *   key_out[0..1] = {seed, counter} as found             (the snapshot acg_inst_noise_add reads)
 * and then state[1] = counter + 1 and, if advance_schedule != 0, updates[0] = k + 1: a replayed graph draws fresh noise and - where
 * it is the program that should - moves along the schedule with no host in the loop.  Checked on the host before anything is
 * launched: pointers not NULL; sigma_start and sigma_final finite and >= 0; offset >= 0; decay_steps >= 0.  Calls that share a
 * state must be stream-ordered.
 *
 * acg_inst_noise_add: in and out [pixels, pitch] of storage dtype = ACG_F32 or ACG_BF16, in != out (no overlap).  For a channel
 * ch in [c0, c0 + cn):  out[p, ch] = in[p, ch] + sigma[0] * z(p, ch - c0) - one fused multiply-add in float32, rounded once to
 * the storage type; every other channel ch < pitch, the pad channels [c, pitch) included, is a copy of bits.  z(p, l) is lane l
 * of Philox4x32-10 block p with the counter words (lo32(key[1]), hi32(key[1]), p, stream_id ^ ACG_DN_STREAM_TAG) and the key
 * (lo32(key[0]), hi32(key[0])), turned into normals as acg_noise_concat's are (the same uniform and Box-Muller pairing); the tag
 * keeps this stream apart from the other draws of the same seed and stream id.  sigma[0] == 0 copies every channel bit for bit
 * (-0.0 stays -0.0).  key uint64 [2] and sigma float32 [1] are read, never written: the result is a pure function of the
 * arguments - no atomics, no workspace, the same bits on every run.  One multi-block, grid-strided launch, one thread per pixel;
 * 16-byte accesses where pitch * element size is a multiple of 16 and both bases are 16-byte aligned, element accesses
 * otherwise, the same bits either way.  1 <= cn <= 4 (a Philox block has four lanes), c0 >= 0, c0 + cn <= c <= pitch,
 * 1 <= pixels < 2^32; a NULL pointer, in == out or a value outside these is ACG_ERR_INVALID_ARG (cn > 4, pixels >= 2^32 and an
 * unknown dtype: ACG_ERR_UNSUPPORTED) and nothing is launched.
 *
 * acg_logit_stats: out4 = {mean of fake, mean of real, share of fake[i] < 0, share of real[i] > 0} - the discriminator's mean
 * logits and its accuracy on either half - over fake and real float32 [n], n >= 1; sums in double in a fixed order (per-thread
 * partials over a strided share, the lanes of a wave by shuffles, the waves in order), each result rounded to float32 once.  One
 * launch of one block. */
#define ACG_DN_STREAM_TAG 0x444E4F49u
int32_t acg_inst_noise_prepare(uint64_t* state, uint64_t* updates, uint64_t* key_out, float* sigma_out, float sigma_start,
                               float sigma_final, int64_t offset, int64_t decay_steps, int32_t advance_schedule, acg_stream_t stream);
int32_t acg_inst_noise_add(const void* in, void* out, const uint64_t* key, const float* sigma, int64_t pixels, int32_t c, int32_t pitch,
                           int32_t c0, int32_t cn, int32_t dtype, int32_t stream_id, acg_stream_t stream);
int32_t acg_logit_stats(const float* fake, const float* real, int32_t n, float* out4, acg_stream_t stream);

/* The learned latent posterior of the noise input.  eps is the draw of acg_noise_concat above - the same Philox4x32-10 counter
 * words (lo32(counter), hi32(counter), block, stream_id) and key, uniform and Box-Muller pairing; element e = b * Z + j is lane
 * e % 4 of block e / 4 and the tail of the last block is dropped - and `state` uint64 [2] = {seed, counter} is the SAME state
 * acg_noise_concat reads (g/noise/state): the two entries draw one stream.  A refused call writes nothing.
 *
 * acg_latent_fwd: actions [B, A], stats [B, 2 Z] (stats[b, 0:Z] = mu, stats[b, Z:2Z] = logvar), out [B, A + Z], all dense float32; state
 * uint64 [2]; mode float32 [2] = {scale, posterior} in device memory (whoever runs the programs writes it between them);
 * kl float32 [1] or NULL.
 *   out[b, :A]    = actions[b, :]                                                      (bit for bit)
 *   posterior == 0:  out[b, A + j] = scale == 0 ? 0 : scale * eps                      (the prior: bit-identical to
 *                    acg_noise_concat given the same state, scale and stream id; stats is not read for out)
 *   posterior != 0:  out[b, A + j] = scale == 0 ? mu : fmaf(scale * expf(0.5f * logvar), eps, mu)
 *                    (scale == 0: the posterior mean, bit for bit, -0.0 included)
 *   kl[0] = (float)(0.5 * sum_{b, j} (mu^2 + exp(logvar) - logvar - 1))                (when kl is not NULL, in BOTH modes)
 * The KL terms are evaluated in double and summed in double in a fixed order (each thread its strided share in ascending order,
 * the lanes of a wave by shuffles, the waves in order) and the sum is rounded to float32 once: the same stats give the same bits
 * in every launch.  With kl == NULL and posterior == 0 stats is not read at all.
 * There is NO clamp on logvar: one large enough for expf to overflow gives z = +-inf (and a kl of inf), as the formula says;
 * whoever produces stats keeps them in range.
 * After the draw the kernel stores counter + 1 (in both modes, and when scale == 0): every thread has read the pair, a barrier,
 * thread 0 stores - no atomics, no workspace.  One launch of one block; 1 <= A, Z <= ACG_NOISE_DIM_MAX and
 * B * Z <= ACG_NOISE_VALUES_MAX.  Calls that share a state must be stream-ordered. */
int32_t acg_latent_fwd(const float* actions, const float* stats, uint64_t* state, const float* mode, float* out, float* kl,
                       int32_t batch, int32_t action_dim, int32_t latent_dim, int32_t stream_id, acg_stream_t stream);

/* acg_latent_bwd: the gradient of  L(out) + kl_weight * kl  with respect to stats, dout = dL/dout [B, A + Z] (NULL: zeros - the KL term alone).
 * With p = (mode[1] != 0), z = out[b, A + j] (read, never redrawn: no state is touched) and dz = dout[b, A + j]:
 *   dstats[b, j]     = p * dz                  + kl_weight * mu
 *   dstats[b, Z + j] = p * 0.5 * (z - mu) * dz + kl_weight * 0.5 * expm1f(logvar)
 * (sigma * eps = z - mu, so d z / d logvar = 0.5 * (z - mu)).  p == 0 leaves the z path out exactly and kl_weight == 0 the KL
 * path: with p != 0 and kl_weight == 0, dstats[b, j] is dz bit for bit.  dactions [B, A], when not NULL, is the copy of dout[:, :A] (zeros for
 * a NULL dout).  out, stats and mode are read only.  One launch of one block, plain vector stores, the limits of
 * acg_latent_fwd. */
int32_t acg_latent_bwd(const float* dout, const float* out, const float* stats, const float* mode, float kl_weight, float* dstats,
                       float* dactions, int32_t batch, int32_t action_dim, int32_t latent_dim, acg_stream_t stream);

/* Differentiable augmentation of the discriminator's inputs (DiffAugment, Zhao et al., NeurIPS 2020): every pair D judges, real
 * and generated, goes through a random colour / translation / cutout transform, and the generator's gradient goes back through
 * its adjoint.  x float32 [rows, h, w, pitch] holds `frames` frames of `cf` channels each at the channels [f * cf, (f + 1) * cf);
 * the channels [frames * cf, pitch) are pad.  params float32 [rows, 8], row r = (b, s, c, ty, tx, cy0, cx0, n): both frames of a
 * row get the same parameters, the rows of a launch independent ones.
 *
 * acg_d_augment_fwd.  Per frame of a row, with X[y, x, ch] its values:
 *   pm[y, x]      = mean over ch of X[y, x, .]          fm = mean over y, x, ch of X
 *   col[y, x, ch] = c * s * X[y, x, ch] + c * (1 - s) * pm[y, x] + (1 - c) * fm + b
 *     (brightness + b, then saturation about the pixel's channel mean by s, then contrast about the frame mean by c)
 *   out[y, x, ch] = 0                          if (y - ty, x - tx) is outside the image
 *                 = 0                          if cy0 <= y < cy0 + n and cx0 <= x < cx0 + n
 *                 = col[y - ty, x - tx, ch]    otherwise
 * and out[y, x, ch] for ch >= frames * cf is a copy of the bits of in[y, x, ch].  In float32: k1 = c * s, k2 = c * (1 - s),
 * out = fmaf(k1, X, fmaf(k2, pm, fmaf(1 - c, fm, b))), pm the channels summed in ascending order over cf, fm a sum in double
 * rounded to float32 once.  The identity (0, 1, 1, 0, 0, 0, 0, 0) therefore gives 1 * X + 0: the valid channels of a frame of
 * finite values come back bit for bit, except that -0.0 becomes +0.0.
 *
 * acg_d_augment_bwd, the adjoint.  Per frame, t = (ty, tx):
 *   g'[q]      = dout[q + t]   if q + t is inside the image and not in the cut rectangle, else 0
 *   din[q, ch] = c * s * g'[q, ch] + c * (1 - s) * mean_ch g'[q, .] + (1 - c) * mean_frame g'
 * and the pad channels of din are written as +0.
 *
 * The shift and cut fields are integer-valued.  They are range-checked in float before any conversion (|v| <= 4096, false for a
 * NaN) and then truncated towards zero; a row with one of the five outside that range has no source pixel that is provably
 * inside: its valid channels come out as 0 (forward) and its g' is 0 (backward).  No index is formed from an unchecked value,
 * so no access leaves the tensors whatever params holds.  b, s, c are used as they are.
 *
 * Two launches each: per-block double partial sums of every (row, frame) - the frame for the forward pass, the live pixels of
 * dout for the adjoint - into the workspace, in a fixed order (each thread its strided share in ascending order, the lanes of a
 * wave by shuffles, the waves in order), then one thread per pixel, which adds the partials in the same fixed way and streams
 * the pixel.  No atomics: the same call gives the same bits.  16-byte accesses where pitch * 4 is a multiple of 16 and both
 * bases are 16-byte aligned, element accesses otherwise, the same bits either way.  acg_d_augment_workspace_bytes is what both
 * need (0 for arguments a launch would refuse); the workspace is 8-byte aligned and holds nothing between calls.
 *
 * acg_d_augment_draw: state uint64 [2] = {seed, counter} (laid out as the noise state above).  Row r uses the Philox4x32-10 blocks
 * 2 r and 2 r + 1 with the counter words (lo32(counter), hi32(counter), block, stream_id ^ ACG_DA_STREAM_TAG) and the key
 * (lo32(seed), hi32(seed)); with x0..x7 their eight words and m_i = x_i >> 9 (23 bits):
 *   ACG_DA_COLOR        b = (m0 - 2^22) * 2^-23 in [-0.5, 0.5),  s = m1 * 2^-22 in [0, 2),  c = 0.5 + m2 * 2^-23 in [0.5, 1.5)
 *   ACG_DA_TRANSLATION  Ry = (h + 4) / 8, Rx = (w + 4) / 8;  ty = ((m3 * (2 Ry + 1)) >> 23) - Ry,  tx likewise from m4 and Rx
 *   ACG_DA_CUTOUT       n = (min(h, w) + 1) / 2;  cy0 = ((m5 * (h + 1)) >> 23) - n / 2,  cx0 = ((m6 * (w + 1)) >> 23) - n / 2
 * (integer divisions, 64-bit products; m7 is not used); a group whose policy bit is clear gets (0, 1, 1), (0, 0), (0, 0, 0).  All
 * of it is integer arithmetic or exact in float32.  Then state[1] = counter + 1: every thread has read the pair, a barrier,
 * thread 0 stores.  One launch of one block.  Calls that share a state must be stream-ordered.
 *
 * 1 <= rows <= ACG_DA_ROWS_MAX, 1 <= frames <= 2, 1 <= cf <= 4, frames * cf <= pitch, 1 <= h, w <= 1024, 0 <= policy <= 7,
 * in != out: a NULL pointer, a workspace that is NULL, misaligned or too small, or a value below its range is
 * ACG_ERR_INVALID_ARG, a value above its range ACG_ERR_UNSUPPORTED; nothing is launched and nothing is written then. */
#define ACG_DA_STREAM_TAG 0x44415547u
#define ACG_DA_ROWS_MAX 1024
#define ACG_DA_COLOR 1
#define ACG_DA_TRANSLATION 2
#define ACG_DA_CUTOUT 4
int32_t acg_d_augment_draw(uint64_t* state, float* params, int32_t rows, int32_t h, int32_t w, int32_t policy, int32_t stream_id,
                           acg_stream_t stream);
int64_t acg_d_augment_workspace_bytes(int32_t rows, int32_t h, int32_t w, int32_t frames, int32_t cf);
int32_t acg_d_augment_fwd(const float* in, const float* params, float* out, int32_t rows, int32_t h, int32_t w, int32_t pitch,
                          int32_t frames, int32_t cf, void* workspace, int64_t workspace_bytes, acg_stream_t stream);
int32_t acg_d_augment_bwd(const float* dout, const float* params, float* din, int32_t rows, int32_t h, int32_t w, int32_t pitch,
                          int32_t frames, int32_t cf, void* workspace, int64_t workspace_bytes, acg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ACGAN_ROLLOUT_H */
