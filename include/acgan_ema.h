/*
 * acgan_ema.h - the exponential moving average of a scope's weights (tf.train.ExponentialMovingAverage with its
 * `num_updates` warm-up): one float32 shadow buffer with the layout of the scope's flat parameter buffer, updated behind
 * every optimizer update - by a launch of its own (acg_ema_update) or inside the optimizer's launch, from the new parameter
 * while it is still in a register (acg_adam_step_ema / acg_rmsprop_step_ema) - and acg_swap_f32, which exchanges the
 * shadow and the parameters in place so that programs captured with their pointers can predict with the averaged weights.
 *
 * An addition under ACG_ABI_VERSION 8: it changes no signature of acgan_hip.h, whose conventions it follows - device
 * pointers are borrowed, calls are asynchronous on `stream`, return ACG_OK or an ACG_ERR_* code with the message in
 * acg_last_error().  The Python binding keeps these entries in a table of their own (_lib.EMA_SIGNATURES): the C oracle
 * does not implement them.
 *
 * The update (k = *num_updates as the launch finds it, p = the parameter after the optimizer update and its clip):
 *   k == 0:  shadow = p                         (a deviation from TensorFlow, which seeds the shadow with the INITIAL value:
 *                                                a counter of 0 - a reset, a checkpoint from before the average existed -
 *                                                then starts cleanly from the weights as they are)
 *   k  > 0:  d   = min((double)decay, (1.0 + k) / (10.0 + k))            in double
 *            omd = (float)(1.0 - d)
 *            shadow = shadow - omd * (shadow - p)                        three separately rounded float32 operations,
 *                                                                        never contracted into an FMA: the same bits in every entry
 *   then     *num_updates = k + 1
 * The counter is advanced INSIDE the launch, by the last block to retire: `state` is one 32-bit word (zero before the first
 * call) that counts retired blocks with agent-scope atomics and is reset to zero by that block, so the launch replays in a
 * captured graph with no memset and nothing ever waits on the word.  Every block reads the counter before it adds itself
 * to the word, so the advance cannot race with the reads of its own launch.  One `state` word belongs to one counter; calls
 * that share them must be ordered on one stream (or by graph edges).
 */
#ifndef ACGAN_EMA_H
#define ACGAN_EMA_H

#include "acgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* shadow, param: float32 [n] (16-byte aligned buffers take 16-byte accesses, a scalar tail covers any n; other alignments run
 * scalar); 0 < decay < 1; num_updates: int64 [1] on the device, 8-byte aligned; state: uint32 [1] on the device. */
int32_t acg_ema_update(float* shadow, const float* param, int64_t n, float decay, int64_t* num_updates, uint32_t* state,
                       acg_stream_t stream);

/* acg_adam_step / acg_rmsprop_step (same arguments, same bits in param and slots) with the update above of shadow[i] from the new
 * param[i] in the same launch: shadow and *num_updates come out as acg_ema_update run behind the plain step leaves them. */
int32_t acg_adam_step_ema(float* param, const float* grad, float* m, float* v, const int32_t* step_dev, int64_t n, float lr,
                          float beta1, float beta2, float eps, float grad_scale, int32_t use_clip, float clip_lo, float clip_hi,
                          float* shadow, float ema_decay, int64_t* num_updates, uint32_t* state, acg_stream_t stream);
int32_t acg_rmsprop_step_ema(float* param, const float* grad, float* ms, int64_t n, float lr, float decay, float eps,
                             float grad_scale, int32_t use_clip, float clip_lo, float clip_hi, float* shadow, float ema_decay,
                             int64_t* num_updates, uint32_t* state, acg_stream_t stream);

/* a[i] <-> b[i], i < n, in one launch; the two buffers must not overlap. */
int32_t acg_swap_f32(float* a, float* b, int64_t n, acg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ACGAN_EMA_H */
