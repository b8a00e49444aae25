/*
 * acgan_bn_infer.h - BatchNorm with STORED statistics: the apply pass on its own (prediction that does not depend on the
 * other rows of the batch) and the calibration pass that pools the moments of the batches it is shown.
 *
 * An addition under ACG_ABI_VERSION 8: it changes no signature of acgan_hip.h, whose conventions it follows - device
 * pointers are borrowed, [rows, channels] NHWC views with rows `pitch` elements apart, calls are asynchronous on `stream`,
 * return ACG_OK or an ACG_ERR_* code with the message in acg_last_error().  No entry uses atomics: the same calls give the
 * same bits.  The Python binding keeps these entries in a table of their own (_lib.BN_INFER_SIGNATURES): the C oracle does
 * not implement them.
 *
 * dtype: the storage type of x and y (ACG_F32 / ACG_BF16), or ACG_DTYPE2(x, y) = ACG_DTYPE2(ACG_BF16, ACG_F32) as
 * acg_bn_act_fwd takes it.  x_pitch / y_pitch: 0 = dense = channels.  Channels at or beyond `channels` are neither read
 * nor written, as in acg_bn_act_fwd: a layer's output may sit inside its concatenation with the action channels, whose
 * columns [channels, pitch) belong to somebody else; the pad channels of a zero-initialised tensor therefore stay zero.
 */
#ifndef ACGAN_BN_INFER_H
#define ACGAN_BN_INFER_H

#include "acgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y[r, c] = act((x[r, c] - mean[c]) * (1 / sqrt(variance[c] + eps)) + beta[c]) in float32 arithmetic; act = ACG_ACT_NONE,
 * ACG_ACT_RELU or ACG_ACT_LRELU (`leak`).  mean, variance, beta: float32 [channels].  Every element is read once and
 * written once; a row's result depends on no other row.  One launch, no workspace. */
int32_t acg_bn_act_infer(const void* x, const float* beta, const float* mean, const float* variance, void* y, int64_t rows,
                         int32_t channels, int32_t x_pitch, int32_t y_pitch, float eps, int32_t act, float leak, int32_t dtype,
                         acg_stream_t stream);

/* Pools the per-channel moments of the `rows` rows of x into the running (count, mean, variance):
 *   n_b, m_b, M2_b = row count, mean and sum of squared deviations of x's rows (per channel);
 *   count == 0:  mean = m_b, variance = M2_b / n_b                        (whatever mean / variance held is ignored)
 *   else:        n = count + n_b, d = m_b - mean,
 *                variance = (variance * count + M2_b + d * d * count * n_b / n) / n,  mean = mean + d * n_b / n
 *   count = count + n_b
 * - the parallel-variance (Chan) update: after any sequence of calls the state holds the mean and the biased variance of
 * the concatenation of all rows shown.  Sums are centred before they are squared (a block shifts by its own first row)
 * and blocks are merged in a fixed order, Chan-style as well: nothing of the size of mean^2 is formed.
 * count: ONE int64 in device memory (a captured graph replays correctly); mean, variance: float32 [channels].
 * x is read once.  Three launches on `stream` (block moments; merge; count).  workspace: acg_bn_collect_workspace_bytes. */
size_t acg_bn_collect_workspace_bytes(int64_t rows, int32_t channels);
int32_t acg_bn_collect(const void* x, int64_t* count, float* mean, float* variance, int64_t rows, int32_t channels,
                       int32_t x_pitch, int32_t dtype, void* workspace, size_t workspace_bytes, acg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ACGAN_BN_INFER_H */
