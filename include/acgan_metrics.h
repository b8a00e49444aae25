/*
 * acgan_metrics.h - evaluation metrics of libacgan_hip.so: per-frame SSIM and squared error of predicted frames against
 * ground truth, on the GPU next to the frames (the quality curves of the reference's report).
 *
 * An addition under ACG_ABI_VERSION 8: it changes no signature of acgan_hip.h, whose conventions it follows - device
 * pointers are borrowed (NHWC), scratch comes in through (workspace, workspace_bytes) sized by the query below, calls are
 * asynchronous on `stream`, return ACG_OK or an ACG_ERR_* code with the message in acg_last_error().  The Python binding
 * keeps these entries in a table of their own (_lib.METRICS_SIGNATURES): the C oracle does not implement them.
 *
 * SSIM (tf.image.ssim's definition; equally skimage.metrics.structural_similarity with gaussian_weights=True,
 * use_sample_covariance=False):
 *   - window: 11 x 11 Gaussian, sigma = 1.5, normalised to sum 1;
 *   - VALID filtering only: (h - 10) x (w - 10) output positions;
 *   - mu_x, mu_y, sigma_x^2, sigma_y^2, sigma_xy are population (Gaussian-weighted) moments;
 *   - C1 = (k1 L)^2, C2 = (k2 L)^2 with L = data_range (2.0 for frames in [-1, 1]; k1 = 0.01, k2 = 0.03 as in the literature);
 *   - SSIM map = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_x^2 + sigma_y^2 + C2));
 *   - the per-frame value is the mean of the map over the positions and then over the channels.
 * Arithmetic is float32 (moments about a per-block shift, covariance through Var(pred - truth): within 1e-5 of float64),
 * sums of the map and of the squared error in float64.  Deterministic: no atomics, fixed summation order.
 */
#ifndef ACGAN_METRICS_H
#define ACGAN_METRICS_H

#include "acgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace acg_frame_metrics needs for n frames of h x w (0 when h or w < 11 or n < 1). */
size_t acg_frame_metrics_workspace_bytes(int32_t n, int32_t h, int32_t w);

/* pred [n, h, w, pitch], truth [n, h, w, pitch] (channels 0..c-1 are read; pitch 0 = c) ->
 *   ssim[n]  (float32): per-frame SSIM as defined above;
 *   sqerr[n] (float32): sum of (pred - truth)^2 over the h * w * c values of the frame.
 * dtype: storage of both inputs (ACG_F32 / ACG_BF16) or ACG_DTYPE2(pred, truth) - e.g. a bf16 session's frames against float32
 * ground truth.  c = 1..4, pitch = c..64.  h < 11 or w < 11: ACG_ERR_INVALID_ARG.  Two launches (one partial pass, one
 * per-frame sum) on `stream`.  The blocking of a frame depends on (n, h, w) only: the same call gives the same bits, a call with
 * another n may differ in the last bits. */
int32_t acg_frame_metrics(const void* pred, const void* truth, float* ssim, float* sqerr, int32_t n, int32_t h, int32_t w,
                          int32_t c, int32_t pitch, int32_t dtype, float data_range, float k1, float k2, void* workspace,
                          size_t workspace_bytes, acg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ACGAN_METRICS_H */
