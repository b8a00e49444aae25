/*
 * acgan_ssim_loss.h - SSIM as a training loss of libacgan_hip.so: the value sum_n (1 - SSIM_n) of predicted frames
 * against ground truth and its gradient with respect to the prediction, on the GPU.
 *
 * An addition under ACG_ABI_VERSION 8: it changes no signature of acgan_hip.h, whose conventions it follows - device
 * pointers are borrowed (NHWC, dense float32), scratch comes in through (workspace, workspace_bytes) sized by the query
 * below, calls are asynchronous on `stream`, return ACG_OK or an ACG_ERR_* code with the message in acg_last_error().  The
 * Python binding keeps these entries in a table of their own (_lib.SSIM_LOSS_SIGNATURES): the C oracle does not implement them.
 *
 * SSIM is acgan_metrics.h's, to the letter: 11 x 11 Gaussian window (sigma 1.5, sum 1), VALID positions only
 * ((h - 10) x (w - 10) of them), population moments, C1 = (k1 L)^2, C2 = (k2 L)^2 with L = data_range, the frame's value the
 * mean of the map over the positions and then over the channels.
 *
 * The gradient, per channel, with G the window, x = pred, y = truth, at map position p:
 *   a = G*x, m = G*y, sxx = G*x^2 - a^2, syy = G*y^2 - m^2, sxy = G*xy - a m
 *   A1 = 2 a m + C1, A2 = 2 sxy + C2, B1 = a^2 + m^2 + C1, B2 = sxx + syy + C2, S = A1 A2 / (B1 B2)
 *   Pq = -S / B2,  Pr = 2 A1 / (B1 B2),  U = 2 m A2 / (B1 B2) - 2 a S / B1
 *   dS/dx_i = sum_p G(p, i) [U(p) + 2 (x_i - a(p)) Pq(p) + (y_i - m(p)) Pr(p)]
 *           = G^T[U - 2 a Pq - m Pr] + x_i G^T[2 Pq] + y_i G^T[Pr]
 * where G^T is the full (zero-padded) correlation of the (h - 10) x (w - 10) map back to h x w, separable like G.  The frame's
 * gradient of (1 - SSIM) is -1 / ((h - 10)(w - 10) c) times that.
 *
 * Arithmetic is float32.  x and y are moved by one constant per (frame, channel) - the frame's first value of that channel,
 * so a constant frame moves to exactly 0 - in the pass that writes the three maps AND in the pass that reads them (the form
 * above is invariant under a shift applied to x_i and a alike), and 2 sxy is taken as sxx + syy - Var(x - y), exact in the
 * limit pred -> truth.  No contraction is left to the compiler: the three kinds of call below give the same bits.  The map
 * sum is float64.  Deterministic: no atomics, one writer per element, fixed summation order.
 */
#ifndef ACGAN_SSIM_LOSS_H
#define ACGAN_SSIM_LOSS_H

#include "acgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace acg_ssim_loss needs for n frames of h x w x c: the three maps of the gradient (float32, one value per
 * position and channel each) and the per-block partial sums of the value.  0 when the shape is not supported (n < 1, h or
 * w < 11, c outside 1..4). */
size_t acg_ssim_loss_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c);

/* pred, truth: [n, h, w, c] dense float32, c = 1..4, h and w >= 11 (else ACG_ERR_INVALID_ARG).
 *   value[1]          = sum_n (1 - SSIM(pred_n, truth_n))
 *   dpred[n, h, w, c] = grad_weight * d value / d pred
 * Either output may be NULL, not both.  dpred only (what a training program asks for): two launches - the maps, then their
 * adjoint - and no reduction.  value only: the map pass (writing no maps) and a one-block sum.  Both: three launches.  The
 * blocking depends on (n, h, w) only: the same call gives the same bits, and each output has the same bits in every kind of
 * call; grad_weight scales dpred by one float32 multiplication per element. */
int32_t acg_ssim_loss(const float* pred, const float* truth, float* value, float* dpred, float grad_weight, int32_t n, int32_t h,
                      int32_t w, int32_t c, float data_range, float k1, float k2, void* workspace, size_t workspace_bytes,
                      acg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ACGAN_SSIM_LOSS_H */
