/*
 * acgan_cdna.h - the CDNA generator's output stage in libacgan_hip.so: normalised per-sample kernels, the M transformed
 * images and their masked composite with the previous image, in one kernel per direction (the M transformed images never
 * reach memory).
 *
 * An addition under ACG_ABI_VERSION 8: it changes no signature of acgan_hip.h, whose conventions it follows - device
 * pointers are borrowed (NHWC, float32), scratch comes in through (workspace, workspace_bytes) sized by the query below,
 * calls are asynchronous on `stream`, return ACG_OK or an ACG_ERR_* code with the message in acg_last_error().  The Python
 * binding keeps these entries in a table of their own (_lib.CDNA_SIGNATURES): the C oracle does not implement them.
 *
 * Definitions (B samples of H x W, C colours, M masks, k x k kernels; 1 <= C <= 4, 1 <= M <= 32, k in {3, 5, 7}):
 *   params      [B, k*k*M]   read as [B, k, k, 1, M] (index (u*k + v)*M + m), as acg_cdna_fwd reads them;
 *   kern_norm   [B, k*k*M]   n = (relu(p - relu_shift) + relu_shift) / sum over the k*k taps of one mask;
 *   T_j         j = 0..M-1   the pieces of acg_cdna_fwd: the depthwise SAME correlation of the image with the normalised
 *                            kernels, channel q = c*M + m, split into M pieces of C channels - piece j, channel i is
 *                            colour (j*C + i) / M under mask (j*C + i) % M;
 *   mask_logits [B, H, W, M+1] z; mask_bias [M+1] b (NULL = zero);
 *   s           softmax over the M+1 channels of z + b, per pixel (max-subtracted);
 *   out         [B, H, W, C] = s_0 * image + sum_j s_{j+1} * T_j.
 * image_pitch: channel pitch of `image` (0 = C; C..64).  The output is dense.
 */
#ifndef ACGAN_CDNA_H
#define ACGAN_CDNA_H

#include "acgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace acg_cdna_composite_bwd needs (0 for an unsupported geometry). */
size_t acg_cdna_composite_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t c, int32_t masks, int32_t ksize);

/* out (and kern_norm, when not NULL, for the backward pass) as defined above.  One launch. */
int32_t acg_cdna_composite_fwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                               int32_t image_pitch, float* out, float* kern_norm, int32_t batch, int32_t h, int32_t w, int32_t c,
                               int32_t masks, int32_t ksize, float relu_shift, acg_stream_t stream);

/* Gradients of the composite from dout [B, H, W, C] (no image gradient: the image is an input of the model):
 *   dmask_logits [B, H, W, M+1]: dz_j = s_j (g_j - sum_l s_l g_l), g_0 = <dout, image>, g_{j+1} = <dout, T_j>;
 *   dmask_bias [M+1] (may be NULL): dmask_bias = (accumulate != 0 ? accumulate * dmask_bias : 0) + sum over pixels of dz;
 *   dparams [B, k*k*M]: through T, the normalisation and the relu (zero where p - relu_shift <= 0).
 * kern_norm is the forward's.  Two launches: a per-tile pass that writes dmask_logits and per-(sample, tile) partials into the
 * workspace, and a final pass that sums the partials in a fixed order.  No atomics: the same call gives the same bits. */
int32_t acg_cdna_composite_bwd(const float* params, const float* kern_norm, const float* mask_logits, const float* mask_bias,
                               const float* image, int32_t image_pitch, const float* dout, float* dparams, float* dmask_logits,
                               float* dmask_bias, float dmask_bias_accumulate, int32_t batch, int32_t h, int32_t w, int32_t c,
                               int32_t masks, int32_t ksize, float relu_shift, void* workspace, size_t workspace_bytes,
                               acg_stream_t stream);

/*
 * The affine composite: the output stage of the affine (STP) generator.  Each of the M masks moves the image by a 2x3 affine
 * transform, sampled bilinearly (a "spatial transformer"); the composite and the mask stage are those above.
 *
 * Definitions (B samples of H x W, C colours, M masks; 1 <= C <= 4, 1 <= M <= 32, H, W >= 2; float32, NHWC):
 *   params [B, M*6]   read as [B, M, 6]; theta = params + (1, 0, 0, 0, 1, 0), so zero parameters are the identity;
 *   for output pixel (y, x):  u = 2x/(W-1) - 1, v = 2y/(H-1) - 1;
 *                             xs = t0*u + t1*v + t2, ys = t3*u + t4*v + t5;
 *                             px = (xs+1)(W-1)/2, py = (ys+1)(H-1)/2;
 *                             x0 = floor(px), fx = px - x0; y0 = floor(py), fy = py - y0;
 *   T_m(y, x, c)      = sum over the 4 taps (x0+dx, y0+dy), dx, dy in {0, 1}, of wx*wy*image(tap, c), wx = fx for dx = 1 and
 *                       1-fx for dx = 0, wy likewise from fy; a tap outside [0, W-1] x [0, H-1] contributes 0 (the zeros
 *                       that SAME padding gives the kernels above).  This is grid_sample(image, affine_grid(theta,
 *                       align_corners), bilinear, zeros, align_corners);
 *   s                 = softmax(mask_logits + mask_bias) over the M+1 channels;
 *   out [B, H, W, C]  = s_0 * image + sum_m s_{m+1} * T_m.
 * Gradients: dmask_logits and dmask_bias as above with g_0 = <dout, image>, g_{m+1} = <dout, T_m>;
 *   dparams[b, m, :]  = sum over pixels of s_{m+1} * (a*u, a*v, a, b*u, b*v, b), a = <dout, dT_m/dpx>*(W-1)/2,
 *                       b = <dout, dT_m/dpy>*(H-1)/2, the derivative taken in the cell floor selects (one-sided at a
 *                       coordinate that is exactly an integer).  No image gradient.
 * px, py are range-checked in float before any conversion to int: unless -1 < px < W and -1 < py < H the piece and its
 * gradient are 0, for NaN / Inf parameters too.
 * Conventions as for acg_cdna_composite_*: NULL mask_bias = zero, dmask_bias may be NULL, the same accumulate, image_pitch 0
 * or C..64, ACG_ERR_UNSUPPORTED and a workspace of 0 for an unsupported geometry.
 */

/* Bytes of workspace acg_affine_composite_bwd needs (0 for an unsupported geometry). */
size_t acg_affine_composite_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t c, int32_t masks);

/* out as defined above.  One launch. */
int32_t acg_affine_composite_fwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                 int32_t image_pitch, float* out, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t masks,
                                 acg_stream_t stream);

/* dparams [B, M*6], dmask_logits [B, H, W, M+1] and dmask_bias [M+1] (may be NULL; = (accumulate != 0 ? accumulate *
 * dmask_bias : 0) + sum over pixels of dz) from dout [B, H, W, C].  The warps are recomputed.  Two launches: a per-tile pass
 * that writes dmask_logits and per-(sample, tile) partials into the workspace, and a final pass that sums the partials in
 * tile order.  No atomics: the same call gives the same bits. */
int32_t acg_affine_composite_bwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                 int32_t image_pitch, const float* dout, float* dparams, float* dmask_logits, float* dmask_bias,
                                 float dmask_bias_accumulate, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t masks,
                                 void* workspace, size_t workspace_bytes, acg_stream_t stream);

/*
 * A canvas among the candidates (both composites): a C-channel image the generator paints itself, composited behind the M
 * moved images under a mask channel of its own.
 *
 * Definitions (as above, with 1 <= M <= 31: the canvas takes one of the 33 mask channels the kernels hold):
 *   canvas      [B, H, W, C], dense;
 *   mask_logits [B, H, W, M+2], mask_bias [M+2] (NULL = zero); channel M+1 is the canvas's;
 *   s           softmax over the M+2 channels of z + b, per pixel;
 *   out         = s_0 * image + sum_{j<M} s_{j+1} * T_j + s_{M+1} * canvas.
 * Gradients: g_{M+1} = <dout, canvas> enters dz_j = s_j (g_j - sum_l s_l g_l) beside the other g; dmask_logits
 * [B, H, W, M+2] and dmask_bias [M+2] as above; dparams keeps its definition (the s in it are those of the M+2 channels);
 *   dcanvas [B, H, W, C], dense: s_{M+1} * dout, every element written by exactly one thread.
 * The entries take the arguments of the entries they extend, `canvas` behind image_pitch and `dcanvas` behind
 * dmask_bias_accumulate; both must not be NULL (ACG_ERR_INVALID_ARG).  M = 32 is ACG_ERR_UNSUPPORTED and a workspace of 0.
 * The workspace holds the bias partials of M+2 channels: size it with the *_canvas_workspace_bytes query.  The same
 * kernels as the entries above, compiled with the canvas term: the same two launches, no atomics, the same bits from the
 * same call.
 */
size_t acg_cdna_composite_canvas_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t c, int32_t masks, int32_t ksize);

int32_t acg_cdna_composite_canvas_fwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                      int32_t image_pitch, const float* canvas, float* out, float* kern_norm, int32_t batch,
                                      int32_t h, int32_t w, int32_t c, int32_t masks, int32_t ksize, float relu_shift,
                                      acg_stream_t stream);

int32_t acg_cdna_composite_canvas_bwd(const float* params, const float* kern_norm, const float* mask_logits, const float* mask_bias,
                                      const float* image, int32_t image_pitch, const float* canvas, const float* dout, float* dparams,
                                      float* dmask_logits, float* dmask_bias, float dmask_bias_accumulate, float* dcanvas,
                                      int32_t batch, int32_t h, int32_t w, int32_t c, int32_t masks, int32_t ksize, float relu_shift,
                                      void* workspace, size_t workspace_bytes, acg_stream_t stream);

size_t acg_affine_composite_canvas_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t c, int32_t masks);

int32_t acg_affine_composite_canvas_fwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                        int32_t image_pitch, const float* canvas, float* out, int32_t batch, int32_t h, int32_t w,
                                        int32_t c, int32_t masks, acg_stream_t stream);

int32_t acg_affine_composite_canvas_bwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                        int32_t image_pitch, const float* canvas, const float* dout, float* dparams,
                                        float* dmask_logits, float* dmask_bias, float dmask_bias_accumulate, float* dcanvas,
                                        int32_t batch, int32_t h, int32_t w, int32_t c, int32_t masks, void* workspace,
                                        size_t workspace_bytes, acg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ACGAN_CDNA_H */
