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

#ifdef __cplusplus
}
#endif

#endif /* ACGAN_ROLLOUT_H */
