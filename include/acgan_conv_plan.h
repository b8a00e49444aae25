/*
 * acgan_conv_plan.h - a read-only answer to "which kernel would this convolution call launch" in libacgan_hip.so.
 *
 * An addition under ACG_ABI_VERSION 8: it changes no signature of acgan_hip.h.  Both queries launch nothing and touch no
 * memory but `out`; they answer from the host functions the conv entries themselves launch through (the planner, the
 * merged-input-gradient rule, the geometry flags, the paired-launch rule and the choice of the split-K reduction in
 * conv_f32.hip), so a retuned constant moves the answer together with the launch.  tests/conv_path_cases.py keeps one small
 * shape per kernel variant and states the path it expects; tools/conv_path_sweep.hip prints the same answers on a host
 * without a GPU.  The C oracle does not implement them.
 */
#ifndef ACGAN_CONV_PLAN_H
#define ACGAN_CONV_PLAN_H

#include "acgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ACG_PATH_DIRECT = 0, ACG_PATH_MFMA_F32 = 1, ACG_PATH_MFMA_BF16 = 2, ACG_PATH_GLDS_BF16 = 3 };
enum { ACG_REDUCE_NONE = 0, ACG_REDUCE_PLAIN = 1, ACG_REDUCE_BF16 = 2, ACG_REDUCE_COLS = 3 };
enum { ACG_PAIR_DIRECT = 1,      /* direct_pair: both contractions on the direct kernels, one launch (conv layers only) */
       ACG_PAIR_F32 = 2,         /* conv_pair_f32 */
       ACG_PAIR_BF16 = 3,        /* conv_pair_bf16 */
       ACG_PAIR_TWO = 4,         /* two launches: the contractions as the separate entries run them */
       ACG_PAIR_MERGED = 5 };    /* the merged input gradient, then the weight gradient as a launch of its own */

typedef struct acg_conv_path {
  int32_t family;                /* ACG_PATH_* */
  int32_t tile_rows, tile_cols;  /* block tile (direct: 64 x 64, unused by those kernels) */
  int32_t tiles, classes, nk, splits;
  int32_t ragged, nvec, lin, compact;      /* fp32 MFMA template / geometry switches; 0 for the other families */
  int32_t merged;                /* DGRAD taken by the merged input gradient: every other field describes the stride-1
                                    forward contraction it runs as */
  int32_t reduce;                /* ACG_REDUCE_*: the kernel that sums the slabs of the plain (not slabs-only) entry */
  int32_t direct_nb;             /* direct family: the NB template argument (1 or 8); 0 otherwise */
  int32_t uniform_k;             /* fp32 MFMA: the loaders keep their K-step state in scalar registers (FWD where lin, and DGRAD,
                                    with 16-byte gathers of a multiple of 32 channels); 0 for the other families */
  int32_t uniform_w;             /* fp32 MFMA weight gradient: `live`, the dY row origin and the range tests ride in the buffer
                                    descriptors, the row table holds byte offsets (16-byte loads on both sides: not ragged, nvec);
                                    0 for the other contractions and families.  As B of conv_pair_f32 the weight gradient
                                    follows this answer except for a 64 x 64 tile beside a 128 x 32 contraction A, which
                                    keeps the generic loaders (same bits) */
} acg_conv_path;

/* The path of acg_conv2d_fwd / _dgrad / _wgrad (`which` = ACG_CONV_*) on `desc` with the storage `dtype` (ACG_F32, ACG_BF16 or
 * ACG_DTYPE2(ACG_BF16, ACG_F32)).  as_pair_a = 1: planned as contraction A of acg_conv2d_bwd_pair / acg_deconv2d_bwd_pair
 * (no 256 x 128 tile, no merged form).  ACG_OK, or the error the entry itself would report for this descriptor. */
int32_t acg_conv2d_path(const acg_conv_desc* desc, int32_t which, int32_t dtype, int32_t as_pair_a, acg_conv_path* out);

/* What acg_conv2d_bwd_pair (transposed = 0) / acg_deconv2d_bwd_pair (1) does with `desc`, `dtype` and its flag word:
 * ACG_PAIR_*, or 0 where the entry would refuse the call.  The contractions of ACG_PAIR_F32 / _BF16 are
 * acg_conv2d_path(desc, A, dtype, 1) and acg_conv2d_path(desc, ACG_CONV_WGRAD, dtype, 0). */
int32_t acg_conv2d_pair_path(const acg_conv_desc* desc, int32_t transposed, int32_t dtype, int32_t flags);

/* Process-wide: on = 0 keeps every fp32 MFMA launch on the generic loaders, 1 (the default) lets the eligible ones take the
 * uniform_k variant.  The two compute the same bits; no plan (tile, splits, reduction, workspace) depends on the switch.  It is
 * there so that a test can run both in one process - not thread-safe against launches in flight on other threads. */
int32_t acg_conv2d_uniform_k(int32_t on);

/* The same switch for the uniform_w variant of the weight gradients: 0 or 1 (the default), the variant alone, never a plan; the two
 * loaders compute the same bits.  Independent of acg_conv2d_uniform_k, which never touches a weight gradient. */
int32_t acg_conv2d_uniform_w(int32_t on);

#ifdef __cplusplus
}
#endif

#endif /* ACGAN_CONV_PLAN_H */
