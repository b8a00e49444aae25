"""ctypes binding of libacgan_hip.so (include/acgan_hip.h).

There is no fallback: if the HIP library has not been built (``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C action_conditioned_gans_amd/csrc``) every
operator raises ``RuntimeError``.  Nothing here knows about the CPU oracle.

``SIGNATURES`` is the core table (include/acgan_hip.h): every library must export all of it.  ``EXTENSIONS`` holds the additions
that live in a header of their own; a ``Library`` binds each group its shared object exports, ``get()`` requires all of them,
and ops look such an entry up with ``entry(lib, name)``.
"""
import collections
import ctypes
import os
from ctypes import c_char_p, c_float, c_int32, c_int64, c_size_t, c_void_p

# torch FIRST: it carries its own copy of the HIP runtime, and the process must end up with ONE.  Loaded after torch,
# libacgan_hip.so binds to the runtime torch has already mapped (streams, device memory and graphs are then shared);
# loaded before it, the library would initialise the system runtime and torch a second one, and the first kernel
# launch from here fails with "no ROCm-capable device is detected" (seen in build() -> smoke() in one process).
import torch  # noqa: F401  (import order is the point)

ACG_F32, ACG_BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
CONV_FWD, CONV_DGRAD, CONV_WGRAD = 0, 1, 2
SLABS_ROWS, SLABS_QUADS = 0, 1       # acgan_hip.h ACG_SLABS_*
BN_NO_GRID_EXCHANGE = 1               # acgan_hip.h ACG_BN_NO_GRID_EXCHANGE
ABI_VERSION = 8       # include/acgan_hip.h ACG_ABI_VERSION: bumped with every signature / layout / flag-meaning change

LIB_NAME = 'libacgan_hip.so'
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', LIB_NAME)


class ConvDesc(ctypes.Structure):
    """struct acg_conv_desc."""
    _fields_ = [(n, c_int32) for n in (
        'batch', 'in_h', 'in_w', 'in_c', 'out_h', 'out_w', 'out_c', 'kh', 'kw',
        'stride_h', 'stride_w', 'pad_top', 'pad_left', 'in_pitch', 'out_pitch', 'dgrad_c', 'adj_dgrad_c')]

    def key(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


class ConvPath(ctypes.Structure):
    """struct acg_conv_path (include/acgan_conv_plan.h)."""
    FAMILIES = ('direct', 'mfma_f32', 'mfma_bf16', 'glds_bf16')
    REDUCES = ('none', 'plain', 'bf16', 'cols')
    _fields_ = [(n, c_int32) for n in (
        'family', 'tile_rows', 'tile_cols', 'tiles', 'classes', 'nk', 'splits', 'ragged', 'nvec', 'lin', 'compact', 'merged', 'reduce',
        'direct_nb', 'uniform_k', 'uniform_w')]


PAIR_KINDS = ('refused', 'direct_pair', 'conv_pair_f32', 'conv_pair_bf16', 'two_launches', 'merged')      # ACG_PAIR_*


class ReduceList(ctypes.Structure):
    """struct acg_reduce_list (ACG_REDUCE_MAX = 32 entries)."""
    _fields_ = [('slabs', c_void_p * 32), ('out', c_void_p * 32), ('numel', c_int64 * 32), ('splits', c_int32 * 32),
                ('accumulate', c_float * 32), ('step_inc', c_void_p)]


class PrepList(ctypes.Structure):
    """struct acg_prep_list (ACG_PREP_MAX = 32 filters)."""
    _fields_ = [('src', c_void_p * 32), ('rm', c_void_p * 32), ('tr', c_void_p * 32), ('taps', c_int32 * 32), ('a', c_int32 * 32),
                ('b', c_int32 * 32)]


class NormSegments(ctypes.Structure):
    """struct acg_norm_segments (ACG_NORM_SEGMENTS_MAX = 64 windows of a flat gradient buffer; include/acgan_rollout.h)."""
    _fields_ = [('count', c_int32), ('offset', c_int64 * 64), ('length', c_int64 * 64)]


class LrSched(ctypes.Structure):
    """struct acg_lr_schedule (acg_adam_step_lr / acg_rmsprop_step_lr; include/acgan_rollout.h)."""
    KINDS = ('constant', 'linear', 'cosine', 'exponential')         # ACG_LR_*
    _fields_ = [('kind', c_int32), ('warmup', c_int64), ('decay_steps', c_int64), ('final_factor', c_float)]


class SsSched(ctypes.Structure):
    """struct acg_ss_schedule (acg_sched_sample_draw; include/acgan_rollout.h)."""
    KINDS = ('constant', 'linear', 'inverse_sigmoid')               # ACG_SS_*
    _fields_ = [('kind', c_int32), ('offset', c_int64), ('decay_steps', c_int64), ('start', c_float), ('final', c_float)]


class OptArgs(ctypes.Structure):
    """struct acg_opt_args (acg_opt_step_prepare_bf16)."""
    _fields_ = [('kind', c_int32), ('lr', c_float), ('beta1_or_decay', c_float), ('beta2', c_float), ('eps', c_float),
                ('grad_scale', c_float), ('use_clip', c_int32), ('clip_lo', c_float), ('clip_hi', c_float)]


class CopyList(ctypes.Structure):
    """struct acg_copy_list (ACG_COPY_MAX = 8 segments)."""
    _fields_ = [('src', c_void_p * 8), ('dst', c_void_p * 8), ('rows', c_int64 * 8), ('cols', c_int32 * 8),
                ('dst_pitch', c_int32 * 8), ('dst_dtype', c_int32 * 8), ('src_div', c_int32 * 8), ('src_mod', c_int32 * 8)]


_P = c_void_p
_D = ctypes.POINTER(ConvDesc)
_conv = [_P, _P, _P, _D, c_int32, _P, c_size_t, _P]
_wgrad = [_P, _P, _P, c_float, _D, c_int32, _P, c_size_t, _P]

# The restype of an entry point whose int32 is an error code: bound as c_int32 and wrapped so that a non-zero result raises
# AcgError with acg_last_error().  A plain c_int32 restype is a value (a count, a layout, a yes/no) and is returned as it is.
STATUS = type('STATUS', (), {})

# name -> (restype, argtypes); mirrors include/acgan_hip.h one to one.
SIGNATURES = {
    'acg_version': (c_int32, []),
    'acg_build_info': (c_char_p, []),
    'acg_last_error': (c_char_p, []),
    'acg_conv_desc_init': (STATUS, [_D] + [c_int32] * 9),
    'acg_conv2d_workspace_bytes': (c_size_t, [_D, c_int32, c_int32]),
    'acg_conv2d_fwd': (STATUS, _conv),
    'acg_conv2d_dgrad': (STATUS, _conv),
    'acg_conv2d_wgrad': (STATUS, _wgrad),
    'acg_conv2d_splits': (c_int32, [_D, c_int32, c_int32]),
    'acg_conv2d_tile': (c_int32, [_D, c_int32, c_int32, ctypes.POINTER(c_int32), ctypes.POINTER(c_int32)]),
    'acg_conv2d_wgrad_slabs': (STATUS, [_P, _P, _D, c_int32, _P, c_size_t, _P]),
    'acg_deconv2d_wgrad_slabs': (STATUS, [_P, _P, _D, c_int32, _P, c_size_t, _P]),
    'acg_conv2d_stats_blocks': (c_int32, [_D, c_int32, c_int32, c_int32]),
    'acg_conv2d_stats_layout': (c_int32, [_D, c_int32, c_int32, c_int32, ctypes.POINTER(c_int32), ctypes.POINTER(c_int32)]),
    'acg_conv2d_fwd_stats': (STATUS, [_P, _P, _P, _D, c_int32, _P, c_size_t, _P, c_int32, _P]),
    'acg_deconv2d_fwd_stats': (STATUS, [_P, _P, _P, _D, c_int32, _P, c_size_t, _P, c_int32, _P]),
    'acg_deconv2d_fwd_bias_act_ok': (c_int32, [_D, c_int32]),
    'acg_deconv2d_fwd_bias_act': (STATUS, [_P, _P, _P, _P, _D, c_int32, c_float, c_int32, _P]),
    'acg_conv2d_slab_layouts': (c_int32, [_D, c_int32, c_int32]),
    'acg_conv2d_fwd_slabs': (STATUS, [_P, _P, _D, c_int32, c_int32, _P, c_size_t, _P]),
    'acg_conv2d_dgrad_slabs': (STATUS, [_P, _P, _D, c_int32, c_int32, _P, c_size_t, _P]),
    'acg_deconv2d_fwd_slabs': (STATUS, [_P, _P, _D, c_int32, c_int32, _P, c_size_t, _P]),
    'acg_deconv2d_dgrad_slabs': (STATUS, [_P, _P, _D, c_int32, c_int32, _P, c_size_t, _P]),
    'acg_conv2d_bwd_pair': (STATUS, [_P, _P, _P, _P, _P, c_float, _D, c_int32, _P, c_size_t, _P, c_size_t, c_int32, _P]),
    'acg_deconv2d_bwd_pair': (STATUS, [_P, _P, _P, _P, _P, c_float, _D, c_int32, _P, c_size_t, _P, c_size_t, c_int32, _P]),
    'acg_splitk_reduce_many': (STATUS, [ctypes.POINTER(ReduceList), c_int32, _P]),
    'acg_weights_prepare_bf16': (STATUS, [ctypes.POINTER(PrepList), c_int32, _P]),
    'acg_deconv2d_fwd': (STATUS, _conv),
    'acg_deconv2d_dgrad': (STATUS, _conv),
    'acg_deconv2d_wgrad': (STATUS, _wgrad),
    'acg_bn_workspace_bytes': (c_size_t, [c_int64, c_int32, c_int32]),
    'acg_bn_moments': (STATUS, [_P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, _P, c_size_t, _P]),
    'acg_bn_act_fwd_moments': (STATUS, [_P, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, c_float,
                                        c_int32, _P]),
    'acg_bn_bwd_sums': (STATUS, [_P, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, _P,
                                 c_size_t, _P]),
    'acg_bn_act_bwd_sums': (STATUS, [_P, _P, _P, _P, _P, _P, _P, c_int64, _P, _P, c_float, c_int64, c_int32, c_int32, c_int32, c_int32,
                                     c_int32, c_float, c_int32, _P]),
    'acg_bn_exchange_selftest': (STATUS, [_P, c_size_t, _P, c_int32, c_int32, c_int32, ctypes.c_uint32, _P]),
    'acg_bn_act_fwd': (STATUS, [_P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, c_float,
                                c_int32, c_int32, _P, c_size_t, _P]),
    'acg_bn_act_bwd': (STATUS, [_P, _P, _P, _P, _P, _P, _P, c_float, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32,
                                c_float, c_int32, c_int32, _P, c_size_t, _P]),
    'acg_bn_act_fwd_partials': (STATUS, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, c_float,
                                         c_int32, _P]),
    'acg_bn_slabs_layout': (c_int32, [c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    'acg_bn_act_fwd_slabs': (STATUS, [_P, c_int32, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, c_float,
                                      c_int32, c_int32, c_int32, _P, c_size_t, _P]),
    'acg_bn_bwd_slabs_ok': (c_int32, [c_int64, c_int32]),
    'acg_bn_act_bwd_slabs': (STATUS, [_P, _P, c_int32, _P, _P, _P, _P, _P, c_float, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32,
                                      c_float, c_int32, c_int32, c_int32, _P, c_size_t, _P]),
    'acg_bias_workspace_bytes': (c_size_t, [c_int64, c_int32]),
    'acg_bias_act_fwd': (STATUS, [_P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, _P]),
    'acg_bias_act_bwd': (STATUS, [_P, _P, _P, _P, c_float, c_int64, c_int32, c_int32, c_int32, c_int32, c_float, c_int32,
                                  _P, c_size_t, _P]),
    'acg_dna_workspace_bytes': (c_size_t, [c_int32] * 4),
    'acg_dna_fwd': (STATUS, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
    'acg_dna_bwd': (STATUS, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, _P, _P, c_float, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P,
                             c_size_t, _P]),
    'acg_cdna_workspace_bytes': (c_size_t, [c_int32] * 6),
    'acg_cdna_fwd': (STATUS, [_P, _P, _P, _P] + [c_int32] * 6 + [c_float, c_int32, _P]),
    'acg_cdna_bwd': (STATUS, [_P, _P, _P, _P, _P, _P] + [c_int32] * 6 + [c_float, c_int32, _P, c_size_t, _P]),
    'acg_concat_actions_fwd': (STATUS, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
    'acg_concat_channels_fwd': (STATUS, [_P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, _P]),
    'acg_slice_channels': (STATUS, [_P, _P, c_float, c_int64, c_int32, c_int32, c_int32, c_int32, _P]),
    'acg_copy_many': (STATUS, [ctypes.POINTER(CopyList), c_int32, c_int32, _P]),
    'acg_stream_edge_create': (STATUS, [ctypes.POINTER(c_void_p)]),
    'acg_stream_edge_destroy': (STATUS, [_P]),
    'acg_stream_edge': (STATUS, [_P, _P, _P]),
    'acg_add': (STATUS, [_P, _P, _P, c_int64, c_int32, _P]),
    'acg_frame_loss_workspace_bytes': (c_size_t, [c_int64]),
    'acg_frame_loss': (STATUS, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_int32,
                                _P, c_size_t, _P]),
    'acg_l2norm_loss': (STATUS, [_P, _P, _P, _P, c_int64, c_float, _P]),
    'acg_sumsq_diff': (STATUS, [_P, _P, _P, c_int64, _P]),
    'acg_l2norm_loss_global': (STATUS, [_P, _P, _P, _P, _P, c_int64, c_float, _P]),
    'acg_sigmoid_ce_loss': (STATUS, [_P, c_float, _P, _P, c_int64, c_float, _P]),
    'acg_mean_loss': (STATUS, [_P, _P, _P, c_int64, c_float, _P]),
    'acg_psnr': (STATUS, [_P, _P, _P, c_int64, c_int32, _P, c_size_t, _P]),
    'acg_scalar_combine': (STATUS, [_P, _P, c_float, _P, c_float, _P, c_float, _P, c_float, _P]),
    'acg_opt_step_prepare_bf16': (STATUS, [_P, _P, _P, _P, _P, c_int64, ctypes.POINTER(OptArgs), ctypes.POINTER(PrepList), c_int32, _P]),
    'acg_adam_step': (STATUS, [_P, _P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_float,
                               c_int32, c_float, c_float, _P]),
    'acg_rmsprop_step': (STATUS, [_P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_int32, c_float,
                                  c_float, _P]),
    'acg_clip': (STATUS, [_P, c_int64, c_float, c_float, _P]),
    'acg_step_inc': (STATUS, [_P, _P]),
}

Extension = collections.namedtuple('Extension', 'header what signatures')

# Additions under ABI version 8, one header each.  The C oracle (oracle/cbind) implements none of them and is never asked for
# one: a Library binds the groups its shared object exports, and entry() names the header when an op asks a library for an
# entry it does not have.  ``what`` closes that message.
EXTENSIONS = {
    # per-frame SSIM and squared error for the evaluation (metrics.frame_metrics)
    'metrics': Extension('include/acgan_metrics.h', 'SSIM runs on the GPU only, there is no host fallback', {
        'acg_frame_metrics_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32]),
        'acg_frame_metrics': (STATUS, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_float,
                                       _P, c_size_t, _P]),
    }),
    # the CDNA generator's fused transform-and-composite (ops.CdnaCompositeOp) and the affine generator's warp-and-composite
    'cdna': Extension('include/acgan_cdna.h', 'the CDNA and the affine generators run on the HIP library only', {
        'acg_cdna_composite_workspace_bytes': (c_size_t, [c_int32] * 6),
        'acg_cdna_composite_fwd': (STATUS, [_P, _P, _P, _P, c_int32, _P, _P] + [c_int32] * 6 + [c_float, _P]),
        'acg_cdna_composite_bwd': (STATUS, [_P, _P, _P, _P, _P, c_int32, _P, _P, _P, _P, c_float] + [c_int32] * 6
                                   + [c_float, _P, c_size_t, _P]),
        # the affine (STP) generator's fused warp-and-composite (ops.AffineCompositeOp)
        'acg_affine_composite_workspace_bytes': (c_size_t, [c_int32] * 5),
        'acg_affine_composite_fwd': (STATUS, [_P, _P, _P, _P, c_int32, _P] + [c_int32] * 5 + [_P]),
        'acg_affine_composite_bwd': (STATUS, [_P, _P, _P, _P, c_int32, _P, _P, _P, _P, c_float] + [c_int32] * 5 + [_P, c_size_t, _P]),
        # the same two with a painted canvas among the candidates (ops.MaskCompositeOp canvas=): ``canvas`` behind the image
        # pitch, ``dcanvas`` behind the accumulate factor
        'acg_cdna_composite_canvas_workspace_bytes': (c_size_t, [c_int32] * 6),
        'acg_cdna_composite_canvas_fwd': (STATUS, [_P, _P, _P, _P, c_int32, _P, _P, _P] + [c_int32] * 6 + [c_float, _P]),
        'acg_cdna_composite_canvas_bwd': (STATUS, [_P, _P, _P, _P, _P, c_int32, _P, _P, _P, _P, _P, c_float, _P] + [c_int32] * 6
                                          + [c_float, _P, c_size_t, _P]),
        'acg_affine_composite_canvas_workspace_bytes': (c_size_t, [c_int32] * 5),
        'acg_affine_composite_canvas_fwd': (STATUS, [_P, _P, _P, _P, c_int32, _P, _P] + [c_int32] * 5 + [_P]),
        'acg_affine_composite_canvas_bwd': (STATUS, [_P, _P, _P, _P, c_int32, _P, _P, _P, _P, _P, c_float, _P] + [c_int32] * 5
                                            + [_P, c_size_t, _P]),
    }),
    # the image gradient of the DNA tail and the gradient of a tiled action vector, which training through the generator's own
    # rollouts needs (train.Trainer rollout_steps > 1; ops.DnaImageGradOp / ActionGradOp), and the global-norm clip of a flat
    # gradient buffer that bounds them (optim.ClipNormOp); the header owns the device-side action vector, so the noise that is
    # appended to it - drawn on the device, the counter advanced by the kernel (ops.NoiseOp) - is here too; and, beside the clip as
    # "what sits in front of the optimizer update", the optimizer steps that evaluate a learning-rate schedule inside their launch
    # from an update counter they advance themselves (optim.LrSchedule); and scheduled sampling of the rollout's fed-back inputs;
    # and the launches of the planner around the generator forwards (plan.Planner)
    # and instance noise on the discriminator's inputs with the statistics of its logits (train.Trainer d_noise / d_stats)
    # and the learned posterior of the noise input, which draws from the noise input's state (train.Trainer posterior)
    'rollout': Extension('include/acgan_rollout.h', 'training through rollouts, scheduled sampling, the gradient clip, the noise input, '
                         'learning-rate schedules, planning, instance noise and the latent posterior run on the HIP library only', {
        'acg_dna_bwd_image': (STATUS, [_P, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_float] + [c_int32] * 6 + [_P]),
        'acg_action_grad': (STATUS, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, _P, c_float, _P]),
        'acg_grad_clip_norm_workspace_bytes': (c_size_t, [c_int64, ctypes.POINTER(NormSegments)]),
        'acg_grad_clip_norm': (STATUS, [_P, c_int64, ctypes.POINTER(NormSegments), c_float, c_float, _P, _P, c_size_t, _P]),
        'acg_noise_concat': (STATUS, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P]),
        'acg_adam_step_lr': (STATUS, [_P, _P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_float, c_int32, c_float, c_float,
                                      ctypes.POINTER(LrSched), _P, _P, _P, _P, c_float, _P, _P, _P]),
        'acg_rmsprop_step_lr': (STATUS, [_P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_int32, c_float, c_float,
                                         ctypes.POINTER(LrSched), _P, _P, _P, _P, c_float, _P, _P, _P]),
        # scheduled sampling of the K-step rollout (ops.SchedSampleDrawOp / SchedSampleOp): coins, row select, adjoint
        'acg_sched_sample_draw': (STATUS, [_P, ctypes.POINTER(SsSched), _P, _P, c_int32, c_int32, c_int32, _P]),
        'acg_sched_sample_fwd': (STATUS, [_P, _P, _P, _P, c_int64, _P, _P, _P, c_int32, c_int32, _P]),
        'acg_sched_sample_bwd': (STATUS, [_P, _P, _P, c_int64, _P, _P, c_int32, c_int32, _P]),
        # planning by the cross-entropy method around the generator forwards (plan.sample_actions / accumulate_cost / refit)
        'acg_plan_sample': (STATUS, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
        'acg_plan_cost': (STATUS, [_P, _P, _P, _P, c_float, c_float, _P, c_int32] + [c_int32] * 7 + [_P]),
        'acg_plan_refit': (STATUS, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_float, c_float, _P]),
        # the planner's designated-pixel cost on the maps the DNA tail advects (plan.accumulate_pixel_cost)
        'acg_plan_pixel_cost': (STATUS, [_P, _P, c_float, _P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P]),
        # instance noise on the discriminator's inputs (ops.InstNoisePrepareOp / InstNoiseOp) and the statistics of its logits
        # (ops.LogitStatsOp)
        'acg_inst_noise_prepare': (STATUS, [_P, _P, _P, _P, c_float, c_float, c_int64, c_int64, c_int32, _P]),
        'acg_inst_noise_add': (STATUS, [_P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
        'acg_logit_stats': (STATUS, [_P, _P, c_int32, _P, _P]),
        # the learned latent posterior of the noise input: the reparameterised draw with its KL term, and the gradient of both
        # (ops.LatentOp / LatentBwdOp, train.Trainer posterior)
        'acg_latent_fwd': (STATUS, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P]),
        'acg_latent_bwd': (STATUS, [_P, _P, _P, _P, c_float, _P, _P, c_int32, c_int32, c_int32, _P]),
        # differentiable augmentation of the discriminator's inputs (ops.DAugmentDrawOp / DAugmentOp / DAugmentBwdOp,
        # train.Trainer d_augment): the parameter draw, the transform and its adjoint
        'acg_d_augment_draw': (STATUS, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
        'acg_d_augment_workspace_bytes': (c_int64, [c_int32] * 5),
        'acg_d_augment_fwd': (STATUS, [_P, _P, _P] + [c_int32] * 6 + [_P, c_int64, _P]),
        'acg_d_augment_bwd': (STATUS, [_P, _P, _P] + [c_int32] * 6 + [_P, c_int64, _P]),
    }),
    # BatchNorm with stored statistics: the apply pass on its own and the calibration pass that pools the moments of the batches
    # it is shown (ops.BnInferOp / BnCollectOp)
    'bn_infer': Extension('include/acgan_bn_infer.h', 'BatchNorm with stored statistics runs on the HIP library only', {
        'acg_bn_act_infer': (STATUS, [_P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_float, c_int32, c_float, c_int32, _P]),
        'acg_bn_collect_workspace_bytes': (c_size_t, [c_int64, c_int32]),
        'acg_bn_collect': (STATUS, [_P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, _P, c_size_t, _P]),
    }),
    # the exponential moving average of a scope's weights: the stand-alone update, the optimizer steps that carry it in their own
    # launch, and the in-place exchange of two flat buffers (optim.StepOp, train.Trainer.ema_weights)
    'ema': Extension('include/acgan_ema.h', 'the weight average runs on the HIP library only', {
        'acg_ema_update': (STATUS, [_P, _P, c_int64, c_float, _P, _P, _P]),
        'acg_adam_step_ema': (STATUS, [_P, _P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_float,
                                       c_int32, c_float, c_float, _P, c_float, _P, _P, _P]),
        'acg_rmsprop_step_ema': (STATUS, [_P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_int32, c_float,
                                          c_float, _P, c_float, _P, _P, _P]),
        'acg_swap_f32': (STATUS, [_P, _P, c_int64, _P]),
    }),
    # SSIM as a training loss: sum_n (1 - SSIM_n) and its gradient with respect to the prediction (ops.SsimLossOp)
    'ssim_loss': Extension('include/acgan_ssim_loss.h', 'the SSIM loss runs on the HIP library only', {
        'acg_ssim_loss_workspace_bytes': (c_size_t, [c_int32] * 4),
        'acg_ssim_loss': (STATUS, [_P, _P, _P, _P, c_float, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_float,
                                   _P, c_size_t, _P]),
    }),
    # which kernel a conv call would launch: a query for the tests (tests/conv_path_cases.py) and the tools, nothing launches
    'conv_plan': Extension('include/acgan_conv_plan.h', 'the kernel paths are those of the HIP library only', {
        'acg_conv2d_path': (STATUS, [_D, c_int32, c_int32, c_int32, ctypes.POINTER(ConvPath)]),
        'acg_conv2d_pair_path': (c_int32, [_D, c_int32, c_int32, c_int32]),
        # the process-wide switch between the uniform_k loaders of the fp32 MFMA kernels and the generic ones (same bits either way)
        'acg_conv2d_uniform_k': (STATUS, [c_int32]),
        'acg_conv2d_uniform_w': (STATUS, [c_int32]),      # the same for the weight gradients' uniform_w loaders
    }),
}


COPY_MAX = 8
REDUCE_MAX = 32
PREP_MAX = 32
NORM_SEGMENTS_MAX = 64
NOISE_DIM_MAX = 64            # acgan_rollout.h ACG_NOISE_DIM_MAX / ACG_NOISE_VALUES_MAX
NOISE_VALUES_MAX = 8192
PLAN_CANDIDATES_MAX = 1024    # acgan_rollout.h ACG_PLAN_*_MAX
PLAN_HORIZON_MAX = 16
PLAN_ACTION_DIM_MAX = 8
PLAN_STATE_DIM_MAX = 16
PLAN_PIXEL_MAPS_MAX = 4       # acgan_rollout.h ACG_PLAN_PIXEL_MAPS_MAX / ACG_PLAN_MAP_SIDE_MAX
PLAN_MAP_SIDE_MAX = 1024
DA_STREAM_TAG = 0x44415547    # acgan_rollout.h ACG_DA_STREAM_TAG / ACG_DA_ROWS_MAX / ACG_DA_COLOR, _TRANSLATION, _CUTOUT
DA_ROWS_MAX = 1024
DA_POLICY_BITS = {'color': 1, 'translation': 2, 'cutout': 4}


def dtype2(first, second):
    """ACG_DTYPE2: two storage types in one dtype argument (the plain code when they agree)."""
    return first if first == second else first | (second << 4) | 0x100


def code(torch_dtype):
    """ACG_F32 / ACG_BF16 of a torch dtype."""
    if torch_dtype == torch.float32:
        return ACG_F32
    if torch_dtype == torch.bfloat16:
        return ACG_BF16
    raise TypeError('no storage code for %s' % torch_dtype)


class AcgError(RuntimeError):
    pass


class Library:
    """A loaded C-ABI library: the core table, ``extra``, and every extension the shared object exports (``extensions``, a
    frozenset of EXTENSIONS keys; ``require`` names the ones it must).  Every STATUS entry point is checked and raises AcgError."""

    def __init__(self, path, extra=None, require=()):
        self.path = path
        self._cdll = ctypes.CDLL(path)
        sigs = dict(SIGNATURES, **(extra or {}))
        missing = [n for n in sigs if not hasattr(self._cdll, n)]
        bound = []
        for key, ext in EXTENSIONS.items():
            absent = [n for n in ext.signatures if not hasattr(self._cdll, n)]
            if key in require or len(absent) < len(ext.signatures):      # asked for, or partly there: a half-built library
                missing += absent
            if not absent:
                sigs.update(ext.signatures)
                bound.append(key)
        if missing:
            raise AcgError('%s does not export %s' % (path, ', '.join(missing)))
        self.extensions = frozenset(bound)
        for name, (res, args) in sigs.items():
            fn = getattr(self._cdll, name)
            fn.restype, fn.argtypes = (c_int32 if res is STATUS else res), args
            if res is STATUS:
                fn = self._checked(name, fn)
            setattr(self, name[4:], fn)
        if self.version() != ABI_VERSION:
            raise AcgError('%s: ABI version %d, expected %d' % (path, self.version(), ABI_VERSION))

    def _checked(self, name, fn):
        last_error = self._cdll.acg_last_error

        def call(*a):
            rc = fn(*a)
            if rc != 0:
                raise AcgError('%s failed (code %d): %s' % (name, rc, last_error().decode()))
        call.__name__ = name
        return call


def entry(lib, name):
    """``lib.<name>``, the bound entry point acg_<name> of an extension header.  ``lib`` is a Library or any stand-in for one; one
    that lacks the entry (the C oracle) is a clear error naming the header."""
    fn = getattr(lib, name, None)
    if fn is None:
        path = getattr(lib, 'path', lib)
        for ext in EXTENSIONS.values():
            if 'acg_' + name in ext.signatures:
                raise AcgError('%s does not implement acg_%s (%s): %s' % (path, name, ext.header, ext.what))
        raise AcgError('%s does not export acg_%s' % (path, name))
    return fn


_LIB = None


def get():
    """The process-wide HIP library; raises if it was not built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                '%s not found: the HIP kernels are not built and there is no fallback path. '
                'Run `python -c "import __graft_entry__ as g; g.build()"` first.' % LIB_PATH)
        _LIB = Library(LIB_PATH, require=tuple(EXTENSIONS))
    return _LIB


TUNING_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), 'libacgan_hip_tuning.so')


def load_tuning():
    """tools/ only: the -DACG_TUNING build (`make -C action_conditioned_gans_amd/csrc tuning`) with acg_debug_conv_plan
    and the ACG_* environment knobs, installed as the process's library.  The package itself never loads it."""
    global _LIB
    if not os.path.exists(TUNING_LIB_PATH):
        # never built from inside a library loader: a hidden 16-way hipcc build at call time would also run under whatever
        # preload (rocprofv3) the calling tool was started with
        raise RuntimeError('%s not found: build it first, before any profiler or GPU process starts: '
                           '`make -s -j16 -C %s tuning`' % (TUNING_LIB_PATH, os.path.dirname(LIB_PATH)))
    _LIB = Library(TUNING_LIB_PATH, extra={'acg_debug_conv_plan': (STATUS, [c_int32, c_int32])})
    return _LIB
