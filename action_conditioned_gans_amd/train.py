"""Adversarial training step and loop with the reference's Trainer / CLI surface (train.py:27-333).

``Trainer(sess, arg_adv, arg_loss, arg_opt, arg_transform)`` builds the static graph once -
placeholders, G, D(fake), D(real), losses, three optimizers, the D weight clip - and its step methods
are single ``sess.run`` calls exactly as in the reference; the session prunes each fetch to what it
needs and replays it as one HIP graph (graph.py).  Hyper-parameters the reference hard-codes as module
constants (train.py:16-25) are constructor arguments here so that the BASELINE configurations (batch
2/32/128/256, 128x128, ksize 11, n_critic) are expressible.

Reference defects resolved here: D1 `==`; D3 D actions tiled to H/4; D4 state head
optional in ``test``; D6 update -> clip; D7 eval uses its own states; D8 boolean flags accept
``--adv`` and ``--adv True|False``; D9 ksize is a parameter (default 5).
"""
import argparse
import contextlib
import json
import math
import os
import time

import numpy as np
import torch

from . import _lib
from . import graph as G
from . import models as M
from . import ops as O
from . import optim
from .metrics import frame_metrics
from .saver import Saver
from .util import build_all_mask

ADAM_LR = 1e-3          # train.py:20
RMSPROP_LR = 5e-5       # train.py:93
L2_WEIGHT = 0.05        # train.py:22
CLIP_VALUE = 0.01       # train.py:89
PRETRAIN_ITER = 20      # train.py:24
TRAIN_ITER = 60000      # train.py:25
ACTION_DIM, STATE_DIM = 10, 5


class Trainer:
    def __init__(self, sess, arg_adv, arg_loss, arg_opt, arg_transform, batch_size=64, img_size=64, ksize=5,
                 seed=0, batched_d=True, lookahead=True, num_masks=10, rollout_steps=1, bn_inference=False, ema_decay=0.0,
                 ssim_weight=0.0, g_clip_norm=0.0, d_clip_norm=0.0, grad_norms=False, noise_dim=0, noise_seed=0,
                 g_lr=None, d_lr=None, beta1=None, lr_schedule='constant', lr_warmup=0, lr_decay_steps=0, lr_final=0.0,
                 sched_sampling='off', ss_start=1.0, ss_final=0.0, ss_decay_steps=0, ss_offset=0, ss_seed=0, pixel_maps=0,
                 d_noise=0.0, d_noise_final=0.0, d_noise_decay_steps=0, d_noise_offset=0, d_noise_seed=0, d_stats=False, canvas=False,
                 posterior=False, kl_weight=1.0, d_augment=None, d_augment_seed=0):
        """``lookahead`` (no reference counterpart, off the reference's call path unless asked for): builds a second generator
        instance on a batch of 2 B - the pair (generator-step samples ; discriminator-step samples), BatchNorm statistics per half -
        that ``train_d(..., next_g=...)`` runs INSTEAD of the batch-B instance; the ``train_g`` call that follows with the announced
        inputs then finds its generator forward pass done.  The two passes read the same generator weights (the D step does not
        touch them), so this is the reference's arithmetic - one D step, then one G step (train.py:241-263) - with the two
        generator forward passes of an iteration sharing their launches at twice the GEMM height.
        ``arg_transform``: False - the plain generator; True or 'dna' - the DNA generator (the reference's ``--dna``); 'cdna' -
        the CDNA generator (models.build_generator_cdna, ``num_masks`` kernels of ``ksize``), trained with the DNA losses;
        'affine' - the affine (STP) generator (models.build_generator_affine, ``num_masks`` 2x3 transforms; ``ksize`` is not
        read), trained with the DNA losses as well.  What declines the CDNA generator declines it too: ``rollout_steps`` > 1 (no
        image gradient) and ``pixel_maps`` (no map advection through the warps).
        ``rollout_steps`` K > 1 (no reference counterpart): also builds the K-step G programs of ``train_g_rollout`` /
        ``pretrain_g_rollout`` - the generator trained through its own rollout (see there).  DNA or plain generator, float32,
        one rank; K = 1 builds nothing more.
        ``bn_inference`` (no reference counterpart; False builds nothing more): also builds a calibration instance and a
        stored-statistics instance of the generator on the same variables (_build_bn_inference) - ``calibrate_bn`` pools the
        BatchNorm moments of the batches it is shown, and ``test`` / ``test_sequence`` / ``rollout_metrics`` with ``bn='stored'``
        predict with them: a row's prediction then depends on no other row of its batch.
        ``ema_decay`` (no reference counterpart; 0 builds nothing more; else 0 < ema_decay < 1): every G parameter update -
        ``pretrain_g``, ``train_g`` and the two rollout steps - also advances ONE exponential moving average of the generator's
        weights (optim.WeightAverage: TF-1.0's ExponentialMovingAverage with its num_updates warm-up, seeded by the first
        update), inside the same program.  The average never feeds back into training: parameters, slots and frames are those of
        the run without it.  ``ema_weights()`` predicts with it; ``test`` / ``test_sequence`` / ``rollout_metrics`` take
        ``weights='ema'``.  Only the generator is averaged.  Rank-local and elementwise: allowed with every generator, with
        rollout_steps > 1, in bf16 graphs (the average is of the float32 master weights) and with more than one rank.
        ``ssim_weight`` W (no reference counterpart; 0 builds nothing more; else finite and > 0): adds W / B * sum_b (1 -
        SSIM(frame_b, next_frame_b)) to ``g_l2_loss`` - after the L2_WEIGHT scaling, not scaled by it - and so to the pretraining
        loss, the G loss and every step of the two rollout losses (ops.ssim_loss: the SSIM the evaluation reports, the gradient by
        acg_ssim_loss on the float32 frame).  The summary ``g_ssim_loss`` is the unweighted sum_b (1 - SSIM_b) / B.  L1 here is a
        sum over the 12 288 values of a frame, so a useful W is in the tens to hundreds.  Every generator, bf16 graphs (the frame
        is float32 there too), the look-ahead path, rollout_steps > 1, ema_decay and bn_inference take it; no variable and no state
        is added.  A per-frame mean over the local batch: averaging the ranks' gradients gives the global-batch value, nothing is
        needed for exact_global_batch - allowed with more than one rank, not verified there.
        ``g_clip_norm`` / ``d_clip_norm`` X (no reference counterpart; 0 builds nothing; else finite and > 0): every update of the
        generator / the discriminator first clips its averaged gradient to a global norm of X (tf.clip_by_global_norm; one
        optim.ClipNormOp in front of each StepOp of the scope - ``pretrain_g``, ``train_g`` and the two rollout steps share one
        optim.GradNorm, ``train_d`` has its own).  ``grad_norms=True`` measures the norms of a scope without a bound as well (its
        gradient is then never written).  ``grad_norm_stats(scope)`` reads the last update's norm, scale and per-variable norms;
        they are not among the summaries.  A gradient with a NaN or an infinity in it is passed on unscaled and the norm says so.
        No variable, no checkpoint key.  Every generator, bf16 graphs (the flat gradient is float32 there), the look-ahead path,
        rollout_steps > 1, ema_decay, ssim_weight and bn_inference take it; with more than one rank the clip sits behind the
        all-reduce, so every rank applies the same scale - not verified there.  ``d_clip_norm`` and the D norms need an
        adversarial trainer; with ``arg_adv=False`` they are ignored as D itself is.
        ``noise_dim`` Z (no reference counterpart; 0 builds nothing: ops, variables and state names are those of a Trainer without
        the argument; else 1 <= Z <= 64): the generator reads [action, z] with z ~ N(0, 1) [B, Z] drawn on the device inside the
        step's program (ops.append_noise, acg_noise_concat: Philox4x32-10 + Box-Muller from the graph state ``g/noise/state`` =
        {``noise_seed``, counter}, which the kernel advances - a replayed HIP graph draws fresh values with no host in the loop).
        ``g/tconv1`` (and ``g/cdna_params`` / ``g/affine_params`` of the CDNA / affine generator) get Z more input channels, drawn by their own initialiser; the
        discriminator keeps the 10-dim action.  Every generator pass draws a fresh z: ``pretrain_g``, ``train_g``, the G pass
        inside ``train_d`` and ``test``; ``last_noise()`` returns the values of the last one.  ``test`` / ``test_sequence`` /
        ``rollout_metrics`` take ``noise='zero'`` (default: z = 0, a deterministic prediction; the counter advances all the same)
        or ``'sample'``; the device rollout loop draws per step.  The state is a checkpoint key (a restored run continues its
        stream), the 0 / 1 factor that switches the noise is not.  bf16 graphs take it (the action vector is float32 there too).
        More than one rank is allowed - the rank is the stream id of the draw, so ranks draw different z from one seed - but not
        verified.  Declined here: the look-ahead pair pass is switched off for Z > 0 (as it is for rollout_steps > 1), and
        Z > 0 with ``rollout_steps`` > 1 or with ``bn_inference`` is a ValueError, as is Z outside 0..64.
        ``g_lr`` / ``d_lr`` (None: the reference's constant - 1e-3 for Adam, 5e-5 for RMSProp; else finite and > 0): the learning rate
        of every generator update (``pretrain_g``, ``train_g``, the two rollout steps) / of ``train_d``.  ``beta1`` (None: 0.9; else
        0 <= beta1 < 1): Adam's first-moment decay for all of them; with ``arg_opt='rmsprop'`` a ValueError.  Plain floats to the
        existing entries: no op, no state.
        ``lr_schedule`` 'constant' | 'linear' | 'cosine' | 'exponential', ``lr_warmup``, ``lr_decay_steps``, ``lr_final`` (no
        reference counterpart; 'constant' with ``lr_warmup=0`` builds nothing: the existing entries run, whatever the rates are):
        each scope's rate rises linearly over its first ``lr_warmup`` updates and then decays from 1 x to ``lr_final`` x the scope's
        rate over ``lr_decay_steps`` updates (optim.LrSchedule; exponential: lr_final ** (j / lr_decay_steps), not clamped).  One
        LrSchedule per scope, the same shape for G and D - ``lr_warmup`` / ``lr_decay_steps`` are counts of UPDATES and may be given
        as a pair (G's, D's) where the two scopes update at different paces - and each scope counts its own updates on the device:
        ``pretrain_g``, ``train_g`` and the two rollout steps share G's counter (so it counts the pretraining updates too),
        ``train_d`` has D's, which exists only with ``arg_adv``.  The optimizer's launch evaluates the rate itself (acg_adam_step_lr /
        acg_rmsprop_step_lr), so the replayed HIP graph of a step follows the schedule with no host in the loop; no op is added, and
        ``g/lr/updates`` / ``d/lr/updates`` are the only new checkpoint keys (a restored run continues its schedule; a checkpoint
        without them starts at 0).  Every generator, bf16 graphs (the update and the refresh of the bf16 filter copies are then two
        launches, not one), the look-ahead path, rollout_steps > 1, ema_decay, ssim_weight, the clip norms, noise and bn_inference
        take it.  With more than one rank every rank advances its own, identical counter: allowed, not verified there.
        ``learning_rates()`` reads the rates the last updates used.
        ``sched_sampling`` 'off' | 'constant' | 'linear' | 'inverse_sigmoid', ``ss_start``, ``ss_final``, ``ss_decay_steps``,
        ``ss_offset``, ``ss_seed`` (no reference counterpart; 'off' builds nothing: ops, op order, state names and checkpoint keys are
        those of a Trainer without the arguments; any other kind needs ``rollout_steps`` > 1): scheduled sampling (Bengio et al. 2015)
        of the K-step programs.  At each of the K - 1 fed-back positions a coin per sample decides whether step j reads the true
        frame t + j and state s_{t+j} (the values fed as ``rollout/next_frame{j-1}`` / ``rollout/next_state{j-1}``) or the ones step
        j - 1 predicted - frame and state under the same coin; the plain generator mixes frames only.  The probability of truth is
        ``ss_start`` ('constant'), or moves from ``ss_start`` to ``ss_final`` over ``ss_decay_steps`` K-step updates, linearly or
        along Bengio's inverse sigmoid, starting after ``ss_offset`` updates (ops.SchedSampleDrawOp; acg_sched_sample_draw has the
        formulas).  At p = 1 the program is K teacher-forced steps, at p = 0 the rollout step without the arguments (the same
        frames bit for bit).  The coins are drawn on the device inside the program - one draw per program, one select and one
        adjoint launch per fed-back position, 1 + 2 (K - 1) launches in all - from the graph state ``g/sched_sampling/state`` =
        {``ss_seed``, counter}, which the draw advances: the counter is the number of K-step updates, ``pretrain_g_rollout``'s
        included, and a replayed HIP graph draws fresh coins and moves along the schedule with no host in the loop.  The state is
        the only new checkpoint key (a restored run continues its coins and its schedule; a checkpoint without it starts at 0); no
        variable and no optimizer slot is added.  The losses of step j and its D(fake) input are built on the mixed input.
        ``sched_sampling_last()`` reads the last program's probability and coins; ``test`` / ``test_sequence`` / ``rollout_metrics``
        never sample.  A coin per batch row, not per pixel; whatever ``rollout_steps`` > 1 declines (bf16, more than one rank, the
        CDNA generator, noise) is declined here too.
        ``pixel_maps`` D (no reference counterpart; 0 builds nothing: ops, op order, state names, variables and checkpoint keys are
        those of a Trainer without the argument; else an integer in 1..4, DNA generator only): a map path through the motion model
        for plan.Planner's designated-pixel cost.  A float32 placeholder ``pixel_map`` [B, S, S, D] (float32 in bf16 graphs too, as the
        DNA image is) and, for every predicting generator instance, a twin of its DnaOp on the same logits and the same folded
        ``g/tconv4`` bias with the maps as its image (ops.dna_map_twin: acg_dna_fwd with c = D): ``g_map_out`` beside
        ``g_next_frame`` and, with ``bn_inference``, ``g_map_stored`` beside ``g_out_stored``.  No variable, no state, no kernel of
        its own; nothing but a fetch reads a twin, so the training programs, the rollout instances and the look-ahead pair do not
        contain it.  The plain generator has no flow and is a ValueError; so is the CDNA generator: its channel split, kept as
        written from the reference, transforms the colour channels of one mask with different kernels, so there is no single flow
        that a map could follow consistently with the frame.
        ``d_noise`` S, ``d_noise_final`` F, ``d_noise_decay_steps``, ``d_noise_offset``, ``d_noise_seed`` (no reference counterpart;
        S = 0 builds nothing: ops, op order, variables, state names, checkpoint keys and summaries are those of a Trainer without
        the arguments; else finite and > 0, needs ``arg_adv``): instance noise (Sonderby et al. 2016; Arjovsky & Bottou 2017) on
        every frame the discriminator judges.  D(both) - D(real) and D(fake) with ``batched_d=False`` - and the G step's D(fake) read
        a copy of their input whose channels 3..5, the judged frame, carry sigma * z with z ~ N(0, 1) per value; the conditioning
        frame in channels 0..2 is left alone (ops.InstNoiseOp, acg_inst_noise_add).  sigma moves linearly from S to F over
        ``d_noise_decay_steps`` D UPDATES that begin after ``d_noise_offset`` of them (0 steps: constant S).  The noise is drawn on
        the device inside the program: one ops.InstNoisePrepareOp per program that runs D snapshots the graph state
        ``d/inst_noise/state`` = {``d_noise_seed``, counter} as the program's key, advances the counter and evaluates sigma at
        ``d/inst_noise/updates``, which it advances in the program that holds D's optimizer step and in no other - a replayed HIP
        graph draws fresh noise and follows the schedule with no host in the loop; the G step and ``test`` draw at the current level
        and leave the schedule alone.  Every D instance has a stream id of its own (rank * 64 + slot: gen 0, real 1, both 2).  The
        two state tensors are the only new checkpoint keys (a restored run continues its key and its schedule; a checkpoint without
        them starts at 0); no variable and no optimizer slot is added.  The noise is an additive constant: the gradient of the
        generated frame is the gradient of D's noisy input.  ``d_noise_last()`` reads sigma and the key of the last program.
        float32 and bf16 graphs, every generator, ema_decay, ssim_weight, the clip norms, the lr schedules and noise_dim
        take it; more than one rank is allowed - the rank is part of the stream id - and not verified.  The look-ahead
        pair pass is switched off, as it is for noise_dim.  Declined before anything is created: ``rollout_steps`` > 1 (the K-step
        programs' D(fake) instances read no noise), ``arg_adv=False``, a negative or non-finite level.
        ``d_augment`` LIST, ``d_augment_seed`` (no reference counterpart; None or '' builds nothing: ops, op order, variables, state
        names, checkpoint keys, summaries and ``graph.collections`` are those of a Trainer without the arguments): differentiable
        augmentation (DiffAugment, Zhao et al. 2020) of every pair the discriminator judges.  LIST is a comma-separated subset of
        ``color``, ``translation``, ``cutout`` in any order.  D(both) - D(real) and D(fake) with ``batched_d=False`` - and the G
        step's D(fake) read a transformed copy of their 6-channel input, both frames of a row under the same parameters, the
        rows (the fake and the real row of a sample too) under independent ones (ops.DAugmentOp, acg_d_augment_fwd), and G's
        gradient goes back through the transform's adjoint (ops.DAugmentBwdOp).  The parameters are drawn on the device inside
        the program, one ops.DAugmentDrawOp per D instance (stream id rank * 64 + slot: gen 0, real 1, both 2) from the graph
        state ``d/augment/state`` = {``d_augment_seed``, counter}; every program that runs a D instance runs its draw once - the
        D step, the G step and the summaries alike - so the counter counts draws.  That state is the only new checkpoint key (a
        checkpoint without it starts at 0); no variable, optimizer slot or summary is added.  With ``d_noise`` the noise is
        added to the augmented input.  ``d_augment_last()`` reads the parameters of the last program, ``d_augment_state()`` the
        state.  The look-ahead pair pass is switched off, as it is for ``d_noise``.  Declined before anything is created
        (check_d_augment): an unknown or repeated name, ``rollout_steps`` > 1, ``arg_adv=False``, a bf16 graph.  More than one
        rank is allowed - the rank is part of the stream id - and not verified.
        ``d_stats=True`` (False adds nothing): the summaries ``d_fake_logit`` / ``d_real_logit`` - the mean logit of D on the
        generated and on the real half - and ``d_fake_acc`` / ``d_real_acc`` - the share of fake logits < 0 and of real logits > 0 -
        computed on the device from the logits the D loss reads (ops.LogitStatsOp), and with ``d_noise`` > 0 ``d_noise_sigma``, the
        level of the program that computed them.
        ``canvas=True`` (no reference counterpart; False builds nothing: ops, variables and checkpoint keys are those of a Trainer
        without the argument; CDNA and affine generators, ``num_masks`` <= 31): every generator instance paints an image of its own
        from its decoder (``g/tconv4_canvas``, 5x5/2 deconvolution + bias + tanh) and composites it as one more candidate behind the
        M moved images, under channel M + 1 of then M + 2 mask logits (models._mask_generator; acg_*_composite_canvas_*) - a
        pixel that no pixel of the input frame can colour has a candidate.  ``g/tconv4/*`` has M + 2 output channels and
        ``g/tconv4_canvas/*`` is new, with their optimizer and average slots: a checkpoint of one setting does not restore into
        the other.  Everything these generators take they take with it (the look-ahead pair pass, HIP-graph replay, noise_dim,
        ema_decay, ssim_weight, the clip norms, the schedules, bn_inference), and what they decline stays declined.  A generator
        without masks (plain, DNA) is a ValueError before anything is created.

        ``posterior`` / ``kl_weight`` W (no reference counterpart; False builds nothing: ops, op order, variables, state names and
        summaries are those of a Trainer without the arguments; needs ``noise_dim`` Z > 0): the VAE half of a VAE-GAN (SV2P,
        Babaeizadeh et al. 2018; SAVP, Lee et al. 2018).  Nothing in L1 + GDL + the adversarial term ties z to the frame, so a
        generator that ignores its noise input minimises them.  With ``posterior`` an encoder under scope ``g/posterior``
        (models.build_posterior) sees (x_t, x_{t+1}) and emits mu, logvar; the generator reads z = mu + exp(logvar / 2) * eps -
        eps the draw of ``noise_dim``, from the same ``g/noise/state`` - and  W / B * KL(q(z | x_t, x_{t+1}) || N(0, 1))  joins
        the G loss AND the pretraining loss (ops.append_latent: one launch forward, one backward for the generator's gradient
        and the KL gradient together).  The encoder's variables are the generator's to the optimizers, the weight average, the
        clip norm and the lr schedule.  The summary ``g_kl`` is KL / B.  The training steps run with the posterior;
        ``test`` / ``test_sequence`` / ``rollout_metrics`` take ``noise`` in NOISE_MODES: 'zero' (z = 0) and 'sample' (z ~ N(0, 1),
        the prior) as before, 'posterior' (z ~ q) and 'posterior_mean' (z = mu), which encode the frames the placeholders
        hold - the current input frame and the fed next frame.  The mode is a device-side float32 [2] written between programs,
        only when it changes.  New checkpoint keys are the ``g/posterior/*`` variables and their optimizer slots: a posterior
        checkpoint restores into a plain ``noise_dim`` Trainer (the Saver ignores extra keys), a plain one into a posterior
        Trainer is refused (it lacks variables).  Declined before anything is created (check_posterior): no ``noise_dim``, a
        bf16 graph (the action gradient is float32 only), a negative or non-finite ``kl_weight``; ``rollout_steps`` > 1 and
        ``bn_inference`` are ``noise_dim``'s refusals.  More than one rank is allowed and not verified (the stream id is the rank)."""
        self.canvas =check_canvas(canvas, model_kind(arg_transform), ksize, num_masks)      # (before anything is created)
        self.d_noise = check_d_noise(d_noise, d_noise_final, d_noise_decay_steps, d_noise_offset, d_noise_seed, rollout_steps,
                                     arg_adv)         # (before anything is created; None: off)
        self.d_augment = check_d_augment(d_augment, d_augment_seed, rollout_steps, arg_adv,
                                         bf16=G.get_default_graph().act_dtype != torch.float32)      # (the same)
        self.pixel_maps = check_pixel_maps(pixel_maps, model_kind(arg_transform))      # (before anything is created)
        self.lr_args = check_lr(g_lr, d_lr, beta1, arg_opt, lr_schedule, lr_warmup, lr_decay_steps, lr_final)   # (before anything is created)
        self.noise_dim = check_noise(noise_dim, noise_seed, rollout_steps, bn_inference, batch_size)        # (before anything is created)
        self.posterior, self.kl_weight = check_posterior(posterior, kl_weight, self.noise_dim,
                                                         bf16=G.get_default_graph().act_dtype != torch.float32)      # (the same)
        self.sched_sampling = check_sched_sampling(sched_sampling, ss_start, ss_final, ss_decay_steps, ss_offset, ss_seed, rollout_steps,
                                                   batch_size)      # (None: off)
        self.ema_decay = ema_decay = check_ema_decay(ema_decay)         # (before anything is created)
        self.ssim_weight = check_ssim_weight(ssim_weight)
        self.g_clip_norm, self.d_clip_norm = check_clip_norm(g_clip_norm, 'g_clip_norm'), check_clip_norm(d_clip_norm, 'd_clip_norm')
        grad_norms = bool(grad_norms)
        self.sess = sess
        self.model = model_kind(arg_transform)
        dp = G.get_default_graph().collections.get('data_parallel')
        self.rollout_steps = check_rollout(rollout_steps, self.model, bf16=G.get_default_graph().act_dtype != torch.float32,
                                           data_parallel=dp is not None and (dp.active or dp.sync_bn))
        self.num_masks = num_masks
        self.batch_size, self.img_size, self.ksize = batch_size, img_size, ksize
        self.arg_adv, self.arg_loss, self.arg_opt, self.arg_transform = arg_adv, arg_loss, arg_opt, arg_transform
        if arg_loss not in ('bce', 'wass'):
            raise ValueError('unexpected loss argument')
        B, S = batch_size, img_size
        O.set_random_seed(seed)

        self.img_ph = G.placeholder((B, S, S, 3), name='current_frame')
        # the same frames with a channel pitch of 4 (zero pad channel): lets g/conv1 gather with 16-byte loads
        self.img_ph.padded = self._img_pad = G.placeholder((B, S, S, 3), name='current_frame_conv', channel_pitch=O.cpad(3), act=True)
        self.next_frame_ph = G.placeholder((B, S, S, 3), name='next_frame')
        self.action_ph = G.placeholder((B, ACTION_DIM), name='action')
        self.next_state = G.placeholder((B, STATE_DIM), name='next_state')

        # generator (train.py:52-61); the action tile + concat is fused inside the model builders
        graph = G.get_default_graph()
        dp = graph.collections.get('data_parallel')
        # (synchronised BatchNorm builds other ops per layer and is a validation mode: it keeps the plain call path)
        self.lookahead = bool(lookahead) and batched_d and not (dp is not None and dp.active and dp.sync_bn) and not self.noise_dim \
            and self.d_noise is None and self.d_augment is None
        self._noise = None            # the [B, 10 + Z] vector the generator reads (noise_dim > 0)

        self._kl = None               # KL(q || N(0, 1)) summed over the batch, a Scalar (posterior)

        def build_g(images, actions, batch, reuse):
            if self.posterior:
                # the encoder reads (x_t, x_{t+1}) as the discriminator reads its real pairs: 6 channels at a pitch of 8
                O.latent_state(noise_seed)
                pair = O.concat([self.img_ph, self.next_frame_ph], axis=3, name='posterior_in', pitch=8, act=True)
                actions, self._kl = O.append_latent(actions, M.build_posterior(pair, self.noise_dim, reuse=reuse))
                self._noise = actions
            elif self.noise_dim:
                O.noise_state(noise_seed)
                actions = self._noise = O.append_noise(actions, self.noise_dim)
            return M.KINDS[self.model].build_with(images, actions, batch, reuse, ksize, num_masks, self.canvas)
        n0 = len(graph.ops)
        self.g_out, self.g_state_out = build_g(self.img_ph, self.action_ph, B, False)
        n1 = len(graph.ops)
        self.g_next_frame = self.g_out
        self.pair_img_ph = self.pair_action_ph = self._g_pair_out = None
        self._stash_copy, self._g_extra = None, []
        if self.lookahead:
            # the pair instance: rows [0, B) = the samples of the G step that follows, rows [B, 2 B) = this D step's samples
            self.pair_img_ph = G.placeholder((2 * B, S, S, 3), name='frame_pair')
            self.pair_img_ph.padded = self._pair_img_pad = G.placeholder((2 * B, S, S, 3), name='frame_pair_conv', channel_pitch=O.cpad(3), act=True)
            self.pair_action_ph = G.placeholder((2 * B, ACTION_DIM), name='action_pair')
            with O.arg_scope([O.batch_norm], groups=2):
                self._g_pair_out, _ = build_g(self.pair_img_ph, self.pair_action_ph, 2 * B, True)
            # every tensor of the batch-B instance IS the first half of its twin in the pair instance: what the pair pass
            # computes for the G step's samples is exactly what that step's backward pass reads
            self._g_ops, g_pair_ops = graph.ops[n0:n1], graph.ops[n1:len(graph.ops)]
            _alias_first_half(self._g_ops, g_pair_ops)

        # discriminator on (x_t, fake) then (x_t, real), sharing variables (train.py:63-70).
        # batched_d: the D step runs D ONCE on [fake ; real] stacked along the batch, BatchNorm statistics kept
        # per half (groups=2) - arithmetically the two reference calls, at twice the GEMM height and half the
        # launches.  The G step still uses the batch-B D(fake) graph (D(real) is pruned there anyway).
        self._pair_concat = None
        if batched_d:
            # ONE buffer of 3 B discriminator inputs [spare ; generated ; real], 6 channels at a pitch of 8 (16-byte gathers in
            # d/conv1): D(both) reads rows [B, 3 B), D(fake) rows [B, 2 B); the pair generator writes rows [0, 2 B) - its second
            # half, the D step's samples, lands where D(both) expects the generated frames
            n_part = B * S * S * 8
            d_in_all = O._new_act((3 * B, S, S, 8), 'd_in_all:0')
            win = lambda k, rows, name: d_in_all.view(k * n_part, (rows, S, S, 8), name=name)     # noqa: E731
            d_in_gen = O.concat([self.img_ph, self.g_next_frame], axis=3, name='d_in_gen', out=win(1, B, 'd_in_all/gen'), pitch=8, act=True)
            d_in_real = O.concat([self.img_ph, self.next_frame_ph], axis=3, name='d_in_real', out=win(2, B, 'd_in_all/real'), pitch=8, act=True)
            d_in_both = win(1, 2 * B, 'd_in_both:0')
            O.JoinOp([d_in_gen, d_in_real], d_in_both, 'd_in_both')
            d_in_both.valid_c = d_in_gen.valid_c
            self._stash_copy = None
            if self.lookahead:
                self._pair_concat = O.concat([self.pair_img_ph, self._g_pair_out], axis=3, name='d_in_pair', out=win(0, 2 * B, 'd_in_all/pair'),
                                             pitch=8, act=True).op
                if self._pair_concat.by_producer:
                    # the pair's DNA kernel writes whole discriminator-input pixels into rows [0, 2 B): the G step's own frames sit
                    # in the spare rows [0, B) afterwards, and the G step moves them to rows [B, 2 B) with one copy
                    self._stash_copy = O.CopyRowsOp(win(0, B, 'd_in_all/spare'), win(1, B, 'd_in_all/gen_copy'), 'd_in_gen/from_pair')
        else:
            d_in_gen = O.concat([self.img_ph, self.g_next_frame], axis=3, name='d_in_gen', pitch=8, act=True)
            d_in_real = O.concat([self.img_ph, self.next_frame_ph], axis=3, name='d_in_real', pitch=8, act=True)
        # what the D instances read: their inputs, or (d_augment) a transformed and / or (d_noise) a noisy copy each - the noise
        # behind the augmentation - drawn under the instance's own stream id
        d_x_gen, d_x_real, d_x_both = d_in_gen, d_in_real, d_in_both if batched_d else None
        self._d_augment_params = {}           # slot name -> the params tensor of that D instance's draw (d_augment)
        if self.d_augment is not None:
            da = self.d_augment
            O.d_augment_state(da['seed'])

            def augmented(t, slot, name):
                draw = O.DAugmentDrawOp(t.shape[0], S, S, da['policy'], D_SLOTS[slot], name + '/draw')
                self._d_augment_params[slot] = draw.params
                return O.DAugmentOp(t, draw.params, 2, 3, name).outputs[0]
            d_x_gen = augmented(d_in_gen, 'gen', 'd_in_gen/augmented')
            if batched_d:
                d_x_both = augmented(d_in_both, 'both', 'd_in_both/augmented')
            else:
                d_x_real = augmented(d_in_real, 'real', 'd_in_real/augmented')
        self._d_noise_prep, self.d_noisy = None, {}
        if self.d_noise is not None:
            dn = self.d_noise
            O.inst_noise_state(dn['seed'])
            prep = self._d_noise_prep = O.InstNoisePrepareOp(dn['start'], dn['final'], dn['decay_steps'], dn['offset'], 0, 'd/inst_noise/prepare')
            noisy = lambda t, slot, name: O.InstNoiseOp(t, prep.key, prep.sigma, 3, 3, slot, name).outputs[0]     # noqa: E731
            d_x_gen = self.d_noisy['gen'] = noisy(d_x_gen, 0, 'd_in_gen/noisy')
            if batched_d:
                d_x_both = self.d_noisy['both'] = noisy(d_x_both, 2, 'd_in_both/noisy')
            else:
                d_x_real = self.d_noisy['real'] = noisy(d_x_real, 1, 'd_in_real/noisy')
        self.d_out_gen = M.build_discriminator(d_x_gen, self.action_ph, reuse=False)
        if batched_d:
            with O.arg_scope([O.batch_norm], groups=2):
                self.d_out_both = M.build_discriminator(d_x_both, O.repeat_batch(self.action_ph, 2), reuse=True)
            self.d_out_real = self.d_out_both.view(self.d_out_gen.numel, self.d_out_gen.shape, name='d_out_real')
        else:
            self.d_out_both = None
            self.d_out_real = M.build_discriminator(d_x_real, self.action_ph, reuse=True)

        # losses (train.py:72-85)
        self.g_psnr = O.build_psnr(self.next_frame_ph, self.g_next_frame)
        self.summaries = {}
        g_l2_loss, self.g_ssim_loss, adv_loss, self.g_loss = self._step_losses(self.g_out, self.g_state_out, self.next_frame_ph, self.next_state,
                                                                               self.d_out_gen, '', mean_ssim=True)
        if self._kl is not None:
            # the ELBO's KL term, per sample like the L1 term it stands against: in the G loss and in the pretraining loss
            kl_term = self._kl * (self.kl_weight / B)
            g_l2_loss, self.g_loss = g_l2_loss + kl_term, self.g_loss + kl_term
            self.summaries['g_kl'] = self._kl / B
        self.g_l2_loss = g_l2_loss
        if self.g_ssim_loss is not None:
            self.summaries['g_ssim_loss'] = self.g_ssim_loss
        if arg_adv:
            self.g_adv_loss = self.summaries['g_adv_loss'] = adv_loss
        if batched_d:
            self.d_loss = O.build_d_loss_batched(self.d_out_both, arg_loss, summaries=self.summaries)
        else:
            self.d_loss = O.build_d_loss(self.d_out_real, self.d_out_gen, arg_loss, summaries=self.summaries)
        if d_stats:
            # on the logits the D loss reads: the first half of D(both), or D(fake) of the two-instance D step
            fake = self.d_out_both.view(0, self.d_out_gen.shape, name='d_out_fake') if batched_d else self.d_out_gen
            stats = O.LogitStatsOp(fake, self.d_out_real, 'd_stats').outputs[0]
            for k, name in enumerate(('d_fake_logit', 'd_real_logit', 'd_fake_acc', 'd_real_acc')):
                self.summaries[name] = stats.view(k, (1,), name='d_stats/' + name)
            if self._d_noise_prep is not None:
                self.summaries['d_noise_sigma'] = self._d_noise_prep.sigma

        graph = G.get_default_graph()
        self.g_vars = graph.trainable_variables('g')
        self.d_vars = graph.trainable_variables('d')
        self.clip_d = [optim.clip_by_value_assign(p, -CLIP_VALUE, CLIP_VALUE) for p in self.d_vars]

        la = self.lr_args
        if arg_opt == 'rmsprop':
            make = lambda name: optim.RMSPropOptimizer(la['d_lr' if name.startswith('d_') else 'g_lr'], name=name)
        elif arg_opt == 'adam':
            adam_kw = {} if la['beta1'] is None else {'beta1': la['beta1']}
            make = lambda name: optim.AdamOptimizer(la['d_lr' if name.startswith('d_') else 'g_lr'], name=name, **adam_kw)
        else:
            raise ValueError('unexpected opt argument')
        # scope -> the optim.LrSchedule every update of the scope shares (None: the scope's rate is its constant)
        self.lr_sched = {'g': None, 'd': None}
        if la['scheduled']:
            for k, scope in enumerate('gd' if arg_adv else 'g'):
                self.lr_sched[scope] = optim.LrSchedule(la['schedule'], scope, la['warmup'][k], la['decay_steps'][k], la['final'])
        g_sched, d_sched = self.lr_sched['g'], self.lr_sched['d']
        self.ema = optim.WeightAverage(ema_decay, 'g') if ema_decay else None      # shared by every G update of this Trainer
        self._ema_swapped = False
        # scope -> the optim.GradNorm every update of the scope shares (None: neither clipped nor measured)
        self.grad_norm = {'g': optim.GradNorm(self.g_clip_norm or math.inf, 'g') if self.g_clip_norm or grad_norms else None,
                          'd': optim.GradNorm(self.d_clip_norm or math.inf, 'd') if arg_adv and (self.d_clip_norm or grad_norms) else None}
        g_norm, d_norm = self.grad_norm['g'], self.grad_norm['d']

        def minimize_g(name, loss, slots_of=None):       # every G update: the same variables, average, clip and schedule
            return make(name).minimize(loss, var_list=self.g_vars, slots_of=slots_of, ema=self.ema, clip_norm=g_norm, lr_schedule=g_sched)
        self.g_opt_op = minimize_g('g_opt', self.g_loss)
        self.g_pretrain_opt_op = minimize_g('g_pretrain_opt', g_l2_loss)
        self.d_opt_op = make('d_opt').minimize(self.d_loss, var_list=self.d_vars, clip_norm=d_norm, lr_schedule=d_sched)
        if self._d_noise_prep is not None:
            self._d_noise_prep.advance_schedule = self.d_opt_op      # sigma's schedule counts D updates: the D step's program alone

        # the seven tf.summary scalars of ops.py:48-49 / train.py:104-111, names kept
        self.summaries.update({'discriminator_loss': self.d_loss, 'g_loss': self.g_loss, 'g_l2_loss': g_l2_loss,
                               'g_psnr': self.g_psnr})
        self._summary_names = sorted(self.summaries)
        self.merged_summaries = [self.summaries[k] for k in self._summary_names]
        self._zero_state = np.zeros((B, STATE_DIM), np.float32)
        self._announced = None          # (images, actions) of the G step a look-ahead D step has prepared
        self._noise_on = None           # the mode of the noise as last written (_noise_switch; None: not yet)
        self._skip_d = self._skip_g = None
        if self.rollout_steps > 1:
            self._build_rollout(build_g, minimize_g)
        if self.lookahead:
            # what the pair pass replaces.  D step: the whole batch-B generator and the launch that puts its frame into D's input.
            # G step: the generator up to and including the frame (an alias of the pair's first half) and, where the DNA kernel
            # wrote the discriminator-input pixels too, the concatenation: those pixels are copied over from the spare rows
            trunk = _ancestors(self.g_out, set(map(id, self._g_ops)))
            self._skip_d = frozenset(trunk + [d_in_gen.op])
            if self._stash_copy is not None:        # DNA generator: the frame AND its copy in D(fake)'s input exist already (one 4 MB copy)
                self._skip_g, self._g_extra = frozenset(trunk + [d_in_gen.op]), [self._stash_copy]
            else:                                   # plain generator: its concat launch puts the (aliased) frame into D(fake)'s input as usual
                self._skip_g, self._g_extra = frozenset(trunk), []
        self.bn_inference = bool(bn_inference)
        if self.bn_inference:
            self._build_bn_inference(build_g)
        self.pixel_map_ph = self.g_map_out = self.g_map_stored = None
        if self.pixel_maps:
            # behind every generator instance, the look-ahead pair's alias walk and the rollout: the twins are nobody's ancestors
            self.pixel_map_ph = G.placeholder((B, S, S, self.pixel_maps), name='pixel_map')
            self.g_map_out = O.dna_map_twin(self.g_out.op, self.pixel_map_ph, 'g_map')
            if self.bn_inference:
                self.g_map_stored = O.dna_map_twin(self.g_out_stored.op, self.pixel_map_ph, 'g_map_stored')
        if self.ema is not None:
            self.ema.build()        # last: every op of the graph keeps the place it has without the average
        for norm in self.grad_norm.values():
            if norm is not None:
                norm.build()        # (the same: after everything else)
        for sched in self.lr_sched.values():
            if sched is not None:
                sched.build()       # (and the schedules' counters last of all)

    # ---- learning rates (g_lr / d_lr / lr_schedule)
    def learning_rates(self):
        """-> {'g': {'lr', 'updates'}, 'd': {...}}: the rate the last update of the scope used, as the float32 the kernel read, and
        the scope's update counter.  A scope without a schedule reports its constant and ``updates`` None (it keeps no counter); a
        scheduled scope reports 0.0 before its first update.  One small device-to-host copy per scheduled scope and value (a
        synchronisation)."""
        out = {}
        for scope in ('g', 'd'):
            sched = self.lr_sched[scope]
            if sched is None:
                out[scope] = {'lr': float(np.float32(self.lr_args[scope + '_lr'])), 'updates': None}
            else:
                out[scope] = {'lr': float(self.sess._materialize(sched.lr).item()), 'updates': int(self.sess._materialize(sched.updates).item())}
        return out

    # ---- the generator's noise input (noise_dim > 0)
    def _noise_switch(self, on, always=False):
        """Write the mode of the noise the next generator pass reads (outside the programs, on their stream): ``on`` is True -
        what the training steps read: the posterior where there is one, else the prior - or one of NOISE_MODES.  Without
        ``posterior`` that is the 0 / 1 factor of ops.noise_state, with it the {scale, posterior} pair of ops.latent_state.  The
        training steps write only when something else was written last; a predicting call always writes (the initializer, run
        again, resets the value behind this object's back)."""
        mode = ('posterior' if self.posterior else 'sample') if on is True else 'zero' if on is False else on
        if self.noise_dim and (always or mode != self._noise_on):
            scale, post = NOISE_MODES[mode]
            if self.posterior:
                buf = self.sess._materialize(O.latent_state()[1])
                buf[0:1].fill_(scale)
                buf[1:2].fill_(post)
            else:
                self.sess._materialize(O.noise_state()[1]).fill_(scale)
            self._noise_on = mode

    def last_noise(self):
        """-> [B, noise_dim] float32: the z the last generator pass read (zeros after a ``noise='zero'`` pass, and before the
        first pass).  One small device-to-host copy (a synchronisation)."""
        if not self.noise_dim:
            raise RuntimeError('this Trainer was built without noise_dim: its generator reads no noise')
        return self.sess._materialize(self._noise).detach()[:, ACTION_DIM:].cpu().numpy().copy()

    def noise_state(self):
        """-> (seed, counter) of ``g/noise/state`` as Python ints in [0, 2^64): the counter is the number of draws so far."""
        if not self.noise_dim:
            raise RuntimeError('this Trainer was built without noise_dim: it keeps no noise state')
        return O.read_draw_state(self.sess._materialize(O.noise_state()[0]))

    def set_noise_state(self, seed, counter=0):
        """Restart the noise stream at (seed, counter): the draws that follow are those of a fresh Trainer built with that seed
        after ``counter`` generator passes."""
        if not self.noise_dim:
            raise RuntimeError('this Trainer was built without noise_dim: it keeps no noise state')
        seed, counter = check_noise_seed(seed), check_noise_seed(counter)
        O.write_draw_state(self.sess._materialize(O.noise_state()[0]), seed, counter)
        self._announced = None

    # ---- instance noise on the discriminator's inputs (d_noise > 0)
    def _require_d_noise(self):
        if self.d_noise is None:
            raise RuntimeError('this Trainer was built without d_noise: its discriminator reads no instance noise')

    def d_noise_last(self):
        """-> {'sigma': the level the last program that ran D used (the float32 the kernel read), 'key': (seed, counter) that
        program drew from}; sigma 0.0 and key (0, 0) before the first one.  Two small device-to-host copies (a synchronisation)."""
        self._require_d_noise()
        prep = self._d_noise_prep
        return {'sigma': float(self.sess._materialize(prep.sigma).item()), 'key': O.read_draw_state(self.sess._materialize(prep.key))}

    def d_noise_state(self):
        """-> (seed, counter, updates) of ``d/inst_noise/state`` and ``d/inst_noise/updates`` as Python ints: the number of draws
        and the schedule position (the number of D updates) so far."""
        self._require_d_noise()
        state, updates = O.inst_noise_state()
        return O.read_draw_state(self.sess._materialize(state)) + (int(self.sess._materialize(updates).item()) % 2 ** 64,)

    # ---- differentiable augmentation of the discriminator's inputs (d_augment)
    def _require_d_augment(self):
        if self.d_augment is None:
            raise RuntimeError('this Trainer was built without d_augment: its discriminator reads no augmented input')

    def d_augment_last(self):
        """-> {slot name ('gen', 'real', 'both'): params float32 [rows, 8] as numpy} - the parameters every D instance's draw
        holds: those of the last program that ran the instance (zeros before the first).  One device-to-host copy per
        instance (a synchronisation)."""
        self._require_d_augment()
        return {slot: self.sess._materialize(t).detach().cpu().numpy().copy() for slot, t in self._d_augment_params.items()}

    def d_augment_state(self):
        """-> (seed, counter) of ``d/augment/state`` as Python ints in [0, 2^64): the counter is the number of draws so far."""
        self._require_d_augment()
        return O.read_draw_state(self.sess._materialize(O.d_augment_state()))

    # ---- scheduled sampling of the K-step programs (sched_sampling != 'off')
    def _require_sched_sampling(self):
        if self.sched_sampling is None:
            raise RuntimeError("this Trainer was built with sched_sampling='off': its K-step programs draw no coins")

    def sched_sampling_last(self):
        """-> {'prob': the probability of truth the last K-step program used (the float32 the kernel compared with), 'mask': bool
        [K - 1, B], True where step j + 1 read the truth at position j}; prob 0.0 and no truth before the first program.  One
        device-to-host copy of both (a synchronisation)."""
        self._require_sched_sampling()
        vals = torch.cat([self.sess._materialize(self._ss_prob).detach().reshape(-1),
                          self.sess._materialize(self._ss_mask).detach().reshape(-1)]).cpu().numpy()
        return {'prob': float(vals[0]), 'mask': (vals[1:] != 0).reshape(self._ss_mask.shape)}

    def sched_sampling_state(self):
        """-> (seed, counter) of ``g/sched_sampling/state`` as Python ints in [0, 2^64): the counter is the number of K-step
        updates so far."""
        self._require_sched_sampling()
        return O.read_draw_state(self.sess._materialize(O.sched_sampling_state()))

    def set_sched_sampling_state(self, seed, counter=0):
        """Restart the coins at (seed, counter): the K-step updates that follow draw what a fresh Trainer built with that seed
        draws after ``counter`` updates, at the schedule's value there."""
        self._require_sched_sampling()
        seed, counter = check_noise_seed(seed, 'seed'), check_noise_seed(counter, 'counter')
        O.write_draw_state(self.sess._materialize(O.sched_sampling_state()), seed, counter)

    # ---- gradient norms (g_clip_norm / d_clip_norm / grad_norms)
    def grad_norm_stats(self, scope):
        """-> {'norm', 'scale', 'per_variable': {variable name: norm}} of the last update of ``scope`` ('g' or 'd') that ran: the
        global norm of the averaged gradient, the factor it was multiplied by (1: it fitted, or it was not finite, or the scope
        is measured only) and each variable's norm BEFORE scaling.  All zero before the first update.  One small device-to-host
        copy (a synchronisation).  Raises when the Trainer keeps no GradNorm for the scope."""
        if scope not in self.grad_norm:
            raise ValueError("grad_norm_stats: scope must be 'g' or 'd', got %r" % (scope,))
        norm = self.grad_norm[scope]
        if norm is None:
            raise RuntimeError('this Trainer was built without %s_clip_norm / grad_norms%s: it measures no gradient norm of scope %r'
                               % (scope, ' (or without arg_adv)' if scope == 'd' else '', scope))
        vals = [float(v) for v in self.sess._materialize(norm.stats).detach().cpu().numpy()]
        return {'norm': vals[0], 'scale': vals[1], 'per_variable': dict(zip(norm.names, vals[2:]))}

    # ---- the generator's weight average (ema_decay > 0)
    def _require_ema(self):
        if self.ema is None:
            raise RuntimeError('this Trainer was built without ema_decay: it keeps no average of the generator weights')

    def ema_updates(self):
        """Updates the average has seen (0: the shadow holds nothing yet); reads the device-side counter."""
        self._require_ema()
        return int(self.sess._materialize(self.ema.num_updates).item())

    def ema_statistics(self):
        """-> {variable name: numpy array}: the averaged value of every generator variable (the shadow buffer by ``layout``)."""
        self._require_ema()
        offsets = self.ema.graph.layout('g')[0]
        shadow = self.sess._materialize(self.ema.shadow).detach().cpu().numpy()
        return {v.name: shadow[offsets[v.name]:offsets[v.name] + v.numel].reshape(v.shape).copy() for v in self.g_vars}

    def reset_ema(self):
        """Counter back to 0: the next G update seeds the shadow with the weights it leaves."""
        self._require_ema()
        self.sess._materialize(self.ema.num_updates).zero_()

    def _ema_buffers(self):
        self._require_ema()
        if self.ema_updates() < 1:
            raise RuntimeError('the weight average has seen 0 updates: there are no averaged weights to predict with')
        flat = self.ema.graph.layout('g')[2]
        return self.sess._materialize(flat), self.sess._materialize(self.ema.shadow)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the generator's variables hold the averaged weights and the shadow holds the raw ones: ONE launch
        exchanges the two flat buffers (programs are captured with their pointers, so the data moves), and a bf16 session
        refreshes its filter copies before its next program.  On exit they are exchanged back, bit for bit.  Predict inside;
        a G update inside would train the average and average the training weights.  Raises when the Trainer keeps no average
        or it has seen no update."""
        flat, shadow = self._ema_buffers()
        if self._ema_swapped:
            raise RuntimeError('ema_weights() is already entered')
        swap = _lib.entry(self.sess.rt.lib, 'swap_f32')
        args = (optim._p(flat), optim._p(shadow), flat.numel())

        def exchange():
            swap(*args, self.sess.rt.stream_ptr())
            self.sess._weights_dirty = True
            self._announced = None           # (a prepared generator pass was computed with the other weights)
        exchange()
        self._ema_swapped = True
        try:
            yield self
        finally:
            exchange()
            self._ema_swapped = False

    def load_ema_weights(self):
        """COPY the averaged weights into the generator's variables (the shadow keeps them too): what a session that only
        predicts wants - a checkpoint saved afterwards restores to the same weights whichever of the two it reads."""
        flat, shadow = self._ema_buffers()
        flat.copy_(shadow)
        self.sess._weights_dirty = True
        self._announced = None

    @contextlib.contextmanager
    def _predicting(self, bn='batch', weights='raw', noise='zero', switch=True):
        """The mode of a predicting call (``test``, ``test_sequence``, ``rollout_metrics``, plan.Planner).  Every argument is
        checked before anything is launched; then, for ``weights='ema'``, the body runs inside ``ema_weights()``, a prepared
        generator pass is dropped and the noise switch is written as ``noise`` says (``switch=False``: checked only - the caller
        has checks of its own to make first, and the ``test`` it goes on to call writes it).  Yields whether the
        stored-statistics instance predicts."""
        if weights not in ('raw', 'ema'):
            raise ValueError("weights must be 'raw' or 'ema', got %r" % (weights,))
        if weights == 'ema':
            self._require_ema()
        if bn not in ('batch', 'stored'):
            raise ValueError("bn must be 'batch' or 'stored', got %r" % (bn,))
        if bn == 'stored':
            self._require_calibrated()
        if noise not in NOISE_MODES:
            raise ValueError("noise must be 'zero', 'sample', 'posterior' or 'posterior_mean', got %r" % (noise,))
        if noise == 'sample' and not self.noise_dim:
            raise RuntimeError("noise='sample': this Trainer was built without noise_dim, its generator reads no noise")
        if NOISE_MODES[noise][1] and not self.posterior:
            raise RuntimeError('noise=%r: this Trainer was built without posterior, it has no encoder to draw from' % (noise,))
        with self.ema_weights() if weights == 'ema' else contextlib.nullcontext():
            self._announced = None
            if switch:
                self._noise_switch(noise, always=True)
            yield bn == 'stored'

    def _build_bn_inference(self, build_g):
        """Two more generator instances on the existing variables and placeholders (the modes arrive through the arg scope of
        ops.batch_norm, as slim's ``is_training`` does).  Calibration: the generator as it runs today, batch statistics in every
        layer, each BatchNorm layer also pooling the moments of its input rows into its stored statistics
        (``g/<layer>/BatchNorm/moving_mean`` / ``moving_variance`` / ``calibration_rows``: graph state, in no variable list and no
        optimizer).  Stored: every BatchNorm layer applies those statistics."""
        graph = G.get_default_graph()
        dp = graph.collections.get('data_parallel')
        if dp is not None and (dp.active or dp.sync_bn):
            raise ValueError('bn_inference runs on one rank (no data parallelism, sync_bn or exact_global_batch)')
        B = self.batch_size
        n_before = len(graph.collections.get('bn_collect', []))
        with O.arg_scope([O.batch_norm], collect_statistics=True):
            build_g(self.img_ph, self.action_ph, B, True)
        self._bn_collect_ops = list(graph.collections['bn_collect'][n_before:])
        with O.arg_scope([O.batch_norm], is_training=False):
            self.g_out_stored, self.g_state_stored = build_g(self.img_ph, self.action_ph, B, True)
        self._stored_psnr = O.build_psnr(self.next_frame_ph, self.g_out_stored)
        # scope -> (mean, variance, rows) of this generator's layers, in layer order
        self._bn_state = {op.name[:-len('/collect')]: tuple(op.extras) for op in self._bn_collect_ops}
        first = self._bn_collect_ops[0]
        self._bn_rows_per_sample = first.rows // B          # layer rows (B * h * w positions) of the first layer per batch row
        self._bn_calibrated = False

    def _require_bn_inference(self):
        if not self.bn_inference:
            raise RuntimeError("this Trainer was built without bn_inference=True: it has no stored BatchNorm statistics")

    def bn_calibration_rows(self):
        """Batch rows (frame / action pairs) pooled into the stored statistics so far; reads the device-side count."""
        self._require_bn_inference()
        count = self._bn_collect_ops[0].extras[2]
        return int(self.sess._materialize(count).item()) // self._bn_rows_per_sample

    def _require_calibrated(self):
        self._require_bn_inference()
        if not self._bn_calibrated:
            if self.bn_calibration_rows() < 1:       # (statistics restored from a checkpoint count as well)
                raise RuntimeError("bn='stored': the BatchNorm statistics are uncalibrated (0 rows): run calibrate_bn, or restore a "
                                   "checkpoint that holds them")
            self._bn_calibrated = True

    def reset_bn_statistics(self):
        """Back to slim's initial values (mean 0, variance 1) and a count of 0: the next calibrate_bn starts afresh."""
        self._require_bn_inference()
        for state in self._bn_state.values():
            for t in state:
                self.sess._materialize(t).fill_(t.init)
        self._bn_calibrated = False

    def calibrate_bn(self, images, actions):
        """Merge one batch (frames [B, H, W, 3], actions [B, 10]) into the stored statistics: the generator runs on batch
        statistics as ``test`` does and every BatchNorm layer pools its input rows (ops.BnCollectOp).  -> batch rows seen so far."""
        self._require_bn_inference()
        self._announced = None
        self.sess.run(self._bn_collect_ops, {self.img_ph: images, self._img_pad: images, self.action_ph: actions})
        self._bn_calibrated = False                  # (re-read from the device by the next stored-mode call)
        return self.bn_calibration_rows()

    def bn_statistics(self):
        """-> {state name: numpy array}: every layer's ``moving_mean`` / ``moving_variance`` [C] float32 and ``calibration_rows``
        [1] int64 (layer rows: batch rows times the layer's h * w)."""
        self._require_bn_inference()
        return {t.name: self.sess._materialize(t).detach().cpu().numpy().copy() for state in self._bn_state.values() for t in state}

    def _step_losses(self, frame, state, next_frame, next_state, d_out, prefix, suffix='', mean_ssim=False):
        """The losses of ONE generator step (train.py:72-85), for the one-step graph and every step of the rollout: L1 / B (times
        L2_WEIGHT plus the state norm / B where the generator has a state head), plus the SSIM term, is the l2 part; the full loss
        adds the adversarial term on ``d_out`` = D(fake) and the GDL with ``arg_adv``.  -> (l2 part, SSIM term or None, adversarial
        term or None, full G loss).  ``mean_ssim``: the SSIM term is the unweighted mean sum_b (1 - SSIM_b) / B, which the one-step
        graph reports as a summary (it divides, then weighs); the rollout steps weigh the sum by ssim_weight / B in one op."""
        B = self.batch_size
        l1, gdl = O.frame_losses(frame, next_frame)
        l2 = l1 / B
        if state is not None:
            with G.get_default_graph().side_branch():      # the state head's loss belongs to its side chain (models.py)
                state_loss = O.l2_norm(state, next_state, name='%sg_state_loss%s' % (prefix, suffix))
            l2 = l2 * L2_WEIGHT + state_loss / B
        ssim = None
        if self.ssim_weight and mean_ssim:
            ssim = O.ssim_loss(frame, next_frame) / B
            l2 = l2 + ssim * self.ssim_weight
        elif self.ssim_weight:
            ssim = O.ssim_loss(frame, next_frame) * (self.ssim_weight / B)
            l2 = l2 + ssim
        if not self.arg_adv:
            return l2, ssim, None, l2
        adv = O.build_g_adv_loss(d_out, self.arg_loss)
        return l2, ssim, adv, l2 + adv + gdl

    def _build_rollout(self, build_g, minimize_g):
        """K generator instances chained through their own predictions and K D(fake) instances, on the existing variables.
        Step j: x_{t+j+1}, s_{t+j+1} = G(in_j, act_j) with in_0 the fed frame and in_j the frame of step j-1; act_0 is fed, act_j
        is [command_j (fed), the state of step j-1] (the plain generator has no state head: act_j is fed whole, as test_sequence
        does).  Each step's loss is the one-step G loss on its own step - L1 / GDL against frame t+j+1, the state norm against
        s_{t+j+1}, the adversarial term on D(concat(in_j, x_{t+j+1}), act_j) - and BatchNorm takes the statistics of each instance.
        The G loss is the mean of the K step losses, the pretraining loss the mean of their l2 parts; both updates continue the
        one-step optimizers' state (optim minimize slots_of)."""
        K, B, S = self.rollout_steps, self.batch_size, self.img_size
        dna = M.KINDS[self.model].state_head
        self.roll_img_ph = G.placeholder((B, S, S, 3), name='rollout/frame0')
        self.roll_img_ph.padded = self._roll_img_pad = G.placeholder((B, S, S, 3), name='rollout/frame0_conv', channel_pitch=O.cpad(3), act=True)
        self.roll_next_ph = [G.placeholder((B, S, S, 3), name='rollout/next_frame%d' % j) for j in range(K)]
        self.roll_state_ph = [G.placeholder((B, STATE_DIM), name='rollout/next_state%d' % j) for j in range(K)]
        # fed action input of each step: the whole vector at step 0 (and every step of the plain generator), the command half else
        self.roll_action_ph = [G.placeholder((B, ACTION_DIM if (j == 0 or not dna) else 5), name='rollout/action%d' % j) for j in range(K)]
        img, act = self.roll_img_ph, self.roll_action_ph[0]
        self._ss_mask = self._ss_prob = None
        ss = self.sched_sampling
        if ss is not None:
            # scheduled sampling: ONE draw for the K - 1 fed-back positions, shared by both K-step programs (each run of either
            # advances the counter); step j mixes under row j - 1 of the mask
            O.sched_sampling_state(ss['seed'])
            self._ss_mask, self._ss_prob = O.sched_sample_draw(K - 1, B, ss['kind'], ss['start'], ss['final'], ss['decay_steps'],
                                                               ss['offset'], name='rollout/sched_sample/draw')
        self.rollout_frames, self.rollout_states, self.rollout_losses, l2_losses = [], [], [], []
        for j in range(K):
            frame, state = build_g(img, act, B, True)
            d_out = M.build_discriminator(O.concat([img, frame], axis=3, name='rollout/d_in%d' % j, pitch=8, act=True), act, reuse=True)
            l2, _, _, loss = self._step_losses(frame, state, self.roll_next_ph[j], self.roll_state_ph[j], d_out, 'rollout/', str(j))
            self.rollout_frames.append(frame)
            self.rollout_states.append(state)
            self.rollout_losses.append(loss)
            l2_losses.append(l2)
            if j + 1 < K:
                if ss is not None:      # per sample the truth (what step j was scored against) or the prediction, by the step's coins
                    frame, state = O.sched_sample(self._ss_mask.view(j * B, (B,), name='rollout/sched_sample/mask%d' % (j + 1)), frame,
                                                  self.roll_next_ph[j], state if dna else None, self.roll_state_ph[j] if dna else None,
                                                  name='rollout/sched_sample%d' % (j + 1))
                img = frame
                act = O.rollout_actions(self.roll_action_ph[j + 1], state, name='rollout/actions%d' % (j + 1)) if dna else self.roll_action_ph[j + 1]
        total, l2_total = sum(self.rollout_losses[1:], self.rollout_losses[0]), sum(l2_losses[1:], l2_losses[0])
        self.g_rollout_opt_op = minimize_g('g_opt_rollout', total / K, slots_of=self.g_opt_op)
        self.g_rollout_pretrain_opt_op = minimize_g('g_pretrain_opt_rollout', l2_total / K, slots_of=self.g_pretrain_opt_op)

    def _rollout_feed(self, frames, actions, states):
        """frames [B, K+1, H, W, 3] (t .. t+K), actions [B, K, 10] (a_t .. a_{t+K-1}, state half read at step 0 only by the DNA
        generator), states [B, K, 5] (s_{t+1} .. s_{t+K}) -> the feed of the K-step programs."""
        K = self.rollout_steps
        if frames.shape[1] != K + 1 or actions.shape[1] != K or states.shape[1] != K:
            raise ValueError('rollout of %d steps: frames [B, %d, ...], actions [B, %d, 10] and states [B, %d, 5] expected, got %s, %s, %s'
                             % (K, K + 1, K, K, tuple(frames.shape), tuple(actions.shape), tuple(states.shape)))
        f0 = frames[:, 0]
        fd = {self.roll_img_ph: f0, self._roll_img_pad: f0}
        for j in range(K):
            fd[self.roll_next_ph[j]] = frames[:, j + 1]
            fd[self.roll_state_ph[j]] = states[:, j]
            a = actions[:, j]
            fd[self.roll_action_ph[j]] = a if self.roll_action_ph[j].shape[1] == ACTION_DIM else a[:, :5]
        return fd

    def train_g_rollout(self, frames, actions, states, device_fetch=False):
        """One G step through the generator's own K-step rollout (K = ``rollout_steps``): the mean of the K step losses, every
        gradient flowing through the fed-back frames and states (_build_rollout).  frames [B, K+1, H, W, 3], actions [B, K, 10],
        states [B, K, 5] (_rollout_feed).  -> the frames of the last step, as train_g returns its frames.  K = 1: train_g."""
        if self.rollout_steps == 1:
            return self.train_g(frames[:, 0], frames[:, 1], actions[:, 0], states[:, 0], device_fetch=device_fetch)
        self._announced = None
        res = self.sess.run([self.g_rollout_opt_op, self.rollout_frames[-1]], self._rollout_feed(frames, actions, states),
                            device_fetch=device_fetch)
        return res[1]

    def pretrain_g_rollout(self, frames, actions, states):
        """pretrain_g through the K-step rollout: the mean of the step l2 losses.  -> the G loss of the last step, as pretrain_g
        returns its G loss.  K = 1: pretrain_g."""
        if self.rollout_steps == 1:
            return self.pretrain_g(frames[:, 0], frames[:, 1], actions[:, 0], states[:, 0])
        self._announced = None
        _, g_res = self.sess.run([self.g_rollout_pretrain_opt_op, self.rollout_losses[-1]], self._rollout_feed(frames, actions, states))
        return float(g_res[0])

    # ---- steps: one sess.run each (train.py:114-155)
    def _feed(self, input_images, next_frame, actions, state=None):
        return {self.img_ph: input_images, self._img_pad: input_images, self.next_frame_ph: next_frame,
                self.action_ph: actions, self.next_state: self._zero_state if state is None else state}

    def pretrain_g(self, input_images, next_frame, actions, state):
        self._announced = None
        self._noise_switch(True)
        _, g_res = self.sess.run([self.g_pretrain_opt_op, self.g_loss], self._feed(input_images, next_frame, actions, state))
        return float(g_res[0])

    def train_g(self, input_images, next_frame, actions, state, device_fetch=False):
        # the generator forward pass of these very inputs was run by the preceding train_d(..., next_g=(input_images, actions)):
        # the program then starts behind it (Session.run skip=)
        prepared, self._announced = self._announced, None
        self._noise_switch(True)
        if prepared is not None and prepared[0] is input_images and prepared[1] is actions:
            fd = self._feed(input_images, next_frame, actions, state)
            if len(prepared) == 4:      # host arrays the announcing D step already put on the device: no second upload
                fd[self.img_ph] = fd[self._img_pad] = prepared[2]
                fd[self.action_ph] = prepared[3]
            res = self.sess.run([self.g_opt_op, self.g_next_frame] + self._g_extra, fd, device_fetch=device_fetch, skip=self._skip_g)
            return res[1]
        _, gen_next_frames = self.sess.run([self.g_opt_op, self.g_next_frame],
                                           self._feed(input_images, next_frame, actions, state), device_fetch=device_fetch)
        return gen_next_frames

    def train_d(self, input_images, next_frame, actions, summarize=False, next_g=None, pair=None, next_d=None):
        """One discriminator step (train.py:132-144).  ``next_g`` / ``next_d`` = (input_images, actions) of the ``train_g`` /
        ``train_d`` call that follows (extension, see __init__ ``lookahead``): this step's generator pass then also covers that
        step's samples, and that step starts behind its generator forward pass (with n_critic > 1 the D steps alternate: one runs
        the pair pass for itself and its successor, the next runs no generator at all).  ``pair`` = the two batches already
        joined, (frames [2 B, H, W, 3], actions [2 B, 10]) with the FOLLOWING step's samples first - saves the concatenation
        here when the caller keeps its batches that way."""
        prepared, self._announced = self._announced, None
        self._noise_switch(True)
        fd = self._feed(input_images, next_frame, actions)
        if summarize:
            _, summ, _ = self.sess.run([self.d_opt_op, self.merged_summaries, self.clip_d], fd)
            return self._named(summ)
        if prepared is not None and prepared[0] is input_images and prepared[1] is actions:
            # the preceding D step ran the generator for these samples: their frames wait in the spare rows
            if len(prepared) == 4:
                fd[self.img_ph] = fd[self._img_pad] = prepared[2]
                fd[self.action_ph] = prepared[3]
            self.sess.run([self.d_opt_op, self.clip_d] + self._g_extra, fd, skip=self._skip_g)
            return None
        nxt = next_g if next_g is not None else next_d
        if nxt is not None and self.lookahead:
            self._announced = (nxt[0], nxt[1])
            if pair is None:
                if self.sess.rt.is_cuda and not torch.is_tensor(input_images) and not torch.is_tensor(nxt[0]):
                    # host arrays (the reference's numpy call path): each batch goes to the device ONCE - the pair is joined there,
                    # this step and the announced one are fed the device copies (round 5: -4.5 MB of uploads and a 3 MB host
                    # concatenation per iteration)
                    # (pinned staging + a copy stream of its own: neither the host nor the running step waits; one copy for the four)
                    x_d, a_d, x_n, a_n = self.sess.upload_many([input_images, actions, nxt[0], nxt[1]])
                    fd[self.img_ph] = fd[self._img_pad] = x_d
                    fd[self.action_ph] = a_d
                    pair = (torch.cat([x_n, x_d]), torch.cat([a_n, a_d]))
                    self._announced = (nxt[0], nxt[1], x_n, a_n)
                else:
                    pair = (_join(nxt[0], input_images), _join(nxt[1], actions))
            fd.update({self.pair_img_ph: pair[0], self._pair_img_pad: pair[0], self.pair_action_ph: pair[1]})
            self.sess.run([self.d_opt_op, self.clip_d, self._pair_concat], fd, skip=self._skip_d)
            return None
        self.sess.run([self.d_opt_op, self.clip_d], fd)
        return None

    def test(self, input_images, next_frame, actions, bn='batch', weights='raw', noise='zero'):
        """``noise`` (a Trainer built with ``noise_dim``): 'zero' - z = 0 - or 'sample' - a fresh z, see ``last_noise``; with
        ``posterior`` also 'posterior' - z drawn from q(z | input_images, next_frame) - and 'posterior_mean' - its mean.
        ``bn='stored'`` (a Trainer built with ``bn_inference``, after calibration): the stored-statistics generator; the
        summaries then hold ``g_psnr`` alone (the other six read the discriminator on the batch-statistics frames).
        ``weights='ema'`` (a Trainer built with ``ema_decay``): the same call inside ``ema_weights()``."""
        with self._predicting(bn, weights, noise) as stored:
            if stored:
                has_state = self.g_state_stored is not None
                fd = {self.img_ph: input_images, self._img_pad: input_images, self.next_frame_ph: next_frame, self.action_ph: actions}
                res = self.sess.run([self.g_out_stored] + ([self.g_state_stored] if has_state else []) + [[self._stored_psnr]], fd)
                return res[0], (res[1] if has_state else None), {'g_psnr': float(np.asarray(res[-1][0]).reshape(-1)[0])}
            tensors = [self.g_next_frame] + ([self.g_state_out] if self.g_state_out is not None else []) + [self.merged_summaries]
            res = self.sess.run(tensors, self._feed(input_images, next_frame, actions))
            gen_next_frames, summ = res[0], res[-1]
            gen_next_state = res[1] if self.g_state_out is not None else None      # defect D4
            return gen_next_frames, gen_next_state, self._named(summ)

    def test_sequence(self, input_images, test_next_frame, test_actions, steps=None, literal=False, device_loop=None, bn='batch',
                      weights='raw', noise='zero'):
        """Recursive rollout: feed each prediction (and predicted state) back in.
        ``device_loop`` (default: on for a GPU session): from the second step on the prediction and the predicted state stay on the
        device between steps - the program of those steps fetches nothing but the two, so it carries no loss ops either - and
        all predictions come to the host in one copy at the end.  Same kernels on the same bits as the step-by-step numpy round
        trip (``device_loop=False``, the reference's own loop), which it replaces only in where the intermediate frames live.

        Default: the evaluation block of the reference's training loop (train.py:285-298) - T-1 steps, step j commanded
        by ``test_actions[:, j]`` and scored against ``test_next_frame[:, j + 1]`` (defect D7: own states); returns
        ``(predicted [B, steps, H, W, 3], summaries of step 0)``.
        ``literal=True``: the reference's method of this name exactly as written (train.py:157-176) - SIX steps, step j
        reads ``test_actions[:, 2 j, :5]`` and ``test_next_frame[:, 2 j]`` (the sequences must hold >= 11 frames),
        and the second return value is ``current_frame[1:7]``, samples 1..6 of the last prediction.
        ``bn``: 'batch' (default: every step normalises with the statistics of its batch) or 'stored' (see ``test``).
        ``weights``: 'raw' or 'ema' (see ``test``).  ``noise``: 'zero' or 'sample' (see ``test``): every step draws its own z."""
        with self._predicting(bn, weights, noise):       # (the steps are ``test`` calls on the weights this has put in place)
            if literal:
                predicted = []
                current_frame = input_images[:, 0]
                current_state = test_actions[:, 0, 5:]
                for j in range(0, 6):
                    acs = np.concatenate((test_actions[:, j * 2, :5], current_state), axis=1).astype(np.float32)
                    out, st, _ = self.test(current_frame, test_next_frame[:, j * 2], acs, bn=bn, noise=noise)
                    predicted.append(out)
                    current_frame = out
                    current_state = st if st is not None else test_actions[:, j * 2, 5:]      # plain generator: no state head (D4)
                return np.transpose(np.array(predicted), (1, 0, 2, 3, 4)), current_frame[1:7]
            steps = steps if steps is not None else test_next_frame.shape[1] - 1
            if device_loop is None:
                device_loop = self.sess.rt.is_cuda
            if device_loop and steps >= 1:
                predicted, summ0 = self._rollout_on_device(input_images, test_next_frame, test_actions, steps, bn=bn, noise=noise)
                return predicted.cpu().numpy(), summ0
            predicted, summ0 = [], None
            current_frame = input_images[:, 0]
            current_state = test_actions[:, 0, 5:]
            for j in range(steps):
                acs = np.concatenate((test_actions[:, j, :5], current_state), axis=1).astype(np.float32)
                out, st, summ = self.test(current_frame, test_next_frame[:, j + 1], acs, bn=bn, noise=noise)
                summ0 = summ0 or summ
                predicted.append(out)
                current_frame = out
                current_state = st if st is not None else test_actions[:, j + 1, 5:]
            return np.transpose(np.array(predicted), (1, 0, 2, 3, 4)), summ0

    def _rollout_on_device(self, input_images, test_next_frame, test_actions, steps, bn='batch', noise='zero'):
        """The device loop of ``test_sequence``: -> (predicted [B, steps, H, W, 3] float32 on the device, summaries of step 0).
        The noise switch ``test`` sets stays as it is for the steps that follow: each of them draws (or zeroes) its own z."""
        out, st, summ0 = self.test(input_images[:, 0], test_next_frame[:, 1], np.asarray(test_actions[:, 0], np.float32), bn=bn,
                                   noise=noise)
        acts = self.sess.upload(np.asarray(test_actions[:, :steps + 1], np.float32))          # [B, steps + 1, 10], once
        frame = self.sess.upload(out)
        state = self.sess.upload(st) if st is not None else acts[:, 1, 5:]
        frames = [frame]
        fetches = [self.g_next_frame] + ([self.g_state_out] if self.g_state_out is not None else [])
        if bn == 'stored':
            fetches = [self.g_out_stored] + ([self.g_state_stored] if self.g_state_stored is not None else [])
        for j in range(1, steps):
            acs = torch.cat([acts[:, j, :5], state], dim=1).contiguous()
            fd = self._feed(frame, test_next_frame[:, j + 1], acs)      # (next_frame is not read by this program: checked, not uploaded)
            self._announced = None
            res = self.sess.run(fetches, fd, device_fetch=True)
            frame = res[0].float().clone()                             # the fetch is the tensor's own buffer: the next step overwrites it
            state = res[1].float().clone() if self.g_state_out is not None else acts[:, j + 1, 5:]
            frames.append(frame)
        return torch.stack(frames, dim=1), summ0

    def rollout_metrics(self, images, actions, steps=None, identity=True, return_frames=False, bn='batch', weights='raw',
                        noise='zero'):
        """Quality of the recursive rollout, scored on the GPU (metrics.frame_metrics; no reference counterpart - the curves of
        its report).  Rollout as ``test_sequence``'s default on the device loop: ``steps`` (default T-1) steps,
        step j commanded by ``actions[:, j]`` with the generator's own predicted state (defect D7) and scored against
        ``images[:, j + 1]``.  The predictions stay on the device; all B * steps frames are scored in one launch.  ``identity``:
        also score the identity baseline - ``images[:, 0]`` carried forward - against the same targets.
        -> dict of numpy arrays [B, steps]: ``ssim``, ``sqerr`` (sum of squared errors of the frame), and ``identity_ssim``,
        ``identity_sqerr``; with ``return_frames`` also ``frames`` [B, steps, H, W, 3] (the only device-to-host copy of frames).
        ``bn``: 'batch' or 'stored', ``weights``: 'raw' or 'ema', ``noise``: 'zero' or 'sample', as ``test`` takes them."""
        from . import metrics
        with self._predicting(bn, weights, noise, switch=False):
            if not self.sess.rt.is_cuda:
                raise RuntimeError('rollout_metrics scores on the GPU: the session has no GPU device')
            steps = steps if steps is not None else images.shape[1] - 1
            if steps < 1 or steps + 1 > images.shape[1]:
                raise ValueError('rollout_metrics: %d steps need %d frames per sequence, got %d' % (steps, steps + 1, images.shape[1]))
            predicted, _ = self._rollout_on_device(images, images, actions, steps, bn=bn, noise=noise)
            seq = self.sess.upload(np.asarray(images[:, :steps + 1], np.float32))                # [B, steps + 1, H, W, 3], once
            truth = seq[:, 1:]
            ssim, sqerr = metrics.frame_metrics(predicted, truth)
            out = {'ssim': ssim, 'sqerr': sqerr}
            if identity:
                out['identity_ssim'], out['identity_sqerr'] = metrics.frame_metrics(seq[:, :1].expand_as(truth), truth)
            out = {k: v.cpu().numpy() for k, v in out.items()}
            if return_frames:
                out['frames'] = predicted.cpu().numpy()
            return out

    def _named(self, values):
        return {k: float(np.asarray(v).reshape(-1)[0]) for k, v in zip(self._summary_names, values)}


model_kind = M.model_kind        # (the generator an ``arg_transform`` names: a key of models.KINDS)


F32_MAX = float(np.finfo(np.float32).max)


def _f32(x):
    return float(np.float32(x))


def _number(value, what, be, lie, ok):
    """``value`` as a float when it is a number - no bool - that ``ok`` accepts (a range test, in float32 too where the kernel
    reads a float32; nan fails every one of them); else ValueError: '<what> must be <be>' for no number, '<what> must <lie>'."""
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s must be %s, got %r' % (what, be, value))
    if isinstance(value, bool) or not ok(x):
        raise ValueError('%s must %s, got %r' % (what, lie, value))
    return x


def _is_count(value):
    """An integer (no bool) in [0, 2^63): a number of updates or iterations the kernels take as int64."""
    return not isinstance(value, bool) and isinstance(value, (int, np.integer)) and 0 <= int(value) < 2 ** 63


def check_ema_decay(ema_decay):
    """ValueError for an ``ema_decay`` that is neither 0 (no average) nor inside (0, 1); -> the decay as a float."""
    return _number(ema_decay, 'ema_decay', '0 (off) or a number in (0, 1)', 'be 0 (off) or lie in (0, 1)',
                   lambda d: 0.0 <= d < 1.0 and (d == 0.0 or 0.0 < _f32(d) < 1.0))


def check_ssim_weight(ssim_weight):
    """ValueError for an ``ssim_weight`` that is not a finite number >= 0; -> the weight as a float (0: no SSIM term)."""
    return _number(ssim_weight, 'ssim_weight', 'a finite number >= 0', 'be finite and >= 0', lambda w: 0.0 <= w <= F32_MAX)


def check_clip_norm(value, what='clip_norm'):
    """ValueError for a ``g_clip_norm`` / ``d_clip_norm`` that is not a finite number >= 0 (or is positive and rounds to 0 in
    float32); -> the bound as a float (0: no clip)."""
    return _number(value, what, 'a finite number >= 0', 'be finite and >= 0 (0: off)',
                   lambda x: 0.0 <= x <= F32_MAX and (x == 0.0 or _f32(x) != 0.0))


LR_SCHEDULES = ('constant', 'linear', 'cosine', 'exponential')


def check_lr(g_lr=None, d_lr=None, beta1=None, arg_opt='adam', lr_schedule='constant', lr_warmup=0, lr_decay_steps=0, lr_final=0.0):
    """ValueError for learning-rate arguments the Trainer does not take: a rate that is not finite and > 0 (in float32 too),
    ``beta1`` outside [0, 1) or given with RMSProp, an unknown schedule, a negative or non-integer ``lr_warmup`` / ``lr_decay_steps``
    (an int, or a pair (G's, D's)), a decaying schedule with ``lr_decay_steps`` < 1, ``lr_final`` outside [0, 1] (exponential:
    (0, 1]).  -> {'g_lr', 'd_lr' (None replaced by the reference's constant), 'beta1' (or None), 'schedule', 'warmup' and
    'decay_steps' (pairs), 'final', 'scheduled' (whether anything but the existing entries is needed)}."""
    default = RMSPROP_LR if arg_opt == 'rmsprop' else ADAM_LR
    rates = {}
    for what, v in (('g_lr', g_lr), ('d_lr', d_lr)):
        rates[what] = default if v is None else _number(v, what, 'a finite number > 0', 'be finite and > 0',
                                                        lambda x: 0.0 < x <= F32_MAX and _f32(x) != 0.0)
    if beta1 is not None:
        if arg_opt == 'rmsprop':
            raise ValueError("beta1 is Adam's: it does not go with the rmsprop optimizer")
        beta1 = _number(beta1, 'beta1', 'a number in [0, 1)', 'lie in [0, 1)', lambda b: 0.0 <= b < 1.0 and _f32(b) < 1.0)
    if lr_schedule not in LR_SCHEDULES:
        raise ValueError('lr_schedule must be one of %s, got %r' % (', '.join(LR_SCHEDULES), lr_schedule))
    counts = {}
    for what, v in (('lr_warmup', lr_warmup), ('lr_decay_steps', lr_decay_steps)):
        pair = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        if len(pair) != 2 or not all(_is_count(c) for c in pair):
            raise ValueError("%s must be an integer >= 0 (or a pair of them: G's, D's), got %r" % (what, v))
        counts[what] = (int(pair[0]), int(pair[1]))
    final = _number(lr_final, 'lr_final', 'a number in [0, 1]', 'lie in [0, 1]', lambda x: 0.0 <= x <= 1.0)
    if lr_schedule != 'constant':
        if min(counts['lr_decay_steps']) < 1:
            raise ValueError('lr_schedule %r needs lr_decay_steps >= 1, got %r' % (lr_schedule, lr_decay_steps))
        if lr_schedule == 'exponential' and not float(np.float32(final)) > 0.0:
            raise ValueError("lr_schedule 'exponential' needs lr_final in (0, 1], got %r" % (lr_final,))
    return {'g_lr': rates['g_lr'], 'd_lr': rates['d_lr'], 'beta1': beta1, 'schedule': lr_schedule, 'warmup': counts['lr_warmup'],
            'decay_steps': counts['lr_decay_steps'], 'final': final,
            'scheduled': lr_schedule != 'constant' or max(counts['lr_warmup']) > 0}


def check_noise_seed(seed, what='noise_seed'):
    """ValueError for a seed (or counter) of a device-side draw - the noise input's, the scheduled-sampling coins' - that is not an
    integer in [0, 2^64); -> it as an int."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError('%s must be an integer in [0, 2^64), got %r' % (what, seed))
    return int(seed)


# ``noise`` of a predicting call -> the {scale, posterior} mode of acg_latent_fwd (without a posterior: scale alone)
NOISE_MODES = {'zero': (0.0, 0.0), 'sample': (1.0, 0.0), 'posterior': (1.0, 1.0), 'posterior_mean': (0.0, 1.0)}


def check_posterior(posterior=False, kl_weight=1.0, noise_dim=0, bf16=False):
    """ValueError for ``posterior`` / ``kl_weight`` the Trainer does not take: a ``kl_weight`` that is not a finite number >= 0,
    ``posterior`` without ``noise_dim`` > 0 or in a bf16 graph.  ``noise_dim`` is the checked one (check_noise, whose refusals
    of rollout_steps > 1 and bn_inference cover the posterior too).  -> (posterior as a bool, kl_weight as a float)."""
    w = _number(kl_weight, 'kl_weight', 'a finite number >= 0', 'be finite and >= 0', lambda x: 0.0 <= x <= F32_MAX)
    if posterior and not noise_dim:
        raise ValueError('posterior needs noise_dim > 0 (the latent it is the posterior of)')
    if posterior and bf16:
        raise ValueError('posterior does not go with a bf16 graph (the action gradient the encoder is trained through is float32 only)')
    return bool(posterior), w


def check_noise(noise_dim, noise_seed=0, rollout_steps=1, bn_inference=False, batch_size=1):
    """ValueError for a ``noise_dim`` the Trainer does not take (outside 0..64; > 0 together with rollout_steps > 1 or with
    bn_inference; more than 8192 values per batch) or a bad ``noise_seed``; -> Z."""
    if isinstance(noise_dim, bool) or not isinstance(noise_dim, (int, np.integer)) or not 0 <= int(noise_dim) <= _lib.NOISE_DIM_MAX:
        raise ValueError('noise_dim must be an integer in 0..%d (0: no noise input), got %r' % (_lib.NOISE_DIM_MAX, noise_dim))
    check_noise_seed(noise_seed)
    z = int(noise_dim)
    if z and int(rollout_steps) > 1:
        raise ValueError('noise_dim > 0 does not go with rollout_steps > 1 (the K-step programs read no noise)')
    if z and bn_inference:
        raise ValueError('noise_dim > 0 does not go with bn_inference (the calibration and stored-statistics instances read no noise)')
    if z * int(batch_size) > _lib.NOISE_VALUES_MAX:
        raise ValueError('noise_dim %d at batch %d: one draw holds at most %d values' % (z, batch_size, _lib.NOISE_VALUES_MAX))
    return z


SCHED_SAMPLING = ('off',) + O.SCHED_SAMPLING_KINDS


def check_sched_sampling(sched_sampling='off', ss_start=1.0, ss_final=0.0, ss_decay_steps=0, ss_offset=0, ss_seed=0, rollout_steps=1,
                         batch_size=1):
    """ValueError for scheduled-sampling arguments the Trainer does not take: an unknown kind, a kind other than 'off' without
    ``rollout_steps`` > 1, ``ss_start`` / ``ss_final`` outside [0, 1], a negative or non-integer ``ss_decay_steps`` / ``ss_offset``, a
    decaying kind with ``ss_decay_steps`` < 1, a bad ``ss_seed``, more than 8192 coins per program.  -> None for 'off', else
    {'kind', 'start', 'final', 'decay_steps', 'offset', 'seed'}."""
    if sched_sampling not in SCHED_SAMPLING:
        raise ValueError('sched_sampling must be one of %s, got %r' % (', '.join(SCHED_SAMPLING), sched_sampling))
    probs = {what: _number(v, what, 'a number in [0, 1]', 'lie in [0, 1]', lambda x: 0.0 <= x <= 1.0)
             for what, v in (('ss_start', ss_start), ('ss_final', ss_final))}
    counts = {}
    for what, v in (('ss_decay_steps', ss_decay_steps), ('ss_offset', ss_offset)):
        if not _is_count(v):
            raise ValueError('%s must be an integer >= 0, got %r' % (what, v))
        counts[what] = int(v)
    seed = check_noise_seed(ss_seed, 'ss_seed')
    if sched_sampling == 'off':
        return None
    if int(rollout_steps) <= 1:
        raise ValueError('sched_sampling %r needs rollout_steps > 1 (a one-step program feeds nothing back)' % (sched_sampling,))
    if sched_sampling != 'constant' and counts['ss_decay_steps'] < 1:
        raise ValueError('sched_sampling %r needs ss_decay_steps >= 1, got %r' % (sched_sampling, ss_decay_steps))
    if (int(rollout_steps) - 1) * int(batch_size) > _lib.NOISE_VALUES_MAX:
        raise ValueError('sched_sampling: %d fed-back steps at batch %d: one draw holds at most %d coins'
                         % (int(rollout_steps) - 1, batch_size, _lib.NOISE_VALUES_MAX))
    return {'kind': sched_sampling, 'start': probs['ss_start'], 'final': probs['ss_final'], 'decay_steps': counts['ss_decay_steps'],
            'offset': counts['ss_offset'], 'seed': seed}


D_SLOTS = {'gen': 0, 'real': 1, 'both': 2}      # the D instances' slots in a draw's stream id (instance noise, d_augment)


def check_d_augment(d_augment=None, d_augment_seed=0, rollout_steps=1, arg_adv=True, bf16=False):
    """The differentiable-augmentation arguments of Trainer / train(), checked before anything is created.  ``d_augment``: None or
    '' (off), or a comma-separated subset of ``color``, ``translation``, ``cutout`` in any order.  Declined (ValueError): an unknown
    or repeated name, a bad ``d_augment_seed``, and an augmentation together with ``rollout_steps`` > 1, without ``arg_adv`` or in
    a bf16 graph.  -> None (off, whatever the other arguments are), else {'names': the names in canonical order, 'policy': the
    ACG_DA_* bits, 'seed'}."""
    if d_augment is None or d_augment == '':
        return None
    if not isinstance(d_augment, str):
        raise ValueError('d_augment is not a valid policy: a comma-separated subset of %s, got %r' % (', '.join(O.D_AUGMENT_NAMES), d_augment))
    names = [n.strip() for n in d_augment.split(',')]
    for n in names:
        if n not in O.D_AUGMENT_NAMES or names.count(n) > 1:
            raise ValueError('d_augment %r is not a valid policy: %r is %s (a comma-separated subset of %s)'
                             % (d_augment, n, 'repeated' if n in O.D_AUGMENT_NAMES else 'unknown', ', '.join(O.D_AUGMENT_NAMES)))
    seed = check_noise_seed(d_augment_seed, 'd_augment_seed')
    if rollout_steps > 1:
        raise ValueError("d_augment does not go with rollout_steps > 1 (the K-step programs' D instances are not augmented)")
    if not arg_adv:
        raise ValueError('d_augment needs an adversarial trainer (arg_adv): without one nothing is trained against the discriminator')
    if bf16:
        raise ValueError('d_augment does not go with a bf16 graph (the augmentation kernels are float32 only)')
    names = [n for n in O.D_AUGMENT_NAMES if n in names]
    return {'names': names, 'policy': sum(_lib.DA_POLICY_BITS[n] for n in names), 'seed': seed}


def check_d_noise(d_noise=0.0, d_noise_final=0.0, d_noise_decay_steps=0, d_noise_offset=0, d_noise_seed=0, rollout_steps=1, arg_adv=True):
    """ValueError for instance-noise arguments the Trainer does not take: a level that is not a finite number >= 0 (in float32
    too), a negative or non-integer ``d_noise_decay_steps`` / ``d_noise_offset``, a bad ``d_noise_seed``, and ``d_noise`` > 0 together
    with ``rollout_steps`` > 1 or without ``arg_adv``.  -> None for ``d_noise`` = 0 (off, whatever the other arguments are), else
    {'start', 'final', 'decay_steps', 'offset', 'seed'}."""
    levels = {what: _number(v, what, 'a finite number >= 0', 'be finite and >= 0', lambda x: 0.0 <= x <= F32_MAX)
              for what, v in (('d_noise', d_noise), ('d_noise_final', d_noise_final))}
    counts = {}
    for what, v in (('d_noise_decay_steps', d_noise_decay_steps), ('d_noise_offset', d_noise_offset)):
        if not _is_count(v):
            raise ValueError('%s must be an integer >= 0, got %r' % (what, v))
        counts[what] = int(v)
    seed = check_noise_seed(d_noise_seed, 'd_noise_seed')
    if levels['d_noise'] == 0.0:
        return None
    if _f32(levels['d_noise']) == 0.0:
        raise ValueError('d_noise must be finite and >= 0 (0: off), got %r: it rounds to 0 in float32' % (d_noise,))
    if int(rollout_steps) > 1:
        raise ValueError("d_noise > 0 does not go with rollout_steps > 1 (the K-step programs' D(fake) instances read no noise)")
    if not arg_adv:
        raise ValueError('d_noise > 0 needs an adversarial trainer (arg_adv): without one nothing is trained against the discriminator')
    return {'start': levels['d_noise'], 'final': levels['d_noise_final'], 'decay_steps': counts['d_noise_decay_steps'],
            'offset': counts['d_noise_offset'], 'seed': seed}


def check_pixel_maps(pixel_maps, model):
    """ValueError for a ``pixel_maps`` the Trainer does not take with the generator ``model``; -> D (0: no map path)."""
    if isinstance(pixel_maps, bool) or not isinstance(pixel_maps, (int, np.integer)) or not 0 <= pixel_maps <= _lib.PLAN_PIXEL_MAPS_MAX:
        raise ValueError('pixel_maps must be an integer in 0..%d, got %r' % (_lib.PLAN_PIXEL_MAPS_MAX, pixel_maps))
    if pixel_maps and M.KINDS[model].no_maps:
        raise ValueError('pixel_maps %d: %s' % (pixel_maps, M.KINDS[model].no_maps))
    return int(pixel_maps)


def check_canvas(canvas, model, ksize, num_masks):
    """ValueError for a ``canvas`` the generator ``model`` does not take (it has no masks, or ``num_masks`` leaves it no mask
    channel); -> bool."""
    if canvas:
        M.KINDS[model].check_args(ksize, num_masks, True)
    return bool(canvas)


def check_rollout(rollout_steps, model, bf16=False, data_parallel=False):
    """ValueError for a ``rollout_steps`` the K-step trainer does not take (with the generator ``model``, a bf16 graph, data
    parallelism / synchronised BatchNorm); -> K."""
    k = int(rollout_steps)
    if k < 1:
        raise ValueError('rollout_steps must be >= 1, got %d' % k)
    if k > 1:
        if M.KINDS[model].no_rollout:
            raise ValueError('rollout_steps > 1 does not train the %s generator (%s)' % (M.KINDS[model].label, M.KINDS[model].no_rollout))
        if bf16:
            raise ValueError('rollout_steps > 1 is float32 only (dtype bf16)')
        if data_parallel:
            raise ValueError('rollout_steps > 1 runs on one rank (no data parallelism, sync_bn or exact_global_batch)')
    return k


def _join(first, second):
    """[first ; second] along the batch axis, numpy arrays or (device) torch tensors."""
    if torch.is_tensor(first):
        return torch.cat([first, second.to(first.device) if torch.is_tensor(second) else torch.as_tensor(second, device=first.device)], dim=0)
    return np.concatenate([np.asarray(first), np.asarray(second.cpu() if torch.is_tensor(second) else second)], axis=0)


def _ancestors(tensor, within):
    """The ops (restricted to the ids in ``within``) that ``tensor`` depends on, its producer included, creation order."""
    seen, stack = {}, [tensor.op]
    while stack:
        op = stack.pop()
        if op is None or id(op) in seen or id(op) not in within:
            continue
        seen[id(op)] = op
        stack.extend(t.op for t in op.inputs)
    return sorted(seen.values(), key=lambda o: o.index)


def _alias_first_half(ops_small, ops_pair):
    """Two instances of one network built by the same code, the second on twice the batch: make every tensor the first
    instance's ops produce a window onto the FIRST HALF of its twin (batch-major storage: the first B samples; BatchNorm
    statistics [groups = 2, C]: group 0).  Tensors that already are windows (a BatchNorm output placed in its concatenation)
    follow through their base."""
    if len(ops_small) != len(ops_pair):
        raise RuntimeError('look-ahead: the two generator instances differ in structure (%d vs %d ops)' % (len(ops_small), len(ops_pair)))
    for a, b in zip(ops_small, ops_pair):
        if type(a) is not type(b) or len(a.outputs) != len(b.outputs):
            raise RuntimeError('look-ahead: %r has no twin in the pair instance (%r)' % (a, b))
        for ta, tb in zip(a.outputs, b.outputs):
            if ta.view_of is not None or ta.alias_of is not None or isinstance(ta, (G.Variable, G.Placeholder)):
                continue
            if tb.numel != 2 * ta.numel or ta.dtype != tb.dtype:
                raise RuntimeError('look-ahead: %r is not half of %r' % (ta, tb))
            ta.view_of = (tb, 0)


# ---- synthetic push-style data (rng(7), frames U(-1,1), action||state N(0,1)) ----------
class SyntheticPush:
    """Seeded random sequences in the shape of the push batches.  ``pool`` > 0: the first ``pool`` batches are kept and handed out
    round robin afterwards (drawing 3 M uniform numbers per batch costs a host core 10-50 ms - many training steps; the loop
    benchmark uses a pool so that what it times is the loop)."""

    def __init__(self, batch_size, seq_len=8, img_size=64, seed=7, rank=0, pool=0):
        self.rng = np.random.default_rng(seed + 1000 * rank)
        self.shape = (batch_size, seq_len, img_size, img_size, 3)
        self.batch_size, self.seq_len = batch_size, seq_len
        self.pool, self._kept, self._next = int(pool), [], 0

    def get_batch(self):
        """-> (frames, frames, action||state [B,T,10], state [B,T,5]) like ops.get_batch (ops.py:15-17)."""
        if self.pool and len(self._kept) == self.pool:
            img, acts = self._kept[self._next % self.pool]
            self._next += 1
            return img, img, acts, acts[:, :, 5:].copy()
        img = self.rng.uniform(-1.0, 1.0, self.shape).astype(np.float32)
        acts = self.rng.standard_normal((self.batch_size, self.seq_len, ACTION_DIM)).astype(np.float32)
        if self.pool:
            self._kept.append((img, acts))
        return img, img, acts, acts[:, :, 5:].copy()


def select_pairs(rng_randint, boolean_mask, batch_size):
    """(t, t+1) selection of train.py:231-232,249-250,258-259."""
    start_mask = boolean_mask[rng_randint(0, len(boolean_mask), size=batch_size)]
    return start_mask, np.roll(start_mask, 1, axis=1)


def select_windows(rng_randint, boolean_mask, batch_size, steps):
    """The (t, t+1, ..., t+steps) selection of a K-step rollout (K = ``steps``): t = randint(0, T-K) per sample, one draw of the
    same size from the same generator as select_pairs.  -> [steps + 1] one-hot masks [B, T] (frame t + i); for K = 1 exactly
    select_pairs' two masks."""
    start_mask = boolean_mask[rng_randint(0, len(boolean_mask) - steps + 1, size=batch_size)]
    return [start_mask] + [np.roll(start_mask, i, axis=1) for i in range(1, steps + 1)]


def window_batch(masks, inp, nxt, acts, states):
    """The K-step inputs of train_g_rollout from one batch and its select_windows masks: frames [B, K+1, ...] (frame t from
    ``inp``, the rest from ``nxt``), actions a_t .. a_{t+K-1} [B, K, 10], target states s_{t+1} .. s_{t+K} [B, K, 5]."""
    frames = np.stack([inp[masks[0]]] + [nxt[m] for m in masks[1:]], axis=1)
    return frames, np.stack([acts[m] for m in masks[:-1]], axis=1), np.stack([states[m] for m in masks[1:]], axis=1)


class _PairSelections:
    """The frame-pair selections of the coming iterations, drawn AHEAD of the loop in the reference's order (train.py:231-232
    per pretraining iteration; 249-250 per D step, then 258-259 once for the G step on the last D batch), from a private copy
    of numpy's global generator as it stands when the loop starts - the same numbers the loop would draw one call at a time,
    since nothing else in the loop draws from it.  Knowing them early is what lets a PushDataset decode only the frames a
    step will read (``data.announce``: 2-4 of a record's 7 JPEGs instead of all of them); a source without ``announce``
    (SyntheticPush) just gets its selections from here."""

    def __init__(self, boolean_mask, batch_size, d_per_g, pretrain_iter, train_iter, data, ahead=8, rollout_steps=1):
        """``rollout_steps`` K > 1: the G steps and pretraining steps select K-step windows (select_windows) instead of pairs; the
        D steps keep their pairs.  Drawn in the same order from the same generator."""
        self.rollout_steps = int(rollout_steps)
        self.rng = np.random.RandomState()
        self.rng.set_state(np.random.get_state())
        self.mask, self.batch_size, self.d_per_g = boolean_mask, batch_size, d_per_g
        self.pretrain_iter, self.train_iter = pretrain_iter, train_iter
        self.announce = getattr(data, 'announce', None)
        self.ahead, self.drawn, self.queue = max(int(ahead), 1), 0, []

    def _draw(self):
        i = self.drawn
        n = 1 if i < self.pretrain_iter else self.d_per_g + 1
        if self.rollout_steps > 1:
            sels = [select_pairs(self.rng.randint, self.mask, self.batch_size) for _ in range(n - 1)]
            sels.append(tuple(select_windows(self.rng.randint, self.mask, self.batch_size, self.rollout_steps)))
        else:
            sels = [select_pairs(self.rng.randint, self.mask, self.batch_size) for _ in range(n)]
        if self.announce is not None and self.rollout_steps > 1:
            if i < self.pretrain_iter:
                self.announce(np.logical_or.reduce(sels[0]))
            else:
                for j in range(self.d_per_g):
                    need = sels[j][0] | sels[j][1]
                    if j == self.d_per_g - 1:                       # the G step's window is on the last D batch
                        need = need | np.logical_or.reduce(sels[-1])
                    self.announce(need)
        elif self.announce is not None:
            if i < self.pretrain_iter:
                self.announce(sels[0][0] | sels[0][1])
            else:
                for j in range(self.d_per_g):
                    need = sels[j][0] | sels[j][1]
                    if j == self.d_per_g - 1:                       # the G step selects again on the last D batch
                        need = need | sels[-1][0] | sels[-1][1]
                    self.announce(need)
        self.queue.append(sels)
        self.drawn += 1

    def next(self):
        """The selections of the next iteration: [(start, end)] while pretraining, else [D_1, ..., D_n, G]."""
        while self.drawn < self.train_iter and len(self.queue) < self.ahead + 1:
            self._draw()
        return self.queue.pop(0)


def train_record(summ, iteration, wall_s, rollout_steps, ema_decay=0.0, ssim_weight=0.0, grad_stats=None, clip_bounds=None, noise_dim=0,
                 rates=None, ss_prob=None, canvas=False, d_augment=None):
    """One ``train.jsonl`` record.  ``grad_stats``: {scope: Trainer.grad_norm_stats(scope)} of the scopes that are measured (none:
    the record is what it was before gradient norms existed) -> ``<scope>_grad_norm`` / ``<scope>_clip_scale``;
    ``clip_bounds``: {scope: bound} -> ``<scope>_clip_norm`` (the first record of a run).  ``noise_dim`` is recorded when > 0.
    ``rates``: Trainer.learning_rates() of a run with a learning-rate schedule (None: no field is added) -> ``g_lr`` / ``d_lr``, the
    rates the iteration's last updates used.  ``ss_prob``: the probability of truth of the iteration's K-step update in a run with
    scheduled sampling (None: no field is added) -> ``ss_prob``.  ``canvas`` is recorded when on, and so is ``d_augment``, the
    canonical policy string of a run with differentiable augmentation (None: no field is added)."""
    record = dict(summ, iteration=iteration, wall_s=wall_s, rollout_steps=rollout_steps,
                  **({'g_ema': ema_decay} if ema_decay else {}),
                  **({'ssim_weight': ssim_weight} if ssim_weight else {}),
                  **({'noise_dim': noise_dim} if noise_dim else {}),
                  **({'canvas': True} if canvas else {}),
                  **({'d_augment': d_augment} if d_augment else {}))
    for scope in sorted(grad_stats or {}, reverse=True):             # g, then d
        record[scope + '_grad_norm'] = grad_stats[scope]['norm']
        record[scope + '_clip_scale'] = grad_stats[scope]['scale']
    for scope in sorted(clip_bounds or {}, reverse=True):
        record[scope + '_clip_norm'] = clip_bounds[scope]
    for scope in sorted(rates or {}, reverse=True):
        record[scope + '_lr'] = rates[scope]['lr']
    if ss_prob is not None:
        record['ss_prob'] = ss_prob
    return record


def _log_jsonl(path, record):
    with open(path, 'a') as f:
        f.write(json.dumps(record) + '\n')


def train(input_path, output_path, test_output_path, log_dir, model_dir, arg_adv, arg_loss, arg_opt, arg_transform,
          batch_size=64, img_size=64, seq_len=8, ksize=5, train_iter=TRAIN_ITER, pretrain_iter=PRETRAIN_ITER,
          n_critic=None, device='cuda:0', world_size=1, rank=0, process_group=None, log_every=100, quiet=False,
          eval_every=500, resume=None, dtype='f32', sync_bn=False, exact_global_batch=False, dp_collectives=None, buckets=0,
          data_workers='thread', data_threads=None, data_decode='exact', data_frames='selected', data_cache_gb=0.0, synthetic_pool=0,
          num_masks=10, rollout_steps=1, ema_decay=0.0, ssim_weight=0.0, g_clip_norm=0.0, d_clip_norm=0.0, grad_norms=False,
          noise_dim=0, noise_seed=0, g_lr=None, d_lr=None, beta1=None, lr_schedule='constant', lr_warmup=0, lr_decay_steps=0,
          lr_final=0.0, sched_sampling='off', ss_start=1.0, ss_final=0.0, ss_decay_steps=0, ss_seed=0, d_noise=0.0, d_noise_final=0.0,
          d_noise_decay_steps=0, d_noise_seed=0, d_stats=False, canvas=False, posterior=False, kl_weight=1.0, d_augment=None,
          d_augment_seed=0):
    """Training loop of train.py:179-309.  ``input_path``: 'synthetic' (seeded random sequences) or a directory of
    push-dataset TFRecords, read by push_data.PushDataset (the reference's build_tfrecord_input, ops.py:140-223).
    ``dtype``: 'f32', or 'bf16' for the bf16 pipeline of BASELINE configs 3 and 5 (bf16 activations, float32 master weights).
    Data parallel (world_size > 1): ``sync_bn`` - BatchNorm statistics of the global batch; ``exact_global_batch`` -
    the run reproduces one device at the global batch (SyncBN + GDL scaled by the world size + global state-loss norm);
    ``dp_collectives`` - 'side' (default with more than one rank: all-reduces on a second HIP stream, overlapping the rest of
    backward) or 'stream' (in program order on the compute stream); ``buckets`` - all-reduce buckets per optimizer (0 = 2 for
    'side', 1 for 'stream').  ``data_workers`` / ``data_threads``: the TFRecord decode workers (push_data.PushDataset: threads or
    spawned processes filling a bounded prefetch queue, the reference's tf.train.batch(num_threads=batch_size), ops.py:209-213).
    ``data_frames``: 'selected' (default) - the loop tells the dataset batches ahead which frames each step will read and only
    those JPEGs are decoded (same frames, same bits; a step reads 2 of a record's 7) - or 'all' (every frame of every record,
    as the reference's queue runners do).  ``data_decode``: 'exact' (decode -> crop -> box mean, the reference's arithmetic) or
    'dct' (opt-in, approximate: the reduction inside libjpeg's inverse DCT, push_data.decode_frame).  ``data_cache_gb``: keep up to
    that many GiB of decoded frames in host memory - a record that comes round again in a later epoch is not decoded again (same
    bits; 0 = off, as the reference).  ``synthetic_pool``: SyntheticPush(pool=...).  ``arg_transform`` / ``num_masks``: the
    generator, as Trainer takes them ('cdna': the CDNA generator with ``num_masks`` kernels of ``ksize``).  ``rollout_steps`` K > 1:
    every G step (and pretraining step) trains through the generator's own K-step rollout on a window t .. t+K
    (Trainer.train_g_rollout); the D steps are unchanged and the loop takes the plain call path (no look-ahead pass).
    ``ema_decay`` > 0: the Trainer keeps the moving average of the generator's weights (Trainer ``ema_decay``); checkpoints hold
    it, ``train.jsonl`` records ``g_ema``, and the evaluation block also scores the rollout of the averaged weights
    (``rollout_psnr_ema`` / ``rollout_ssim_ema`` in ``test.jsonl``).  Training itself is unchanged.
    ``ssim_weight`` W > 0: the generator's losses carry W / B * sum_b (1 - SSIM_b) (Trainer ``ssim_weight``); ``train.jsonl``
    records ``ssim_weight`` and the summary ``g_ssim_loss``.  Checkpoints and the evaluation block are unchanged.
    ``g_clip_norm`` / ``d_clip_norm`` X > 0: the G / D updates clip their gradient to a global norm of X; ``grad_norms``: measure
    the norms of a scope without a bound too (Trainer, same keywords).  With any of them ``train.jsonl`` records
    ``g_grad_norm`` / ``g_clip_scale`` / ``d_grad_norm`` / ``d_clip_scale`` of the iteration's last updates at every log
    interval (the scopes that are measured) and the configured bounds once, in its first record.  Checkpoints are unchanged.
    ``noise_dim`` Z > 0 / ``noise_seed``: the generator reads Z noise values drawn on the device (Trainer, same keywords); the loop
    takes the plain call path (no look-ahead pass; ``posterior`` / ``kl_weight``: the latent posterior and its KL weight, Trainer,
    same keywords - ``train.jsonl`` then records ``g_kl``), checkpoints hold ``g/noise/state``, ``train.jsonl`` records ``noise_dim`` and
    the evaluation block predicts with z = 0.
    ``g_lr`` / ``d_lr`` / ``beta1``: the rates of the G and D updates and Adam's beta1 (Trainer, same keywords; None: the
    reference's).  ``lr_schedule`` / ``lr_warmup`` / ``lr_decay_steps`` / ``lr_final``: a learning-rate schedule (Trainer, same
    keywords), with ``lr_warmup`` and ``lr_decay_steps`` given in TRAINING ITERATIONS: D's schedule gets them multiplied by its
    updates per iteration (``n_critic``; 5 for the wass loss, else 1), G's gets them as they are.  G's counter also counts the
    ``pretrain_iter`` pretraining updates, so its warmup starts there.  With a schedule ``train.jsonl`` records ``g_lr`` / ``d_lr``,
    the rates of the iteration's last updates, and checkpoints hold the counters; without one both are unchanged.
    ``sched_sampling`` / ``ss_start`` / ``ss_final`` / ``ss_decay_steps`` / ``ss_seed``: scheduled sampling of the K-step updates
    (Trainer, same keywords; needs ``rollout_steps`` > 1), ``ss_decay_steps`` in TRAINING ITERATIONS - there is one K-step update per
    iteration.  The Trainer gets ``ss_offset = pretrain_iter``: the pretraining updates are teacher-forced at ``ss_start`` and the
    decay begins behind them.  With sampling on ``train.jsonl`` records ``ss_prob``, the probability of truth of the iteration's
    update, and checkpoints hold ``g/sched_sampling/state``; a pretraining iteration at a log interval then logs too (``ss_prob`` and
    ``pretrain_g_loss``) and writes the interval's checkpoint.  With sampling off all of this is unchanged.
    ``d_noise`` / ``d_noise_final`` / ``d_noise_decay_steps`` / ``d_noise_seed``: instance noise on the discriminator's inputs (Trainer,
    same keywords; needs ``arg_adv`` and ``rollout_steps`` = 1), ``d_noise_decay_steps`` in TRAINING ITERATIONS: the Trainer gets them
    multiplied by D's updates per iteration, as the learning-rate schedule does (the pretraining iterations update no D: no
    offset).  The loop takes the plain call path (no look-ahead pass) and checkpoints hold ``d/inst_noise/state`` and
    ``d/inst_noise/updates``.  ``d_stats``: ``train.jsonl`` records ``d_fake_logit`` / ``d_real_logit`` / ``d_fake_acc`` /
    ``d_real_acc`` of the interval's last D step and, with ``d_noise`` > 0, its ``d_noise_sigma`` (Trainer ``d_stats``: they are
    summaries).  With both off all of this is unchanged.
    ``canvas``: the CDNA / affine generator composites an image it paints itself (Trainer ``canvas``); ``train.jsonl`` records
    ``canvas`` and checkpoints hold ``g/tconv4_canvas/*``.  Off, all of this is unchanged.
    ``d_augment`` / ``d_augment_seed``: differentiable augmentation of the discriminator's inputs (Trainer, same keywords; needs
    ``arg_adv``, ``rollout_steps`` = 1 and ``dtype`` 'f32').  The loop takes the plain call path (no look-ahead pass), checkpoints
    hold ``d/augment/state`` and ``train.jsonl`` records ``d_augment``, the policy in canonical order.  Off, all of this is
    unchanged."""
    for what, v in (('lr_warmup', lr_warmup), ('lr_decay_steps', lr_decay_steps)):
        if isinstance(v, (tuple, list)):
            raise ValueError('%s is a number of training iterations here, got %r' % (what, v))
    # every option is checked here, before anything is created, and handed to the Trainer once: an option at its "off" value is
    # not passed at all (the Trainer then builds the graph it built before the option existed)
    D_per_G = n_critic if n_critic else (5 if arg_loss == 'wass' else 1)      # train.py:217-220
    options = dict(arg_adv=arg_adv, arg_loss=arg_loss, arg_opt=arg_opt, arg_transform=arg_transform, batch_size=batch_size, img_size=img_size,
                   ksize=ksize, num_masks=num_masks)
    la = check_lr(g_lr, d_lr, beta1, arg_opt, lr_schedule, lr_warmup, lr_decay_steps, lr_final)
    if (g_lr, d_lr, beta1) != (None, None, None):
        options.update(g_lr=la['g_lr'], d_lr=la['d_lr'], beta1=la['beta1'])
    if la['scheduled']:                 # iterations -> updates: D takes D_per_G of them per iteration
        options.update(lr_schedule=la['schedule'], lr_final=la['final'], lr_warmup=(la['warmup'][0], la['warmup'][0] * D_per_G),
                       lr_decay_steps=(la['decay_steps'][0], la['decay_steps'][0] * D_per_G))
    if check_canvas(canvas, model_kind(arg_transform), ksize, num_masks):
        options['canvas'] = True
    noise_dim = check_noise(noise_dim, noise_seed, rollout_steps, False, batch_size)
    if noise_dim:
        options.update(noise_dim=noise_dim, noise_seed=noise_seed)
    posterior, kl_weight = check_posterior(posterior, kl_weight, noise_dim, bf16=dtype != 'f32')
    if posterior:
        options.update(posterior=True, kl_weight=kl_weight)
    ss = check_sched_sampling(sched_sampling, ss_start, ss_final, ss_decay_steps, max(int(pretrain_iter), 0), ss_seed, rollout_steps,
                              batch_size)           # (the pretraining updates count too: the decay begins behind them)
    if ss is not None:
        options.update(sched_sampling=ss['kind'], ss_start=ss['start'], ss_final=ss['final'], ss_decay_steps=ss['decay_steps'],
                       ss_offset=ss['offset'], ss_seed=ss['seed'])
    dn = check_d_noise(d_noise, d_noise_final, d_noise_decay_steps, 0, d_noise_seed, rollout_steps, arg_adv)
    if dn is not None:                  # iterations -> D updates
        options.update(d_noise=dn['start'], d_noise_final=dn['final'], d_noise_decay_steps=dn['decay_steps'] * D_per_G, d_noise_seed=dn['seed'])
    da = check_d_augment(d_augment, d_augment_seed, rollout_steps, arg_adv, bf16=dtype != 'f32')
    if da is not None:
        options.update(d_augment=','.join(da['names']), d_augment_seed=da['seed'])
    if d_stats:
        options['d_stats'] = True
    for key, value in (('ema_decay', check_ema_decay(ema_decay)), ('ssim_weight', check_ssim_weight(ssim_weight))):
        if value:
            options[key] = value
    g_clip_norm, d_clip_norm = check_clip_norm(g_clip_norm, 'g_clip_norm'), check_clip_norm(d_clip_norm, 'd_clip_norm')
    if g_clip_norm or d_clip_norm or grad_norms:
        options.update(g_clip_norm=g_clip_norm, d_clip_norm=d_clip_norm, grad_norms=bool(grad_norms))
    if data_frames not in ('selected', 'all'):
        raise ValueError("data_frames must be 'selected' or 'all'")
    if int(rollout_steps) > 1:          # (the K-step G step takes the plain call path: no pair instance to build)
        check_rollout(rollout_steps, model_kind(arg_transform), bf16=dtype == 'bf16',
                      data_parallel=world_size > 1 or sync_bn or exact_global_batch)
        if int(rollout_steps) > seq_len - 1:
            raise ValueError('rollout_steps %d needs sequences of more than %d frames (seq_len %d)' % (rollout_steps, rollout_steps, seq_len))
        options.update(lookahead=False, rollout_steps=int(rollout_steps))
    np.random.seed(7)                                           # train.py:14
    synthetic = input_path in (None, '', 'synthetic')
    if synthetic:
        data = SyntheticPush(batch_size, seq_len, img_size, rank=rank, pool=synthetic_pool)
    else:
        from .push_data import PushDataset
        data = PushDataset(input_path, batch_size, training=True, img_size=img_size, rank=rank, world_size=world_size,
                           workers=data_workers, num_threads=data_threads, decode=data_decode, cache_bytes=int(data_cache_gb * 2 ** 30))
        seq_len = data.seq_len
    boolean_mask = build_all_mask(seq_len)
    G.reset_default_graph()
    if dp_collectives is None:
        dp_collectives = 'side' if world_size > 1 else 'stream'
    optim.set_data_parallel(world_size, n_buckets=buckets or None, sync_bn=sync_bn, exact_global_batch=exact_global_batch,
                            collectives=dp_collectives)
    sess = G.Session(device=device, world_size=world_size, rank=rank, process_group=process_group, dtype=dtype)
    try:
        trainer = _train_loop(sess, data, input_path, synthetic, boolean_mask, log_dir, model_dir, seq_len, train_iter, pretrain_iter, D_per_G,
                              rank, log_every, quiet, eval_every, resume, select_frames=data_frames == 'selected', options=options)
        sess.rt.check_exchange_flags()     # a last look at the device-side flags of the iterations since the last log interval
    except BaseException:
        sess.close(check=False)            # tear the transport down; the exception on its way out is the one to report
        raise
    finally:
        if hasattr(data, 'close'):
            data.close()                   # PushDataset: stop the decode workers and the feeder thread
    # The session stays OPEN: the returned Trainer is usable (evaluation, more steps, reading variables).  Its owner closes it -
    # `trainer.sess.close()` (main() does): ncclCommDestroy under data parallelism and a last check of the device-side flags.
    return trainer


def _train_loop(sess, data, input_path, synthetic, boolean_mask, log_dir, model_dir, seq_len, train_iter, pretrain_iter, D_per_G, rank,
                log_every, quiet, eval_every, resume, select_frames=True, options=None):
    """The loop of ``train``: ``options`` are the Trainer's keywords as ``train`` checked and converted them; what the loop logs or
    branches on it reads from the Trainer it builds."""
    trainer = Trainer(sess, **options)
    batch_size, img_size, rollout_steps = trainer.batch_size, trainer.img_size, trainer.rollout_steps
    sampling, scheduled = trainer.sched_sampling is not None, trainer.lr_args['scheduled']
    sess.run(G.global_variables_initializer())
    saver = Saver()                                                           # train.py:215
    if resume:
        saver.restore(sess, resume)
    if synthetic:
        eval_data = SyntheticPush(batch_size, seq_len, img_size, seed=1007, rank=rank)
    else:
        from .push_data import PushDataset
        try:                                                                  # validation files: the tail of the split
            eval_data = PushDataset(input_path, batch_size, training=False, img_size=img_size, seed=1007)
        except RuntimeError:
            eval_data = PushDataset(input_path, batch_size, training=True, img_size=img_size, seed=1007)
    log_file = os.path.join(log_dir, 'train.jsonl') if log_dir else None
    t0 = time.time()
    bounds_logged = False
    selections = _PairSelections(boolean_mask, batch_size, D_per_G, pretrain_iter, train_iter, data if select_frames else None,
                                 rollout_steps=rollout_steps)
    for i in range(train_iter):
        sels = selections.next()
        if i < pretrain_iter:
            inp, nxt, acts, states = data.get_batch()
            if rollout_steps > 1:
                pre_loss = trainer.pretrain_g_rollout(*window_batch(sels[0], inp, nxt, acts, states))
                if sampling and i % log_every == 0 and rank == 0:
                    # scheduled sampling: ss_prob at EVERY log interval, the pretraining iterations' included (they advance the counter
                    # the checkpoint holds), with the interval's checkpoint
                    if log_file:
                        _log_jsonl(log_file, train_record({'pretrain_g_loss': pre_loss}, i, time.time() - t0, rollout_steps,
                                                          ss_prob=trainer.sched_sampling_last()['prob']))
                    if model_dir:
                        saver.save(sess, os.path.join(model_dir, 'model{:d}'.format(i)), background=True)
            else:
                sm, em = sels[0]
                trainer.pretrain_g(inp[sm], nxt[em], acts[sm], states[em])
            if not quiet:
                print('pre-train iter: ' + str(i))
            continue
        if rollout_steps > 1:
            summ = _rollout_iteration(trainer, data, sels, i, D_per_G, log_every)
        else:
            # The iteration's sub-steps, drawn up front in the reference's order (train.py:241-259: per D step a fresh batch and a
            # fresh frame-pair selection, then a NEW selection on the last batch for the G step; the steps themselves draw nothing;
            # the selections come from _PairSelections, which drew them some iterations ago in that same order),
            # so that a step can announce its successor's inputs to Trainer.train_d (look-ahead generator pass): D1 runs the
            # generator for D1 and D2, D2 runs none, ... the last pair pass covers the G step.  Logging iterations keep the plain path
            # for their last D step (its summaries read that step's own generated frames).
            subs = []
            for j in range(D_per_G):
                inp, nxt, acts, states = data.get_batch()
                sm, em = sels[j]
                subs.append((inp[sm], nxt[em], acts[sm]))
            smg, emg = sels[-1]
            g_in, g_act = inp[smg], acts[smg]
            summ, carried = None, False
            for j, (x_d, y_d, a_d) in enumerate(subs):
                last = j == D_per_G - 1
                summarize = (i % log_every == 0) and last
                follow = None
                if not carried and not summarize:                    # this step runs the pair pass for itself and its successor
                    follow = (g_in, g_act) if last else ((subs[j + 1][0], subs[j + 1][2]) if not ((i % log_every == 0) and j + 1 == D_per_G - 1) else None)
                summ = trainer.train_d(x_d, y_d, a_d, summarize=summarize, next_d=follow)
                carried = follow is not None and not carried
            # (the generated frames stay on the device: the reference fetches them every step only to dump samples at i % 100 == 0,
            # train.py:130,269-273, which this loop does not do - no D2H copy, no synchronisation per iteration)
            trainer.train_g(g_in, nxt[emg], g_act, states[emg], device_fetch=True)
        if i % log_every == 0:
            # the fetches above synchronised anyway: look at the device-side flags of the one-launch BatchNorm kernels HERE, on
            # every rank, so that a step that ran on wrong statistics fails now - before anything of it is logged or
            # checkpointed - and not at exit, thousands of iterations later (graph.Runtime.check_exchange_flags)
            sess.rt.check_exchange_flags()
        if i % log_every == 0 and rank == 0:
            if not quiet:
                print('Iteration {:d}'.format(i))
            if log_file and summ:
                stats = {sc: trainer.grad_norm_stats(sc) for sc, norm in trainer.grad_norm.items() if norm is not None}
                bounds = None if bounds_logged or not stats else {'g': trainer.g_clip_norm, 'd': trainer.d_clip_norm}
                _log_jsonl(log_file, train_record(summ, i, time.time() - t0, rollout_steps, trainer.ema_decay, trainer.ssim_weight, stats, bounds,
                                                    trainer.noise_dim, trainer.learning_rates() if scheduled else None,
                                                    ss_prob=trainer.sched_sampling_last()['prob'] if sampling else None,
                                                    canvas=trainer.canvas,
                                                    d_augment=','.join(trainer.d_augment['names']) if trainer.d_augment else None))
                bounds_logged = True
            if model_dir:
                saver.save(sess, os.path.join(model_dir, 'model{:d}'.format(i)), background=True)      # train.py:274; written by a writer thread
        if eval_every and i % eval_every == 0 and rank == 0:
            # recursive rollout over T-1 steps on held-out sequences (train.py:278-309; defect D7: own states)
            t_img, _, t_acts, _ = eval_data.get_batch()

            def score(weights):
                """-> (summaries of step 0, PSNR per step, SSIM per step or None) of the rollout with ``weights``."""
                predicted, e_summ = trainer.test_sequence(t_img, t_img, t_acts, weights=weights)
                psnr = [float(10.0 * np.log10(1.0 / max(np.mean((predicted[:, j] - t_img[:, j + 1]) ** 2), 1e-30)))
                        for j in range(predicted.shape[1])]
                if not log_file:
                    return e_summ, psnr, None
                # SSIM per step (mean over the batch) by the GPU kernel (metrics.frame_metrics) on the same predictions
                ssim, _ = frame_metrics(sess.upload(predicted), sess.upload(np.asarray(t_img[:, 1:predicted.shape[1] + 1], np.float32)))
                return e_summ, psnr, [float(v) for v in ssim.mean(dim=0, dtype=torch.float64).cpu().numpy()]
            e_summ, psnr, ssim = score('raw')
            if log_file:
                record = dict(e_summ or {}, iteration=i, rollout_psnr=psnr, rollout_ssim=ssim)
                if trainer.ema is not None and trainer.ema_updates() > 0:      # the same sequences through the averaged weights
                    _, record['rollout_psnr_ema'], record['rollout_ssim_ema'] = score('ema')
                _log_jsonl(os.path.join(log_dir, 'test.jsonl'), record)
    if hasattr(eval_data, 'close'):
        eval_data.close()
    saver.wait()                     # the last checkpoints are on disk when train() returns
    return trainer


def _rollout_iteration(trainer, data, sels, i, D_per_G, log_every):
    """One iteration after pretraining with rollout_steps > 1 -> the summaries of its last D step (or None).  The D steps take
    their pair selections on fresh batches as the one-step loop does, on its plain call path; the G step trains through the
    K-step rollout on the window its selection draws on the last D batch (train.py:258-259's order)."""
    summ = None
    for j in range(D_per_G):
        inp, nxt, acts, states = data.get_batch()
        sm, em = sels[j]
        summ = trainer.train_d(inp[sm], nxt[em], acts[sm], summarize=(i % log_every == 0) and j == D_per_G - 1)
    trainer.train_g_rollout(*window_batch(sels[-1], inp, nxt, acts, states), device_fetch=True)
    return summ


def _flag(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ('true', '1', 'yes'):
        return True
    if v.lower() in ('false', '0', 'no'):
        return False
    raise argparse.ArgumentTypeError('boolean expected')


def add_model_args(parser):
    """The generator flags shared by this CLI, evaluate's and plan's: --dna (the reference's), --cdna, --affine, --num_masks and
    --canvas."""
    for kind in M.KINDS.values():
        if kind.flag:
            parser.add_argument('--' + kind.flag, nargs='?', const=True, default=False, type=_flag, help=kind.help)
    parser.add_argument('--num_masks', type=int, default=10, help='CDNA kernels / affine transforms, and their masks (1..32)')
    parser.add_argument('--canvas', nargs='?', const=True, default=False, type=_flag,
                        help='--cdna / --affine: composite an image the generator paints itself as one more candidate (--num_masks <= 31)')


def check_model_args(parser, args):
    """parser.error for generator flags that do not go together, and for what the generator they name does not take (before
    anything is created); -> Trainer's arg_transform."""
    if args.num_masks not in M.NUM_MASKS:
        parser.error('--num_masks must be in 1..32')
    try:
        transform = M.transform_argument(vars(args), '--%s')
        kind = M.KINDS[model_kind(transform)]
        kind.check_args(args.ksize, args.num_masks, args.canvas)
    except ValueError as e:
        parser.error(str(e))
    if kind.float32_only and args.dtype == 'bf16':
        parser.error('the %s generator is float32 only (--dtype bf16)' % kind.label)
    return transform


def check_rollout_args(parser, args):
    """parser.error for a --rollout_steps the K-step trainer does not take (before anything is created)."""
    k = args.rollout_steps
    if k < 1:
        parser.error('--rollout_steps must be >= 1')
    if k == 1:
        return
    if k > args.seq_len - 1:
        parser.error('--rollout_steps %d needs sequences of more than %d frames (--seq_len %d)' % (k, k, args.seq_len))
    try:
        check_rollout(k, model_kind(M.transform_argument(vars(args))))      # (the Trainer's own refusal of a generator)
    except ValueError as e:
        parser.error('--%s' % e)
    if args.dtype == 'bf16':
        parser.error('--rollout_steps > 1 is float32 only (--dtype bf16)')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        parser.error('--rollout_steps > 1 runs on one rank (WORLD_SIZE %s)' % os.environ['WORLD_SIZE'])
    if args.sync_bn:
        parser.error('--rollout_steps > 1 runs on one rank (--sync_bn)')
    if args.exact_global_batch:
        parser.error('--rollout_steps > 1 runs on one rank (--exact_global_batch)')


def add_noise_args(parser):
    """The noise flags shared by this CLI and evaluate's: --noise_dim and --noise_seed."""
    parser.add_argument('--noise_dim', type=int, default=0, metavar='Z',
                        help='give the generator Z noise values per sample, drawn on the device inside the step (1..64; 0 = off, the '
                             'deterministic generator); evaluate takes the same --noise_dim')
    parser.add_argument('--noise_seed', type=int, default=0, metavar='S', help='seed of the noise stream (0 <= S < 2^64)')


def check_noise_args(parser, args):
    """parser.error for a --noise_dim / --noise_seed the Trainer does not take (before anything is created)."""
    try:
        check_noise(args.noise_dim, args.noise_seed, getattr(args, 'rollout_steps', 1), False, args.batch_size)
    except ValueError as e:
        parser.error('--noise_dim / --noise_seed: %s' % e)


def add_posterior_args(parser, training=True):
    """The flags of the latent posterior, beside the noise flags: --posterior, shared by this CLI and evaluate's, and --kl_weight
    (``training``: this CLI alone)."""
    parser.add_argument('--posterior', nargs='?', const=True, default=False, type=_flag,
                        help='train an encoder q(z | x_t, x_t+1) of the noise input with a KL term towards the N(0, 1) prior (the VAE '
                             'half of a VAE-GAN; needs --noise_dim; float32); evaluate takes the same --posterior' if training else
                             'build the encoder of a run trained with --posterior (needs --noise_dim): --noise posterior / '
                             'posterior_mean then draw z from it')
    if training:
        parser.add_argument('--kl_weight', type=float, default=1.0, metavar='W',
                            help="weight of KL / batch in the G loss and the pretraining loss (1 = the ELBO's own weight against the "
                                 'summed-L1 reconstruction term: a starting point, not a tuned value)')


def check_posterior_args(parser, args):
    """parser.error for a --posterior / --kl_weight the Trainer does not take (before anything is created; behind
    check_noise_args, whose refusals of --rollout_steps > 1 cover the posterior too)."""
    try:
        check_posterior(args.posterior, getattr(args, 'kl_weight', 1.0), args.noise_dim, bf16=getattr(args, 'dtype', 'f32') != 'f32')
    except ValueError as e:
        parser.error('--posterior / --kl_weight: %s' % e)


def add_sched_sampling_args(parser):
    """The scheduled-sampling flags of --rollout_steps > 1."""
    parser.add_argument('--sched_sampling', type=str, default='off', metavar='KIND',
                        help='off, constant, linear or inverse_sigmoid: at every fed-back position of a K-step update a coin per sample '
                             'feeds the next step the true frame and state instead of the predicted ones, with a probability that '
                             'follows this schedule (needs --rollout_steps > 1; drawn on the device inside the step)')
    parser.add_argument('--ss_start', type=float, default=1.0, metavar='P', help='probability of truth at the start (and of constant)')
    parser.add_argument('--ss_final', type=float, default=0.0, metavar='P', help='probability of truth at the end of the decay')
    parser.add_argument('--ss_decay_iters', type=int, default=0, metavar='N',
                        help='training iterations over which the probability decays, counted behind --pretrain_iter')
    parser.add_argument('--ss_seed', type=int, default=0, metavar='S', help='seed of the coins (0 <= S < 2^64)')


def add_d_noise_args(parser):
    """The flags of the instance noise on the discriminator's inputs, and of the statistics to choose its level by."""
    parser.add_argument('--d_noise', type=float, default=0.0, metavar='S',
                        help='add Gaussian noise of standard deviation S to every frame the discriminator judges, real and generated, '
                             'drawn on the device inside the step (instance noise; 0 = off; needs --adv)')
    parser.add_argument('--d_noise_final', type=float, default=0.0, metavar='F', help='the level at the end of the decay')
    parser.add_argument('--d_noise_decay_iters', type=int, default=0, metavar='N',
                        help='training iterations over which the level moves linearly from S to F (0: constant S)')
    parser.add_argument('--d_noise_seed', type=int, default=0, metavar='SEED', help='seed of the instance noise (0 <= SEED < 2^64)')
    parser.add_argument('--log_d_stats', nargs='?', const=True, default=False, type=_flag,
                        help="record the discriminator's mean logits and accuracies on the generated and the real half in train.jsonl "
                             '(d_fake_logit, d_real_logit, d_fake_acc, d_real_acc) and, with --d_noise, d_noise_sigma')


def add_d_augment_args(parser):
    """The flags of the differentiable augmentation of the discriminator's inputs."""
    parser.add_argument('--d_augment', type=str, default=None, metavar='LIST',
                        help='put every pair the discriminator judges, real and generated, through random transforms drawn on the '
                             'device inside the step, and the generator\'s gradient through their adjoint (DiffAugment): a '
                             'comma-separated subset of color, translation, cutout (needs --adv; float32 only)')
    parser.add_argument('--d_augment_seed', type=int, default=0, metavar='SEED', help='seed of the augmentation parameters (0 <= SEED < 2^64)')


def add_lr_args(parser):
    """The learning-rate flags: the rates of G and D, Adam's beta1 and the schedule."""
    parser.add_argument('--g_lr', type=float, default=None, metavar='LR', help='learning rate of the generator updates (default: 1e-3 for adam, 5e-5 for rmsprop)')
    parser.add_argument('--d_lr', type=float, default=None, metavar='LR', help='learning rate of the discriminator updates (same default)')
    parser.add_argument('--beta1', type=float, default=None, metavar='B', help="Adam's beta1 for every update (0 <= B < 1; default 0.9; --opt adam only)")
    parser.add_argument('--lr_schedule', type=str, default='constant',
                        help='constant, linear, cosine or exponential: how the rates decay behind the warmup, evaluated on the device '
                             'inside the optimizer launch (constant with --lr_warmup 0: off)')
    parser.add_argument('--lr_warmup', type=int, default=0, metavar='N', help='raise the rates linearly over the first N training iterations')
    parser.add_argument('--lr_decay_iters', type=int, default=0, metavar='N', help='training iterations over which the rates decay (behind the warmup)')
    parser.add_argument('--lr_final', type=float, default=0.0, metavar='F',
                        help='the rates end at F x their value (0 <= F <= 1; exponential: F x per --lr_decay_iters iterations, 0 < F)')


def main(argv=None):
    parser = argparse.ArgumentParser(description='action-conditioned video-prediction GAN on MI355X')
    parser.add_argument('input_path', type=str)
    parser.add_argument('output_path', type=str)
    parser.add_argument('--adv', nargs='?', const=True, default=False, type=_flag)
    parser.add_argument('--loss', type=str, default='bce')
    parser.add_argument('--opt', type=str, default='adam')
    add_model_args(parser)
    parser.add_argument('--batch_size', type=int, default=64)
    parser.add_argument('--img_size', type=int, default=64)
    parser.add_argument('--seq_len', type=int, default=8)
    parser.add_argument('--ksize', type=int, default=5)
    parser.add_argument('--n_critic', type=int, default=None)
    parser.add_argument('--train_iter', type=int, default=TRAIN_ITER)
    parser.add_argument('--pretrain_iter', type=int, default=PRETRAIN_ITER)
    parser.add_argument('--dtype', type=str, default='f32', choices=['f32', 'bf16'])
    parser.add_argument('--rollout_steps', type=int, default=1,
                        help='train the generator through its own K-step rollouts (frames and states fed back; 1 = one-step pairs)')
    # data parallel (one process per GPU under torch.distributed.run; no reference counterpart - SURVEY 8(e))
    parser.add_argument('--sync_bn', nargs='?', const=True, default=False, type=_flag,
                        help='BatchNorm statistics of the GLOBAL batch (one small all-reduce per BatchNorm layer and direction)')
    parser.add_argument('--exact_global_batch', nargs='?', const=True, default=False, type=_flag,
                        help='reproduce ONE device at the global batch: SyncBN + GDL scaled by the world size + global state-loss norm')
    parser.add_argument('--dp_collectives', type=str, default=None, choices=['stream', 'side'],
                        help="gradient all-reduces in program order on the compute stream, or on a side HIP stream overlapping "
                             "the rest of backward (default with more than one rank)")
    parser.add_argument('--buckets', type=int, default=0, help='all-reduce buckets per optimizer (0: 2 for side, 1 for stream)')
    parser.add_argument('--data_workers', type=str, default='process', choices=['thread', 'process'],
                        help='TFRecord decode workers: spawned processes (default here: 2.3x the rate of threads on the GPU box, '
                             'profiles/r5/d_train_loop.txt) or threads (the default of train() / PushDataset: no __main__ guard needed)')
    parser.add_argument('--data_threads', type=int, default=None, help='number of decode workers (default: batch size, at most 16)')
    parser.add_argument('--data_frames', type=str, default='selected', choices=['selected', 'all'],
                        help="decode only the frames a step will read (same frames, same bits) or every frame of every record")
    parser.add_argument('--data_cache_gb', type=float, default=8.0,
                        help='GiB of host memory for decoded frames: a record seen in an earlier epoch is served from memory (same bits; '
                             '0 = decode every time as the reference; the 64x64 push training set is ~17 GiB decoded)')
    parser.add_argument('--data_decode', type=str, default='exact', choices=['exact', 'dct'],
                        help="'dct': approximate 8x reduction inside libjpeg's inverse DCT (3x cheaper; within 2-3 levels of 255)")
    parser.add_argument('--g_ema', type=float, default=0.0, metavar='DECAY',
                        help='keep an exponential moving average of the generator weights with this decay (0 < DECAY < 1; 0 = off): '
                             'checkpoints hold it, the evaluation block also scores it, evaluate --weights ema predicts with it')
    parser.add_argument('--ssim_weight', type=float, default=0.0, metavar='W',
                        help='add W / B * sum_b (1 - SSIM_b) of the generated frame against the next frame to the generator\'s '
                             'reconstruction loss (0 = off; the L1 term is a SUM over the 12 288 values of a frame, so a useful W is in '
                             'the tens to hundreds)')
    parser.add_argument('--g_clip_norm', type=float, default=0.0, metavar='X',
                        help='clip the gradient of every generator update to a global norm of X (tf.clip_by_global_norm; 0 = off)')
    parser.add_argument('--d_clip_norm', type=float, default=0.0, metavar='X',
                        help='clip the gradient of every discriminator update to a global norm of X (0 = off; needs --adv)')
    parser.add_argument('--log_grad_norms', nargs='?', const=True, default=False, type=_flag,
                        help='record the gradient norms of G and D in train.jsonl (g_grad_norm, d_grad_norm, ..._clip_scale), also '
                             'where no bound is set')
    add_noise_args(parser)
    add_posterior_args(parser)
    add_lr_args(parser)
    add_sched_sampling_args(parser)
    add_d_noise_args(parser)
    add_d_augment_args(parser)
    args = parser.parse_args(argv)
    if args.buckets < 0:
        parser.error('--buckets must be >= 0')
    transform = check_model_args(parser, args)
    check_rollout_args(parser, args)
    check_noise_args(parser, args)
    check_posterior_args(parser, args)
    # every other option: the check train() makes, its ValueError reported under the flags' names ({}: the check's own words)
    for message, check in (
            ('--g_lr / --d_lr / --beta1 / --lr_*: {}', lambda: check_lr(args.g_lr, args.d_lr, args.beta1, args.opt, args.lr_schedule,
                                                                        args.lr_warmup, args.lr_decay_iters, args.lr_final)),
            ('--ssim_weight must be finite and >= 0, got %r' % args.ssim_weight, lambda: check_ssim_weight(args.ssim_weight)),
            ('--g_ema must be 0 (off) or lie in (0, 1), got %r' % args.g_ema, lambda: check_ema_decay(args.g_ema)),
            ('--g_clip_norm must be finite and >= 0, got %r' % args.g_clip_norm, lambda: check_clip_norm(args.g_clip_norm)),
            ('--d_clip_norm must be finite and >= 0, got %r' % args.d_clip_norm, lambda: check_clip_norm(args.d_clip_norm)),
            ('--sched_sampling / --ss_*: {}', lambda: check_sched_sampling(args.sched_sampling, args.ss_start, args.ss_final, args.ss_decay_iters,
                                                                           0, args.ss_seed, args.rollout_steps, args.batch_size)),
            ('--d_noise / --d_noise_*: {}', lambda: check_d_noise(args.d_noise, args.d_noise_final, args.d_noise_decay_iters, 0,
                                                                   args.d_noise_seed, args.rollout_steps, args.adv)),
            ('--d_augment / --d_augment_seed: {}', lambda: check_d_augment(args.d_augment, args.d_augment_seed, args.rollout_steps, args.adv,
                                                                           bf16=args.dtype != 'f32'))):
        try:
            check()
        except ValueError as e:
            parser.error(message.format(e))
    model_dir = os.path.join(args.output_path, 'models')
    log_dir = os.path.join(args.output_path, 'logs')
    os.makedirs(args.output_path)
    os.makedirs(model_dir)
    os.makedirs(log_dir)
    world_size, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world_size > 1:
        # control plane only (bootstrap of the RCCL communicator, comm.py): gradients never go through torch.distributed
        torch.cuda.set_device(local_rank)
        torch.distributed.init_process_group('gloo')
    # every other flag is a keyword of train() under its own name, but for these four
    options = {k: v for k, v in vars(args).items() if k not in ['input_path', 'output_path', 'adv', 'loss', 'opt'] + M.flags()}
    for flag, keyword in (('g_ema', 'ema_decay'), ('log_grad_norms', 'grad_norms'), ('lr_decay_iters', 'lr_decay_steps'),
                          ('ss_decay_iters', 'ss_decay_steps'), ('d_noise_decay_iters', 'd_noise_decay_steps'), ('log_d_stats', 'd_stats')):
        options[keyword] = options.pop(flag)
    trainer = train(args.input_path, os.path.join(args.output_path, 'train_output'), os.path.join(args.output_path, 'test_output'),
                    log_dir, model_dir, args.adv, args.loss, args.opt, transform, device='cuda:%d' % local_rank, world_size=world_size,
                    rank=rank, **options)
    if trainer is not None:
        trainer.sess.close()        # ncclCommDestroy under data parallelism + a last check of the device-side flags


if __name__ == '__main__':
    main()
