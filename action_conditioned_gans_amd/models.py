"""Generator / discriminator builders with the reference's signatures (models.py:8, 24-29, 76-78).

Each network is a short table of (scope, width) rows walked under an ``arg_scope`` that carries the
slim defaults the reference sets (stride 2, SAME, batch_norm, relu / lrelu); the rows that deviate
(heads without BatchNorm, the VALID state head, d/conv6 without activation) override per call.
Variables are named exactly as slim names them (``g/conv1/weights``, ``g/conv1/BatchNorm/beta``,
``g/tconv4/biases``), so ``reuse=True`` shares them across calls.

Deviations from the reference text, which does not run as committed:
  D2  ``slim.argscope`` is read as ``slim.arg_scope``.
  D3  the discriminator tiles its actions to its own conv2 output size, not to 4x4.
  D9  ``ksize`` is honoured (default 5) and H, W come from the tensor instead of a literal 64.
``images.padded`` (optional attribute): the same frames stored with a channel pitch of 4; g/conv1 then gathers
with 16-byte loads.  Actions may be given as ``[B, A]`` (tiled and concatenated in one fused op) or already tiled
``[B, h, w, A]`` as the reference Trainer passes them (train.py:48-50).
"""
import typing

from . import graph as G
from . import ops as O

G_PLAIN = {'encoder': (('conv1', 64), ('conv2', 128), ('conv3', 256), ('conv4', 512)),
           'decoder': (('tconv1', 256), ('tconv2', 128), ('tconv3', 64))}
G_DNA = {'encoder': (('conv1', 32), ('conv2', 64), ('conv3', 128), ('conv4', 256)),
         'decoder_a': (('tconv1', 128), ('tconv2', 128)),
         'state': (('sconv3', 32), ('sconv4', 16)),
         'decoder_b': (('tconv3', 128),)}
Q_NET = (('conv1', 32), ('conv2', 64), ('conv3', 128), ('conv4', 256))
D_NET = {'pre': (('conv1', 64), ('conv2', 128)), 'post': (('conv3', 128), ('conv4', 256), ('conv5', 512))}


def _with_actions(features, actions, name):
    """Channel-concatenate the action/state vector, broadcast over the feature map."""
    if len(actions.shape) == 2:
        return O.concat_actions(features, actions, name=name)
    if len(actions.shape) == 4 and actions.shape[1:3] == features.shape[1:3]:
        if O.half_mode():
            raise NotImplementedError('bf16 graphs take the actions as [B, A] (tiled and concatenated in one fused op)')
        return O.concat([features, actions], axis=3, name=name)
    raise ValueError('actions %s cannot be concatenated with a %s feature map' % (actions.shape, features.shape))


def _stack(net, rows, layer, size=5):
    for scope, width in rows:
        net = layer(net, width, [size, size], scope=scope)
    return net


def build_generator(images, actions, reuse=False):
    """Plain generator (models.py:8-22): 4 conv down, actions, 3 deconv up, deconv + bias + tanh."""
    with O.variable_scope('g', reuse=reuse), \
            O.arg_scope([O.conv2d, O.deconv2d], activation_fn=O.relu, stride=2, padding='SAME',
                        normalizer_fn=O.batch_norm, reuse=reuse):
        net = _stack(getattr(images, 'padded', images), G_PLAIN['encoder'], O.conv2d)
        net = _with_actions(net, actions, 'actions')
        net = _stack(net, G_PLAIN['decoder'], O.deconv2d)
        return O.deconv2d(net, images.shape[3], [5, 5], activation_fn=O.tanh, normalizer_fn=None, scope='tconv4')


def _check_images(images, batch_size, color_channels):
    if batch_size is not None and batch_size != images.shape[0]:
        raise ValueError('batch_size %r does not match images %s' % (batch_size, images.shape))
    if images.shape[3] != color_channels:
        raise ValueError('color_channels %r does not match images %s' % (color_channels, images.shape))


def _state_head(net):
    """The 5-d next state from the decoder's 16x16 features.  It reads nothing of what the frame decoder does next: a side chain
    (five tiny latency-bound layers that hide behind tconv3 / tconv4 / the frame's last op, forward and backward)."""
    with G.get_default_graph().side_branch():
        state = _stack(net, G_DNA['state'], O.conv2d, size=3)
        sk = state.shape[1]           # 4 at 64x64: the reference's 4x4 VALID head (models.py:44-51)
        state = O.conv2d(state, 5, [sk, sk], activation_fn=None, stride=1, padding='VALID', normalizer_fn=None,
                         scope='sconv5')
        return O.squeeze(state, axis=(1, 2))       # [B, 1, 1, 5] -> [B, 5], also at B = 1


def build_generator_transform(images, actions, batch_size=None, reuse=False, color_channels=3, ksize=5):
    """DNA generator (models.py:24-74): predicts k*k per-pixel kernel logits and a 5-d next state.

    Returns ``(frame, state)``; ``batch_size`` is accepted for signature compatibility (the static
    shape already carries it).
    """
    _check_images(images, batch_size, color_channels)
    KINDS['dna'].check_args(ksize, None)
    with O.variable_scope('g', reuse=reuse), \
            O.arg_scope([O.conv2d, O.deconv2d], activation_fn=O.relu, stride=2, padding='SAME',
                        normalizer_fn=O.batch_norm, reuse=reuse):
        net = _stack(getattr(images, 'padded', images), G_DNA['encoder'], O.conv2d)
        net = _with_actions(net, actions, 'actions')
        net = _stack(net, G_DNA['decoder_a'], O.deconv2d)
        state = _state_head(net)
        net = _stack(net, G_DNA['decoder_b'], O.deconv2d)
        logits = O.deconv2d(net, ksize * ksize, [5, 5], activation_fn=None, normalizer_fn=None, scope='tconv4')
        frame = O.dna_gather(logits, images, ksize)
        return frame, state


def build_generator_cdna(images, actions, batch_size=None, reuse=False, color_channels=3, num_masks=10, ksize=5, canvas=False):
    """CDNA generator: the DNA generator's trunk with the reference's ``cdna_transformation`` (ops.py:52-98, which none of
    its models calls) as the motion model.  Returns ``(frame, state)``.

    ``cdna_params``, a linear layer (bias, no BatchNorm or activation) on the action-conditioned bottleneck h0
    [B, S/16, S/16, 266] - stored as a VALID S/16 x S/16 conv, ``g/cdna_params/weights`` [S/16, S/16, 266, k*k*M], the same
    numbers as slim's [S/16 * S/16 * 266, k*k*M] in reshape order - predicts M = ``num_masks`` k x k kernels per sample.
    tconv1, tconv2, the state head and tconv3 are the DNA generator's; ``tconv4`` (5x5/2, bias only) gives M+1 mask logits.
    The frame is s_0 * images + sum_j s_{j+1} * T_j with s = softmax over the M+1 channels and T_j the pieces of
    cdna_transformation (its channel split kept as written), in one fused kernel (ops.cdna_composite).

    Two differences from the CDNA model of the paper the push dataset comes from: without ``canvas`` there is no image
    generated from scratch among the composited candidates, and the masks come from the 5x5/2 ``tconv4`` instead of a 1x1
    layer.  ``canvas=True`` adds that image (see _mask_generator): ``tconv4`` then gives M+2 mask logits, a new layer
    ``g/tconv4_canvas`` paints the candidate, and the frame gains s_{M+1} * canvas; 1 <= ``num_masks`` <= 31 then.
    float32 only; ``ksize`` 3, 5 or 7, 1 <= ``num_masks`` <= 32, image size a multiple of 16."""
    return _mask_generator(KINDS['cdna'], images, actions, batch_size, reuse, color_channels, ksize, num_masks,
                           'cdna_params', ksize * ksize * num_masks,
                           lambda logits, params, **kw: O.cdna_composite(logits, images, params, num_masks, ksize, **kw), canvas)


def _mask_generator(kind, images, actions, batch_size, reuse, color_channels, ksize, num_masks, scope, width, composite,
                    canvas=False):
    """The CDNA and the affine generators: what generator ``kind`` does not take is refused before anything is created; then
    the DNA generator's layers, a linear layer ``scope`` of ``width`` outputs per sample on the action-conditioned bottleneck,
    tconv4 to M+1 mask logits and ``composite(logits, params)``.
    ``canvas``: tconv4 gives M+2 mask logits, and ``tconv4_canvas`` - a 5x5/2 deconvolution of the same ``tconv3`` output to
    ``color_channels``, bias only, tanh, as the plain generator's tconv4 is - paints an image that the composite takes as one
    more candidate, ``composite(logits, params, canvas=image)``, under mask channel M+1."""
    _check_images(images, batch_size, color_channels)
    kind.check_args(ksize, num_masks, canvas)
    if images.shape[1] % 16 or images.shape[2] % 16:
        raise ValueError('%s generator: image size %s is not a multiple of 16' % (kind.label, images.shape[1:3]))
    if kind.float32_only and O.half_mode():
        raise NotImplementedError('the %s generator is float32 only' % kind.label)
    with O.variable_scope('g', reuse=reuse), \
            O.arg_scope([O.conv2d, O.deconv2d], activation_fn=O.relu, stride=2, padding='SAME',
                        normalizer_fn=O.batch_norm, reuse=reuse):
        net = _stack(getattr(images, 'padded', images), G_DNA['encoder'], O.conv2d)
        net = _with_actions(net, actions, 'actions')
        params = O.conv2d(net, width, [net.shape[1], net.shape[2]], activation_fn=None, stride=1, padding='VALID',
                          normalizer_fn=None, scope=scope)
        params = params.reshape((images.shape[0], width))
        net = _stack(net, G_DNA['decoder_a'], O.deconv2d)
        state = _state_head(net)
        net = _stack(net, G_DNA['decoder_b'], O.deconv2d)
        logits = O.deconv2d(net, num_masks + (2 if canvas else 1), [5, 5], activation_fn=None, normalizer_fn=None, scope='tconv4')
        if not canvas:
            return composite(logits, params), state
        painted = O.deconv2d(net, color_channels, [5, 5], activation_fn=O.tanh, normalizer_fn=None, scope='tconv4_canvas')
        return composite(logits, params, canvas=painted), state


def build_generator_affine(images, actions, batch_size=None, reuse=False, color_channels=3, num_masks=10, canvas=False):
    """Affine (STP) generator: ``build_generator_cdna`` with a 2x3 affine transform per mask in place of a k x k kernel.
    Returns ``(frame, state)``.

    ``g/affine_params`` (weights [S/16, S/16, 266, 6*M], biases, default initialisers) stands where ``g/cdna_params`` does and
    predicts M = ``num_masks`` transforms per sample, read as theta = params + (1, 0, 0, 0, 1, 0): zero parameters are the
    identity.  The frame is s_0 * images + sum_m s_{m+1} * T_m with T_m the image warped by theta_m, bilinear with zeros
    outside (include/acgan_cdna.h has the formula), in one fused kernel (ops.affine_composite).  Rotation, scale and shear of
    an object take 6 numbers here; the k x k kernels of DNA / CDNA cannot move anything further than (k-1)/2 pixels.
    As for CDNA there is no image generated from scratch among the candidates unless ``canvas=True`` adds one (as
    build_generator_cdna does; 1 <= ``num_masks`` <= 31 then), and the masks come from the 5x5/2 ``tconv4``.
    float32 only; 1 <= ``num_masks`` <= 32, image size a multiple of 16."""
    return _mask_generator(KINDS['affine'], images, actions, batch_size, reuse, color_channels, None, num_masks,
                           'affine_params', 6 * num_masks,
                           lambda logits, params, **kw: O.affine_composite(logits, images, params, num_masks, **kw), canvas)


def build_discriminator(inputs, actions, reuse=False):
    """Discriminator (models.py:76-89): 5 x [conv5x5/2 + BN + lrelu], actions after conv2, 2x2 logit conv + BN."""
    with O.variable_scope('d', reuse=reuse), \
            O.arg_scope([O.conv2d], activation_fn=O.lrelu, stride=2, padding='SAME', normalizer_fn=O.batch_norm,
                        reuse=reuse):
        net = _stack(inputs, D_NET['pre'], O.conv2d)
        if len(actions.shape) == 4 and actions.shape[1:3] != net.shape[1:3]:
            raise ValueError('discriminator: actions tiled to %s but conv2 output is %s (reference defect D3: '
                             'pass [B, A] actions or tile to H/4)' % (actions.shape[1:3], net.shape[1:3]))
        net = _with_actions(net, actions, 'actions')
        net = _stack(net, D_NET['post'], O.conv2d)
        return O.conv2d(net, 1, [2, 2], activation_fn=None, stride=1, scope='conv6')


def build_posterior(frames6, z, reuse=False):
    """The encoder of the latent posterior q(z | x_t, x_{t+1}) (no reference counterpart; the inference network of SV2P / SAVP
    cut down to one transition): ``frames6`` = concat([x_t, x_{t+1}]), 6 channels at pitch 8 as the discriminator's inputs are
    stored -> stats [B, 2 z] = [mu, logvar].

    Four conv 5x5 / 2 + BatchNorm + lrelu layers (Q_NET) and a VALID stride-1 head over the whole remaining map with bias, no
    BatchNorm and no activation - sized as ``g/sconv5`` sizes itself - under scope ``g/posterior``: the variables are the
    generator's to every optimizer, average, clip and schedule that acts on scope ``g``.  The head starts from the default
    initializer and a zero bias; nothing clamps logvar."""
    if len(frames6.shape) != 4 or (frames6.valid_c or frames6.shape[3]) != 6:
        raise ValueError('posterior: [B, H, W, 6] frames (concat([x_t, x_t+1])) expected, got %s' % (frames6.shape,))
    if O.half_mode():
        raise NotImplementedError('the latent posterior is float32 only (the action gradient it is trained through is)')
    with O.variable_scope('g', reuse=reuse), O.variable_scope('posterior'), \
            O.arg_scope([O.conv2d], activation_fn=O.lrelu, stride=2, padding='SAME', normalizer_fn=O.batch_norm, reuse=reuse):
        net = _stack(frames6, Q_NET, O.conv2d)
        sk = net.shape[1]
        if net.shape[2] != sk:
            raise ValueError('posterior: square frames expected, got a %s map' % (net.shape[1:3],))
        stats = O.conv2d(net, 2 * int(z), [sk, sk], activation_fn=None, stride=1, padding='VALID', normalizer_fn=None, scope='head')
        return O.squeeze(stats, axis=(1, 2))       # [B, 1, 1, 2 z] -> [B, 2 z], also at B = 1


# ================================================================================================
# the generator kinds
# ================================================================================================
NUM_MASKS = range(1, 33)


_NO_MASKS = 'it composites no masked candidates a canvas could join: --cdna or --affine'


class Kind(typing.NamedTuple):
    """What the layers above the builders know about one generator.  train.Trainer, the checks of train / evaluate / plan and
    their CLIs read these records and compare no names: a new generator is one more record in KINDS, a new capability of an
    existing one is a changed field."""
    name: str                    # what Trainer.model, metrics.json and plan.json call it, and the string arg_transform that names it
    label: str                   # what messages call it
    build: object                # (images, actions, batch, reuse, ksize, num_masks) -> (frame, state or None); one that takes a
                                 # canvas is also called with the keyword canvas=True
    ksizes: tuple = None         # the ``ksize`` values it takes (None: it does not read ksize) ...
    ksize_text: str = None       # ... and the same in words
    num_masks: bool = False      # whether it reads ``num_masks`` (one of NUM_MASKS)
    float32_only: bool = False
    state_head: bool = True      # whether it predicts the next state beside the frame
    no_rollout: str = None       # why rollout_steps > 1 cannot train it (None: it can)
    no_maps: str = None          # why designated-pixel maps (pixel_maps) cannot follow it (None: they can)
    flag: str = None             # its CLI flag, which is also its keyword of evaluate.evaluate / plan.plan_sequences (None: the default)
    help: str = None
    no_canvas: str = _NO_MASKS   # why it cannot composite a painted canvas (None: it can)

    def check_args(self, ksize, num_masks, canvas=False):
        """ValueError for a ``ksize`` / ``num_masks`` that this generator reads and does not take, and for a ``canvas`` that
        it does not take or that leaves no mask channel for ``num_masks``."""
        if self.ksizes is not None and ksize not in self.ksizes:
            raise ValueError('%s generator: ksize must be %s (got %r)' % (self.label, self.ksize_text, ksize))
        if self.num_masks and num_masks not in NUM_MASKS:
            raise ValueError('%s generator: num_masks must be in 1..32 (got %r)' % (self.label, num_masks))
        if canvas and self.no_canvas:
            raise ValueError('canvas does not go with the %s generator (%s)' % (self.label, self.no_canvas))
        if canvas and num_masks > O.CANVAS_MAX_MASKS:
            raise ValueError('%s generator: num_masks must be in 1..%d with a canvas, which takes one of the 33 mask channels '
                             '(got %r)' % (self.label, O.CANVAS_MAX_MASKS, num_masks))

    def build_with(self, images, actions, batch, reuse, ksize, num_masks, canvas=False):
        """``build``; the canvas is passed only when it is set, so a ``build`` of six arguments stays one."""
        return self.build(images, actions, batch, reuse, ksize, num_masks, **({'canvas': True} if canvas else {}))

    def result_fields(self, ksize, num_masks, canvas=False):
        """The 'num_masks' / 'ksize' entries of metrics.json and plan.json: None for what this generator does not read; and
        'canvas': True when it is on."""
        return dict({'num_masks': num_masks if self.num_masks else None, 'ksize': ksize if self.ksizes is not None else None},
                    **({'canvas': True} if canvas else {}))


_NO_IMAGE_GRADIENT = 'its composite has no image gradient: train the DNA or the plain generator'
KINDS = {kind.name: kind for kind in (
    Kind('plain', 'plain', lambda images, actions, batch, reuse, ksize, num_masks: (build_generator(images, actions, reuse=reuse), None),
         state_head=False, no_maps='the plain generator predicts no flow a map could follow (DNA generator only)'),
    Kind('dna', 'DNA', lambda images, actions, batch, reuse, ksize, num_masks:
         build_generator_transform(images, actions, batch_size=batch, ksize=ksize, reuse=reuse),
         ksizes=tuple(range(1, 12)), ksize_text='in 1..11', flag='dna'),
    Kind('cdna', 'CDNA', lambda images, actions, batch, reuse, ksize, num_masks, canvas=False:
         build_generator_cdna(images, actions, batch_size=batch, num_masks=num_masks, ksize=ksize, reuse=reuse, canvas=canvas),
         ksizes=(3, 5, 7), ksize_text='3, 5 or 7', num_masks=True, float32_only=True, no_rollout=_NO_IMAGE_GRADIENT,
         no_maps='the CDNA generator is declined - its channel split, kept as written from the reference, transforms the colour '
                 'channels of one mask with different kernels, so there is no single flow that a map could follow consistently '
                 'with the frame (DNA generator only)',
         flag='cdna', help='the CDNA generator (models.build_generator_cdna): float32, --ksize 3, 5 or 7', no_canvas=None),
    Kind('affine', 'affine', lambda images, actions, batch, reuse, ksize, num_masks, canvas=False:
         build_generator_affine(images, actions, batch_size=batch, num_masks=num_masks, reuse=reuse, canvas=canvas),
         num_masks=True, float32_only=True, no_rollout=_NO_IMAGE_GRADIENT,
         no_maps='the affine generator is declined - there is no map advection through its warps (DNA generator only)',
         flag='affine', help='the affine (STP) generator (models.build_generator_affine): float32, --ksize is not read',
         no_canvas=None),
)}
BOOLEAN = {False: 'plain', True: 'dna'}        # the reference's arg_transform is its boolean --dna: these two kinds keep it


def model_kind(arg_transform):
    """The name in KINDS of the generator an ``arg_transform`` names: that name itself, or the reference's boolean ``--dna``
    (False: 'plain', True: 'dna')."""
    if isinstance(arg_transform, str):
        if arg_transform in KINDS:
            return arg_transform
        raise ValueError('unexpected transform argument %r (False, True or one of %s)' % (arg_transform, ', '.join(map(repr, KINDS))))
    return BOOLEAN[bool(arg_transform)]


def flags():
    """The CLI flags that name a generator (the keywords of evaluate.evaluate / plan.plan_sequences that do)."""
    return [kind.flag for kind in KINDS.values() if kind.flag]


def transform_argument(given, fmt='%s'):
    """The Trainer's arg_transform for the generator flags ``given`` {flag: value, ...; other keys are ignored}: the name of the
    generator whose flag is set, the boolean for the reference's ``--dna``, False without one.  Two set flags are a ValueError
    that names them through ``fmt`` ('--%s' for a CLI)."""
    named = [kind for kind in KINDS.values() if kind.flag and given.get(kind.flag)]
    if len(named) > 1:
        raise ValueError('%s and %s name two different generators' % (fmt % named[0].flag, fmt % named[1].flag))
    name = named[0].name if named else BOOLEAN[False]
    return next((b for b, n in BOOLEAN.items() if n == name), name)
