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
from . import graph as G
from . import ops as O

G_PLAIN = {'encoder': (('conv1', 64), ('conv2', 128), ('conv3', 256), ('conv4', 512)),
           'decoder': (('tconv1', 256), ('tconv2', 128), ('tconv3', 64))}
G_DNA = {'encoder': (('conv1', 32), ('conv2', 64), ('conv3', 128), ('conv4', 256)),
         'decoder_a': (('tconv1', 128), ('tconv2', 128)),
         'state': (('sconv3', 32), ('sconv4', 16)),
         'decoder_b': (('tconv3', 128),)}
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


def build_generator_transform(images, actions, batch_size=None, reuse=False, color_channels=3, ksize=5):
    """DNA generator (models.py:24-74): predicts k*k per-pixel kernel logits and a 5-d next state.

    Returns ``(frame, state)``; ``batch_size`` is accepted for signature compatibility (the static
    shape already carries it).
    """
    if batch_size is not None and batch_size != images.shape[0]:
        raise ValueError('batch_size %r does not match images %s' % (batch_size, images.shape))
    if images.shape[3] != color_channels:
        raise ValueError('color_channels %r does not match images %s' % (color_channels, images.shape))
    with O.variable_scope('g', reuse=reuse), \
            O.arg_scope([O.conv2d, O.deconv2d], activation_fn=O.relu, stride=2, padding='SAME',
                        normalizer_fn=O.batch_norm, reuse=reuse):
        net = _stack(getattr(images, 'padded', images), G_DNA['encoder'], O.conv2d)
        net = _with_actions(net, actions, 'actions')
        net = _stack(net, G_DNA['decoder_a'], O.deconv2d)

        # the state head reads the decoder's 16x16 features and nothing of what the frame decoder does next: a side chain
        # (five tiny latency-bound layers that hide behind tconv3 / tconv4 / the DNA gather, forward and backward)
        with G.get_default_graph().side_branch():
            state = _stack(net, G_DNA['state'], O.conv2d, size=3)
            sk = state.shape[1]           # 4 at 64x64: the reference's 4x4 VALID head (models.py:44-51)
            state = O.conv2d(state, 5, [sk, sk], activation_fn=None, stride=1, padding='VALID', normalizer_fn=None,
                             scope='sconv5')
            state = O.squeeze(state, axis=(1, 2))       # [B, 1, 1, 5] -> [B, 5], also at B = 1

        net = _stack(net, G_DNA['decoder_b'], O.deconv2d)
        logits = O.deconv2d(net, ksize * ksize, [5, 5], activation_fn=None, normalizer_fn=None, scope='tconv4')
        frame = O.dna_gather(logits, images, ksize)
        return frame, state


def build_generator_cdna(images, actions, batch_size=None, reuse=False, color_channels=3, num_masks=10, ksize=5):
    """CDNA generator: the DNA generator's trunk with the reference's ``cdna_transformation`` (ops.py:52-98, which none of
    its models calls) as the motion model.  Returns ``(frame, state)``.

    ``cdna_params``, a linear layer (bias, no BatchNorm or activation) on the action-conditioned bottleneck h0
    [B, S/16, S/16, 266] - stored as a VALID S/16 x S/16 conv, ``g/cdna_params/weights`` [S/16, S/16, 266, k*k*M], the same
    numbers as slim's [S/16 * S/16 * 266, k*k*M] in reshape order - predicts M = ``num_masks`` k x k kernels per sample.
    tconv1, tconv2, the state head and tconv3 are the DNA generator's; ``tconv4`` (5x5/2, bias only) gives M+1 mask logits.
    The frame is s_0 * images + sum_j s_{j+1} * T_j with s = softmax over the M+1 channels and T_j the pieces of
    cdna_transformation (its channel split kept as written), in one fused kernel (ops.cdna_composite).

    Two differences from the CDNA model of the paper the push dataset comes from: there is no image generated from
    scratch among the composited candidates, and the masks come from the 5x5/2 ``tconv4`` instead of a 1x1 layer.
    float32 only; ``ksize`` 3, 5 or 7, 1 <= ``num_masks`` <= 32, image size a multiple of 16."""
    if batch_size is not None and batch_size != images.shape[0]:
        raise ValueError('batch_size %r does not match images %s' % (batch_size, images.shape))
    if images.shape[3] != color_channels:
        raise ValueError('color_channels %r does not match images %s' % (color_channels, images.shape))
    if ksize not in (3, 5, 7) or not 1 <= num_masks <= 32:
        raise ValueError('CDNA generator: ksize must be 3, 5 or 7 and num_masks 1..32 (got %r, %r)' % (ksize, num_masks))
    if images.shape[1] % 16 or images.shape[2] % 16:
        raise ValueError('CDNA generator: image size %s is not a multiple of 16' % (images.shape[1:3],))
    if O.half_mode():
        raise NotImplementedError('the CDNA generator is float32 only')
    return _mask_generator(images, actions, reuse, 'cdna_params', ksize * ksize * num_masks, num_masks,
                           lambda logits, params: O.cdna_composite(logits, images, params, num_masks, ksize))


def _mask_generator(images, actions, reuse, scope, width, num_masks, composite):
    """The trunk the CDNA and the affine generators share: the DNA generator's layers, a linear layer ``scope`` of ``width``
    outputs per sample on the action-conditioned bottleneck, tconv4 to M+1 mask logits and ``composite(logits, params)``."""
    with O.variable_scope('g', reuse=reuse), \
            O.arg_scope([O.conv2d, O.deconv2d], activation_fn=O.relu, stride=2, padding='SAME',
                        normalizer_fn=O.batch_norm, reuse=reuse):
        net = _stack(getattr(images, 'padded', images), G_DNA['encoder'], O.conv2d)
        net = _with_actions(net, actions, 'actions')
        params = O.conv2d(net, width, [net.shape[1], net.shape[2]], activation_fn=None, stride=1, padding='VALID',
                          normalizer_fn=None, scope=scope)
        params = params.reshape((images.shape[0], width))
        net = _stack(net, G_DNA['decoder_a'], O.deconv2d)
        with G.get_default_graph().side_branch():
            state = _stack(net, G_DNA['state'], O.conv2d, size=3)
            sk = state.shape[1]
            state = O.conv2d(state, 5, [sk, sk], activation_fn=None, stride=1, padding='VALID', normalizer_fn=None,
                             scope='sconv5')
            state = O.squeeze(state, axis=(1, 2))       # [B, 1, 1, 5] -> [B, 5], also at B = 1
        net = _stack(net, G_DNA['decoder_b'], O.deconv2d)
        logits = O.deconv2d(net, num_masks + 1, [5, 5], activation_fn=None, normalizer_fn=None, scope='tconv4')
        return composite(logits, params), state


def build_generator_affine(images, actions, batch_size=None, reuse=False, color_channels=3, num_masks=10):
    """Affine (STP) generator: ``build_generator_cdna`` with a 2x3 affine transform per mask in place of a k x k kernel.
    Returns ``(frame, state)``.

    ``g/affine_params`` (weights [S/16, S/16, 266, 6*M], biases, default initialisers) stands where ``g/cdna_params`` does and
    predicts M = ``num_masks`` transforms per sample, read as theta = params + (1, 0, 0, 0, 1, 0): zero parameters are the
    identity.  The frame is s_0 * images + sum_m s_{m+1} * T_m with T_m the image warped by theta_m, bilinear with zeros
    outside (include/acgan_cdna.h has the formula), in one fused kernel (ops.affine_composite).  Rotation, scale and shear of
    an object take 6 numbers here; the k x k kernels of DNA / CDNA cannot move anything further than (k-1)/2 pixels.
    As for CDNA there is no image generated from scratch among the candidates and the masks come from the 5x5/2 ``tconv4``.
    float32 only; 1 <= ``num_masks`` <= 32, image size a multiple of 16."""
    if batch_size is not None and batch_size != images.shape[0]:
        raise ValueError('batch_size %r does not match images %s' % (batch_size, images.shape))
    if images.shape[3] != color_channels:
        raise ValueError('color_channels %r does not match images %s' % (color_channels, images.shape))
    if not 1 <= num_masks <= 32:
        raise ValueError('affine generator: num_masks must be in 1..32 (got %r)' % (num_masks,))
    if images.shape[1] % 16 or images.shape[2] % 16:
        raise ValueError('affine generator: image size %s is not a multiple of 16' % (images.shape[1:3],))
    if O.half_mode():
        raise NotImplementedError('the affine generator is float32 only')
    return _mask_generator(images, actions, reuse, 'affine_params', 6 * num_masks, num_masks,
                           lambda logits, params: O.affine_composite(logits, images, params, num_masks))


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
