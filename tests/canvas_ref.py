"""float64 restatement of the painted canvas of the CDNA and affine generators (models._mask_generator canvas=True;
include/acgan_cdna.h acg_*_composite_canvas_*): cdna_ref / affine_ref with the extra softmax channel, the canvas term and the
tconv4_canvas layer, and the oracle trainers of the two generators with it.  Test infrastructure."""
import torch

import affine_ref
import cdna_ref
from oracle import models as OM
from oracle import tf_ops as T


def blend(logits, image, pieces, canvas):
    """s = softmax(logits) over the M+2 channels; s_0 * image + sum_j s_{j+1} * pieces[j] + s_{M+1} * canvas."""
    assert logits.shape[-1] == len(pieces) + 2
    s = torch.softmax(logits, dim=-1)
    out = s[..., :1] * image
    for j, t in enumerate(pieces):
        out = out + s[..., j + 1:j + 2] * t
    return out + s[..., -1:] * canvas


def cdna_composite(logits, image, params, canvas, num_masks, ksize):
    """cdna_ref.composite with the canvas as the last candidate (logits [B,H,W,M+2])."""
    return blend(logits, image, T.cdna_transform(params, image, num_masks, ksize, cdna_ref.RELU_SHIFT), canvas)


def affine_composite(logits, image, params, canvas, num_masks):
    """affine_ref.composite with the canvas as the last candidate (logits [B,H,W,M+2])."""
    t = affine_ref.warp(image, params)
    assert t.shape[1] == num_masks
    return blend(logits, image, [t[:, m] for m in range(num_masks)], canvas)


def _generator(params, images, actions, scope, width, k, M, composite, create):
    """models._mask_generator with canvas=True: the trunk of cdna_ref.generator_cdna / affine_ref.generator_affine, tconv4 to
    M+2 mask logits, tconv4_canvas (5x5/2 deconvolution + bias + tanh of the tconv3 output) and ``composite``."""
    L = OM.generator_transform_layers(k, images.shape[1] // 16)
    out = images
    for spec in L['enc']:
        out = OM._layer(params, 'g', spec, out, create)
    h0 = torch.cat([out, OM.tile_actions(actions, out.shape[1]).to(out.dtype)], dim=3)
    mp = OM._layer(params, 'g', (scope, 'c', width, h0.shape[1], 1, 'VALID', False, None), h0, create)
    mp = mp.reshape(mp.shape[0], width)
    out = h0
    for spec in L['dec1']:
        out = OM._layer(params, 'g', spec, out, create)
    st = out
    for spec in L['state']:
        st = OM._layer(params, 'g', spec, st, create)
    out = OM._layer(params, 'g', L['dec2'][0], out, create)
    z = OM._layer(params, 'g', ('tconv4', 't', M + 2, 5, 2, 'SAME', False, None), out, create)
    canvas = OM._layer(params, 'g', ('tconv4_canvas', 't', images.shape[3], 5, 2, 'SAME', False, 'tanh'), out, create)
    return composite(z, mp, canvas), st.reshape(st.shape[0], -1)


def generator_cdna(params, images, actions, M=10, k=5, create=None):
    """build_generator_cdna(canvas=True) -> (frame [B,H,W,3], state [B,5])."""
    return _generator(params, images, actions, 'cdna_params', k * k * M, k, M,
                      lambda z, mp, canvas: cdna_composite(z, images, mp, canvas, M, k), create)


def generator_affine(params, images, actions, M=10, create=None):
    """build_generator_affine(canvas=True) -> (frame [B,H,W,3], state [B,5])."""
    return _generator(params, images, actions, 'affine_params', 6 * M, 5, M,
                      lambda z, mp, canvas: affine_composite(z, images, mp, canvas, M), create)


def init_params(kind, batch=2, img=64, ksize=5, num_masks=10, seed=0, dtype=torch.float32, act_dim=10):
    """All g/ and d/ variables of a ``kind`` ('cdna' or 'affine') trainer with a canvas (slim xavier-uniform weights, zero beta /
    biases)."""
    gen = torch.Generator().manual_seed(seed)
    params = {}
    x = torch.zeros(batch, img, img, 3, dtype=dtype)
    a = torch.zeros(batch, act_dim, dtype=dtype)
    with torch.no_grad():
        if kind == 'cdna':
            frame, _ = generator_cdna(params, x, a, num_masks, ksize, create=(gen, dtype))
        else:
            frame, _ = generator_affine(params, x, a, num_masks, create=(gen, dtype))
        OM.discriminator(params, torch.cat([x, frame], dim=3), a, create=(gen, dtype))
    return params


class CdnaCanvasOracleTrainer(cdna_ref.CdnaOracleTrainer):
    """CdnaOracleTrainer with the canvas: only the generator differs."""

    def _g(self, p, img, actions):
        return generator_cdna(p, img, actions, self.num_masks, self.ksize)


class AffineCanvasOracleTrainer(affine_ref.AffineOracleTrainer):
    """AffineOracleTrainer with the canvas: only the generator differs."""

    def _g(self, p, img, actions):
        return generator_affine(p, img, actions, self.num_masks)


ORACLE_TRAINERS = {'cdna': CdnaCanvasOracleTrainer, 'affine': AffineCanvasOracleTrainer}


# ---- the gradients as the kernels state them (include/acgan_cdna.h), for the check against autograd --------------------------
def blend_grads(logits, image, pieces, canvas, dout):
    """g_0 = <dout, image>, g_{j+1} = <dout, T_j>, g_{M+1} = <dout, canvas>; dz_j = s_j (g_j - sum_l s_l g_l); dT_j = s_{j+1} dout;
    dcanvas = s_{M+1} dout.  -> (dz, [dT_j], dcanvas)."""
    s = torch.softmax(logits, dim=-1)
    g = torch.stack([(dout * c).sum(dim=-1) for c in [image] + list(pieces) + [canvas]], dim=-1)
    dz = s * (g - (s * g).sum(dim=-1, keepdim=True))
    return dz, [s[..., j + 1:j + 2] * dout for j in range(len(pieces))], s[..., -1:] * dout


def composite_grads(kind, z, bias, image, params, canvas, dout, num_masks, ksize=None):
    """(dz, dparams, dbias, dcanvas) of the ``kind`` composite by blend_grads; dparams is the pieces' own vector-Jacobian product
    with dT_j (cdna: through the normalisation and the relu; affine: the six sums per mask)."""
    params = params.detach().clone().requires_grad_(True)
    if kind == 'cdna':
        pieces = list(T.cdna_transform(params, image, num_masks, ksize, cdna_ref.RELU_SHIFT))
    else:
        t = affine_ref.warp(image, params)
        pieces = [t[:, m] for m in range(num_masks)]
    dz, dpieces, dcanvas = blend_grads(z + bias, image, [p.detach() for p in pieces], canvas, dout)
    dparams, = torch.autograd.grad(pieces, params, dpieces)
    return dz, dparams, dz.sum(dim=(0, 1, 2)), dcanvas


# ---- the shared cases of the canvas tests ------------------------------------------------------------------------------------
def _canvas_rows(z, num_masks):
    """+30 and -30 on the canvas's mask channel, in a row each (rows 1 and 2)."""
    z[:, 1, :, num_masks + 1], z[:, 2, :, num_masks + 1] = 30.0, -30.0
    return z


def cdna_case(shape, seed=0):
    """(params, z [.., M+2], bias [M+2], image, canvas, dout) of a (b, h, w, c, m, k) case, float32 on the CPU: as
    test_gpu_cdna._case builds them - whole masks clamped (every tap <= shift), logits of +-30 in places - with a canvas in
    [-1, 1] and +-30 on its channel in a row each."""
    b, h, w, c, m, k = shape
    g = torch.Generator().manual_seed(seed)
    params = torch.randn(b, k * k * m, generator=g) * 0.7 + 0.3
    params.view(b, k * k, m)[:, :, 0] = -0.5
    z = torch.randn(b, h, w, m + 2, generator=g) * 2
    z[:, 0, :, 0], z[:, -1, :, m] = 30.0, -30.0
    bias = torch.randn(m + 2, generator=g)
    img = torch.rand(b, h, w, c, generator=g) * 2 - 1
    dout = torch.randn(b, h, w, c, generator=g)
    canvas = torch.rand(b, h, w, c, generator=g) * 2 - 1
    return params.float(), _canvas_rows(z, m).float(), bias.float(), img.float(), canvas.float(), dout.float()


def affine_case(shape, seed=0, spread=1):
    """(params, z [.., M+2], bias [M+2], image, canvas, dout) of a (b, h, w, c, m) case: affine_ref.case as test_gpu_affine._case
    dresses it (a bias, logits of +-30 in a row each), with a canvas in [-1, 1] and +-30 on its channel in a row each."""
    b, h, w, c, m = shape
    params, z, img, dout = affine_ref.case(shape, seed, spread)
    g = torch.Generator().manual_seed(seed + 3000)
    z = torch.cat([z, 2 * torch.randn(b, h, w, 1, generator=g)], dim=-1)
    z[:, 0, :, 0], z[:, -1, :, m] = 30.0, -30.0
    bias = torch.randn(m + 2, generator=torch.Generator().manual_seed(seed + 2000))
    canvas = torch.rand(b, h, w, c, generator=g) * 2 - 1
    return params, _canvas_rows(z, m), bias, img, canvas, dout
