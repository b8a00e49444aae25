"""float64 restatement of the affine (STP) generator (models.build_generator_affine) and of its warp-and-composite
(include/acgan_cdna.h), from the explicit formula, in torch with autograd; the shared cases of the affine tests and the kink
rule.  Test infrastructure."""
import numpy as np
import torch

from oracle import models as OM
from oracle.trainer import OracleTrainer

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
PARAM_SCALE = (.15, .15, .25, .15, .15, .25)
KINK = 2.5e-4                 # dout is zeroed where a source coordinate is this close to an integer
KINK_SHARE = 0.06             # at most this share of a case's pixels may be zeroed


def coords(params, h, w):
    """params [B, M*6] -> (px, py) [B, M, H, W], the source coordinates in pixels of every output pixel."""
    b = params.shape[0]
    t = params.reshape(b, -1, 6) + torch.tensor(IDENTITY, dtype=params.dtype)
    u = (2 * torch.arange(w, dtype=params.dtype) / (w - 1) - 1).view(1, 1, 1, w)
    v = (2 * torch.arange(h, dtype=params.dtype) / (h - 1) - 1).view(1, 1, h, 1)
    c = lambda i: t[:, :, i].view(b, -1, 1, 1)     # noqa: E731
    xs, ys = c(0) * u + c(1) * v + c(2), c(3) * u + c(4) * v + c(5)
    return (xs + 1) * (w - 1) / 2, (ys + 1) * (h - 1) / 2


def warp(image, params):
    """T [B, M, H, W, C]: the 4 bilinear taps of every (pixel, mask), a tap outside the image contributing 0.  Differentiable
    with respect to params (the derivative in the cell floor selects)."""
    b, h, w, ch = image.shape
    px, py = coords(params, h, w)
    x0, y0 = torch.floor(px).detach(), torch.floor(py).detach()
    fx, fy = px - x0, py - y0
    bi = torch.arange(b).view(b, 1, 1, 1)
    out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
            val = image[bi, yi.clamp(0, h - 1), xi.clamp(0, w - 1)] * ok.unsqueeze(-1).to(image.dtype)
            wgt = (fx if dx else 1 - fx) * (fy if dy else 1 - fy)
            out = out + wgt.unsqueeze(-1) * val
    return out


def composite(logits, image, params, num_masks):
    """s = softmax(logits) over the M+1 channels; s_0 * image + sum_m s_{m+1} * T_m."""
    t = warp(image, params)
    assert t.shape[1] == num_masks
    s = torch.softmax(logits, dim=-1)
    out = s[..., :1] * image
    for m in range(num_masks):
        out = out + s[..., m + 1:m + 2] * t[:, m]
    return out


def case(shape, seed=0, spread=1):
    """(params [B, M*6], z, image, dout) of a (b, h, w, c, m) case, float32 on the CPU.  spread 1: near the identity; 8: wide -
    large scales and shears, many taps (and some whole masks) fall outside the image."""
    b, h, w, c, m = shape
    g = torch.Generator().manual_seed(seed)
    params = torch.randn(b, m, 6, generator=g) * torch.tensor(PARAM_SCALE) * spread
    image = torch.rand(b, h, w, c, generator=g) * 2 - 1
    g2 = torch.Generator().manual_seed(seed + 1000)
    z = 2 * torch.randn(b, h, w, m + 1, generator=g2)
    dout = torch.randn(b, h, w, c, generator=g2)
    return params.reshape(b, m * 6).contiguous(), z, image, dout


def apply_kink_rule(params, dout):
    """dout with zeros at every output pixel where any mask's px or py (float64) lies within KINK of an integer, and the share
    of pixels that were zeroed.  The derivative of a bilinear sample jumps there, and a float32 coordinate may land on the
    other side."""
    b, h, w, _ = dout.shape
    px, py = coords(params.double(), h, w)
    near = ((px - px.round()).abs() < KINK) | ((py - py.round()).abs() < KINK)
    hit = near.any(dim=1)                                     # [B, H, W]
    return dout * (~hit).unsqueeze(-1).to(dout.dtype), float(hit.double().mean())


# ---- the generator and its trainer ----------------------------------------------------------------------------------------
def generator_affine(params, images, actions, M=10, create=None):
    """build_generator_affine: the DNA generator's trunk, the affine_params linear layer (a VALID S/16 x S/16 conv) on the
    action-conditioned bottleneck, tconv4 to M+1 mask logits, the composite.  -> (frame [B,H,W,3], state [B,5])."""
    L = OM.generator_transform_layers(5, images.shape[1] // 16)
    out = images
    for spec in L['enc']:
        out = OM._layer(params, 'g', spec, out, create)
    h0 = torch.cat([out, OM.tile_actions(actions, out.shape[1]).to(out.dtype)], dim=3)
    tp = OM._layer(params, 'g', ('affine_params', 'c', 6 * M, h0.shape[1], 1, 'VALID', False, None), h0, create)
    tp = tp.reshape(tp.shape[0], 6 * M)
    out = h0
    for spec in L['dec1']:
        out = OM._layer(params, 'g', spec, out, create)
    st = out
    for spec in L['state']:
        st = OM._layer(params, 'g', spec, st, create)
    out = OM._layer(params, 'g', L['dec2'][0], out, create)
    z = OM._layer(params, 'g', ('tconv4', 't', M + 1, 5, 2, 'SAME', False, None), out, create)
    return composite(z, images, tp, M), st.reshape(st.shape[0], -1)


def init_params_affine(batch=2, img=64, num_masks=10, seed=0, dtype=torch.float32, act_dim=10):
    """All g/ and d/ variables of an affine trainer (slim xavier-uniform weights, zero beta / biases)."""
    gen = torch.Generator().manual_seed(seed)
    params = {}
    x = torch.zeros(batch, img, img, 3, dtype=dtype)
    a = torch.zeros(batch, act_dim, dtype=dtype)
    with torch.no_grad():
        frame, _ = generator_affine(params, x, a, num_masks, create=(gen, dtype))
        OM.discriminator(params, torch.cat([x, frame], dim=3), a, create=(gen, dtype))
    return params


class AffineOracleTrainer(OracleTrainer):
    """OracleTrainer with the affine generator: the DNA generator's losses (state head included); every step and
    test_sequence go through _g."""

    def __init__(self, params, arg_adv, arg_loss, arg_opt, num_masks=10):
        super().__init__(params, arg_adv, arg_loss, arg_opt, True, 5)
        self.num_masks = num_masks

    def _g(self, p, img, actions):
        return generator_affine(p, img, actions, self.num_masks)


def smooth_frames(batch, size=64, seed=0):
    """(x, y, actions, state): frames that are a sum of a few 2-D sinusoids with no period under 32 px, plus the shifted next
    frame - not noise, so that a float32 coordinate on the other side of a kink changes no gradient by much."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing='ij')
    x = np.zeros((batch, size, size, 3))
    for b in range(batch):
        for c in range(3):
            for _ in range(4):
                fy, fx = rng.uniform(-1, 1, 2) / 32.0          # cycles per pixel: period >= 32 px
                x[b, :, :, c] += rng.uniform(0.1, 0.25) * np.sin(2 * np.pi * (fy * yy + fx * xx) + rng.uniform(0, 2 * np.pi))
    x = x.astype(np.float32)
    y = np.roll(x, 2, axis=2)
    return x, y, rng.standard_normal((batch, 10)).astype(np.float32), rng.standard_normal((batch, 5)).astype(np.float32)
