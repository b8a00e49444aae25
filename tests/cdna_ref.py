"""float64 restatement of the CDNA generator (models.build_generator_cdna) from read-only oracle pieces: oracle.models._layer
and tile_actions, oracle.tf_ops.cdna_transform, plus the softmax and the composite.  Test infrastructure."""
import torch

from oracle import models as OM
from oracle import tf_ops as T
from oracle.trainer import OracleTrainer

RELU_SHIFT = 1e-12


def composite(logits, image, params, num_masks, ksize):
    """s = softmax(logits) over the M+1 channels; s_0 * image + sum_j s_{j+1} * T_j (T_j: cdna_transform's pieces)."""
    pieces = T.cdna_transform(params, image, num_masks, ksize, RELU_SHIFT)
    s = torch.softmax(logits, dim=-1)
    out = s[..., :1] * image
    for j, t in enumerate(pieces):
        out = out + s[..., j + 1:j + 2] * t
    return out


def generator_cdna(params, images, actions, M=10, k=5, create=None):
    """build_generator_cdna: the DNA generator's trunk, the cdna_params linear layer (a VALID S/16 x S/16 conv) on the
    action-conditioned bottleneck, tconv4 to M+1 mask logits, the composite.  -> (frame [B,H,W,3], state [B,5])."""
    L = OM.generator_transform_layers(k, images.shape[1] // 16)
    out = images
    for spec in L['enc']:
        out = OM._layer(params, 'g', spec, out, create)
    h0 = torch.cat([out, OM.tile_actions(actions, out.shape[1]).to(out.dtype)], dim=3)
    kp = OM._layer(params, 'g', ('cdna_params', 'c', k * k * M, h0.shape[1], 1, 'VALID', False, None), h0, create)
    kp = kp.reshape(kp.shape[0], k * k * M)
    out = h0
    for spec in L['dec1']:
        out = OM._layer(params, 'g', spec, out, create)
    st = out
    for spec in L['state']:
        st = OM._layer(params, 'g', spec, st, create)
    out = OM._layer(params, 'g', L['dec2'][0], out, create)
    z = OM._layer(params, 'g', ('tconv4', 't', M + 1, 5, 2, 'SAME', False, None), out, create)
    return composite(z, images, kp, M, k), st.reshape(st.shape[0], -1)


def init_params_cdna(batch=2, img=64, ksize=5, num_masks=10, seed=0, dtype=torch.float32, act_dim=10):
    """All g/ and d/ variables of a CDNA trainer (slim xavier-uniform weights, zero beta / biases)."""
    gen = torch.Generator().manual_seed(seed)
    params = {}
    x = torch.zeros(batch, img, img, 3, dtype=dtype)
    a = torch.zeros(batch, act_dim, dtype=dtype)
    with torch.no_grad():
        frame, _ = generator_cdna(params, x, a, num_masks, ksize, create=(gen, dtype))
        OM.discriminator(params, torch.cat([x, frame], dim=3), a, create=(gen, dtype))
    return params


class CdnaOracleTrainer(OracleTrainer):
    """OracleTrainer with the CDNA generator: the DNA generator's losses (state head included); every step and
    test_sequence go through _g."""

    def __init__(self, params, arg_adv, arg_loss, arg_opt, num_masks=10, ksize=5):
        super().__init__(params, arg_adv, arg_loss, arg_opt, True, ksize)
        self.num_masks = num_masks

    def _g(self, p, img, actions):
        return generator_cdna(p, img, actions, self.num_masks, self.ksize)
