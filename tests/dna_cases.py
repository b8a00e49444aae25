"""The DNA tail at every kernel size, storage type, channel count and staging path of dna.hip (dna_kernel, dna_rows_kernel) and
rollout.hip (dna_dimage_kernel), against float64.  Shared by the GPU suite (tests/test_gpu_dna_paths.py) and - the float32 rows -
the CPU suite on the C oracle (tests/test_dna_paths_cpu.py), which proves the references, the NaN / guard bookkeeping and the
bars before anything goes to a GPU.  The oracle takes float32 logits and a float32 second home only: bf16 rows are GPU-only.

``dna_paths`` restates the host side of dna.hip - which kernel family, channel body and logits staging a launch takes - so every
row of ``PATH_CASES`` names the paths it is there for and the case fails, by name, when a retune moves the shape off them.

Bars (tests/test_gpu_ops.py, tests/op_cases.py case_dna_bias / case_dna_bf16): float32 logits - the frame to TOL = 2e-5, dlogits
to 4 TOL, dbias to 8 TOL; bf16 logits - the frame (float32, from the bf16-rounded logits) to TOL, dlogits and dbias to 6e-3.
No row of the tables needed another bar; the backward of a softmax saturated by +40 is the one check float64 cannot referee by
max |reference| - case_dna_one_hot says why and what holds it instead.  On an MI355X the float32 kernels sit within 3 % of these
bars, the bf16 dlogits within 60 % (their storage rounding, up to 2^-8 of the tensor's scale).

``launched()`` lists the (ksize, storage, C, family, staging) combinations launched before these tables and by them."""
import ctypes
import math

import torch

from action_conditioned_gans_amd import _lib as L
from op_cases import SENTINEL, T, close, r16, randn, uniform

TOL = 2e-5
TOL16 = 6e-3
GUARD = 64                    # sentinel elements in front of and behind every output the kernels write

TX, TY, ROWS_MIN = 64, 4, 6            # dna.hip: TX, ACG_DNA_TY, ACG_DNA_ROWS_MIN


def round8(n):
    return (n + 7) // 8 * 8


# ----------------------------------------------------------------------------------------------- the restated dispatch
def dna_grid(k, b, h, w):
    """dna.hip dna_grid (lines 453-456): the launch grid, whose block count is also the number of dbias partial rows."""
    if k >= ROWS_MIN:
        return (-(-w // 64), h, b)
    return (-(-w // TX), -(-h // TY), b)


def dna_paths(b, h, w, c, k, half):
    """The paths a launch of acg_dna_fwd / acg_dna_bwd takes, restated from dna.hip in plain Python:
      launch_k (lines 458-471)   'rows' (k >= ACG_DNA_ROWS_MIN = 6, lines 445-447) or 'tile' (64 x ACG_DNA_TY = 4 pixels, lines
                                 450-452); 'cc3' (the compile-time C = 3 body) or 'crt' (runtime C)
      dna_kernel (lines 80, 94-96)   float32 tile blocks stage their logits as float4 ('vec') or element by element ('scalar'):
                                 vec = (S == KK) && pix0 * KK % 4 == 0 && W * KK % 4 == 0 && txv * KK % 4 == 0 && the pointer is
                                 16-byte aligned - which include/acgan_hip.h:12 demands of every tensor - with S = KK | 1,
                                 pix0 = (b H + y0) W + x0, txv = min(64, W - x0), evaluated per block over the whole grid
      'ragged_x' (W % 64 != 0: the last block of a row is partial, in both families), 'ragged_y' (tile: H % 4 != 0),
      'multi_block_x' (W > 64), 'smaller_than_halo' (H < k and W < k: every window leaves the frame on both axes)
      'partials=N'               dna_grid (lines 453-456): N blocks = N dbias partial rows; 'dbias_two_stage' from N > 1024 on
                                 (acg_dna_bwd, lines 539-547), else 'dbias_one_stage'."""
    assert 1 <= k <= 11 and 1 <= c <= 4
    kk, paths = k * k, set()
    rows = k >= ROWS_MIN
    paths.add('rows' if rows else 'tile')
    paths.add('cc3' if c == 3 else 'crt')
    gx, gy, gz = dna_grid(k, b, h, w)
    if not rows and not half:
        s = kk | 1
        for bz in range(gz):
            for by in range(gy):
                for bx in range(gx):
                    x0, y0 = bx * TX, by * TY
                    txv = min(TX, w - x0)
                    pix0 = (bz * h + y0) * w + x0
                    vec = s == kk and (pix0 * kk) % 4 == 0 and (w * kk) % 4 == 0 and (txv * kk) % 4 == 0
                    paths.add('vec' if vec else 'scalar')
    if w % 64:
        paths.add('ragged_x')
    if not rows and h % TY:
        paths.add('ragged_y')
    if w > 64:
        paths.add('multi_block_x')
    if h < k and w < k:
        paths.add('smaller_than_halo')
    n = gx * gy * gz
    paths.add('partials=%d' % n)
    paths.add('dbias_two_stage' if n > 1024 else 'dbias_one_stage')
    return paths


def staging(b, h, w, c, k, half):
    """How the logits of a launch reach the arithmetic, for the coverage lists: the tile kernel through LDS ('vec' / 'scalar' /
    both, or 'bf16' 8-byte pieces), the rows kernel straight into registers."""
    p = dna_paths(b, h, w, c, k, half)
    if 'rows' in p:
        return 'regs'
    return 'bf16' if half else '+'.join(sorted(p & {'vec', 'scalar'}))


def combo(b, h, w, c, k, half):
    """(ksize, storage, C, family, staging) of a launch."""
    return (k, 'bf16' if half else 'f32', c, 'rows' if k >= ROWS_MIN else 'tile', staging(b, h, w, c, k, half))


# ----------------------------------------------------------------------------------------------- the table
RUNTIME_C = (1, 2, 4)


def _path_cases():
    """(name, (b, h, w, c, k), half, {paths the row is there for}).  Per k: C = 3 and one runtime C in each storage type, the
    runtime C cycling through 1, 2, 4 so that each meets both families.
      tile (k < 6)   W = 68: two blocks per row, the second 4 pixels wide; H = 6: the second tile row holds 2 of 4 rows; W % 4 == 0
                     is what lets an odd k stage float4 (KK odd), and no even k can (S = KK | 1 != KK).  W = 7, H = 5: W % 4 != 0
                     puts every block on the scalar staging.
      rows (k >= 6)  W = 131 = 2 x 64 + 3 and W = 65 = 64 + 1: the last block holds 3 pixels / one pixel (15 of its 16 pixel groups
                     idle, all four `it` steps past the row's end for most).
      small          an image below the kernel size on both axes: (1, 2, 3) from k = 4 on, (1, 2, 2) at k = 3, (1, 1, 1) at k = 2."""
    rows = []
    for k in range(1, 12):
        ca, cb = RUNTIME_C[k % 3], RUNTIME_C[(k + 1) % 3]
        if k < ROWS_MIN:
            stage = 'vec' if k % 2 else 'scalar'
            rows += [('t%d_f32_c3_w68' % k, (2, 6, 68, 3, k), False, {'tile', 'cc3', stage, 'ragged_x', 'ragged_y', 'multi_block_x'}),
                     ('t%d_f32_c%d_w7' % (k, ca), (1, 5, 7, ca, k), False, {'tile', 'crt', 'scalar', 'ragged_x', 'ragged_y'}),
                     ('t%d_bf16_c%d_w68' % (k, cb), (2, 6, 68, cb, k), True, {'tile', 'crt', 'ragged_x', 'ragged_y', 'multi_block_x'}),
                     ('t%d_bf16_c3_w7' % k, (1, 5, 7, 3, k), True, {'tile', 'cc3', 'ragged_x', 'ragged_y'})]
        else:
            big = (1, 6, 131, 3, k) if k == 11 else (2, 3, 131, 3, k)
            rows += [('r%d_f32_c3_w131' % k, big, False, {'rows', 'cc3', 'ragged_x', 'multi_block_x'}),
                     ('r%d_f32_c%d_w65' % (k, ca), (1, 2, 65, ca, k), False, {'rows', 'crt', 'ragged_x', 'multi_block_x'}),
                     ('r%d_bf16_c%d_w131' % (k, cb), (2, 3, 131, cb, k), True, {'rows', 'crt', 'ragged_x', 'multi_block_x'}),
                     ('r%d_bf16_c3_w65' % k, (1, 2, 65, 3, k), True, {'rows', 'cc3', 'ragged_x', 'multi_block_x'})]
        if k >= 2:
            hw = (2, 3) if k >= 4 else (k - 1, k - 1)
            fam = 'tile' if k < ROWS_MIN else 'rows'
            rows += [('s%d_f32_c3' % k, (1,) + hw + (3, k), False, {fam, 'cc3', 'smaller_than_halo', 'ragged_x'}),
                     ('s%d_bf16_c%d' % (k, ca), (1,) + hw + (ca, k), True, {fam, 'crt', 'smaller_than_halo', 'ragged_x'})]
    # odd k of the tile kernel: the other two of (cc3 | crt) x (vec | scalar), so that each channel body meets each staging; at
    # k = 5 with C = 2, which nothing ran before, in both storage types
    for k, cv in ((1, 4), (3, 2), (5, 2)):
        rows += [('t%d_f32_c%d_w68' % (k, cv), (2, 6, 68, cv, k), False, {'tile', 'crt', 'vec', 'ragged_x', 'ragged_y', 'multi_block_x'}),
                 ('t%d_f32_c3_w7' % k, (1, 5, 7, 3, k), False, {'tile', 'cc3', 'scalar', 'ragged_x', 'ragged_y'})]
    rows += [('t5_bf16_c2_w7', (1, 5, 7, 2, 5), True, {'tile', 'crt', 'ragged_x', 'ragged_y'})]
    return rows


PATH_CASES = _path_cases()
PATH_NAMES = [r[0] for r in PATH_CASES]
BY_NAME = {r[0]: r for r in PATH_CASES}

# What ran before this table (tests/op_cases.py DNA_SHAPES through test_dna / test_dna_bias in float32 and test_dna_bf16 - with
# (2, 128, 128, 3, 11) - in bf16; case_dna_second, case_dna_extreme_logits; tests/bn_cases.py DNA_ACC_SHAPES in both storage
# types), for the before / after list of (ksize, storage, C, family, staging).
OLD_LAUNCHES = ([(s, False) for s in [(2, 64, 64, 3, 5), (1, 16, 16, 3, 6), (1, 24, 20, 3, 11), (2, 7, 5, 3, 5), (1, 3, 3, 1, 5), (1, 8, 8, 4, 3),
                                      (1, 9, 70, 3, 7), (2, 5, 130, 1, 6), (1, 6, 33, 4, 9), (1, 4, 4, 2, 8)]]
                + [(s, True) for s in [(2, 64, 64, 3, 5), (1, 16, 16, 3, 6), (1, 24, 20, 3, 11), (2, 7, 5, 3, 5), (1, 3, 3, 1, 5), (1, 8, 8, 4, 3),
                                       (1, 9, 70, 3, 7), (2, 5, 130, 1, 6), (1, 6, 33, 4, 9), (1, 4, 4, 2, 8), (2, 128, 128, 3, 11)]]
                + [(s, False) for s in [(2, 16, 12, 3, 5), (1, 9, 20, 3, 6), (1, 8, 8, 3, 11), (1, 6, 6, 3, 5)]]
                + [(s, hf) for s in [(2, 7, 5, 3, 5), (130, 32, 3, 3, 5), (1, 9, 70, 3, 7), (50, 21, 5, 1, 6)] for hf in (False, True)])


# ----------------------------------------------------------------------------------------------- helpers
def reference(ld, bd, img, k):
    """The float64 reference of the frame: models.py:60-72 on logits + bias.  The sensitivity tests replace this."""
    return T.dna_gather(ld + bd, img, k)


def tap_ij(t, k):
    """Tap t of a pixel's k*k logits weighs the window element (row i, column j).  The sensitivity tests replace this."""
    return t // k, t % k


def window_taps(img, k):
    """[B, H, W, k*k, C]: the window element each tap weighs, for the saturated backward.  The sensitivity tests replace this."""
    return T.extract_image_patches(img, k)


def guarded(shape, dtype, dev, fill=float('nan')):
    """A tensor of ``shape`` filled with ``fill`` inside a larger buffer, GUARD sentinel elements in front of it and behind it
    -> (buffer, tensor).  The tensor starts on a 16-byte boundary, as the ABI demands."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0, 'test premise: the guarded tensor is 16-byte aligned'
    return buf, view.view(shape)


def guards_intact(buf, what):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]]).float().cpu()
    assert bool((g == SENTINEL).all()), '%s: %d guard elements next to the tensor were written' % (what, int((g != SENTINEL).sum()))


def bits(t):
    """The tensor's bit patterns (NaN compares equal to itself here)."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def store_logits(abi, logits, half):
    """float32 [.., kk] as it is, or bf16 at the pitch round8(kk) with zero pad taps (what graph.py keeps there)."""
    dev = abi.device
    if not half:
        return logits.to(dev)
    kk = logits.shape[-1]
    l16 = torch.zeros(*logits.shape[:-1], round8(kk), dtype=torch.bfloat16, device=dev)
    l16[..., :kk] = logits.to(dev).to(torch.bfloat16)
    return l16


def run_fwd(abi, lg, img, k, bias, what):
    """acg_dna_fwd into a NaN-filled, guarded frame: the guards stay, no NaN remains."""
    buf, out = guarded(tuple(img.shape), torch.float32, abi.device)
    abi.dna_fwd(lg, img, k, bias=bias, out=out)
    abi.sync()
    guards_intact(buf, what + ' out')
    assert not bool(torch.isnan(out).any()), '%s: %d elements of out were not written' % (what, int(torch.isnan(out).sum()))
    return out


def run_bwd(abi, lg, img, dout, k, bias, what, dout2=None, dout2_off=0):
    """acg_dna_bwd into NaN-filled, guarded dlogits and dbias: the guards stay, no NaN remains in the taps [0, k*k), and every bf16
    pad tap [k*k, round8(k*k)) is still NaN or exactly zero (the tile kernel zeroes the rest of the last 4-group, the rows kernel
    tap k*k when k*k is odd; callers keep them zero by zero-initialising) -> (dlogits as stored, dbias)."""
    kk = k * k
    bufl, dl = guarded(tuple(lg.shape), lg.dtype, abi.device)
    bufb, db = guarded((kk,), torch.float32, abi.device)
    abi.dna_bwd(lg, img, dout, k, bias=bias, dout2=dout2, dout2_off=dout2_off, dbias=db, accumulate=0.0, dlogits=dl)
    abi.sync()
    guards_intact(bufl, what + ' dlogits')
    guards_intact(bufb, what + ' dbias')
    taps = dl[..., :kk]
    assert not bool(torch.isnan(taps).any()), '%s: %d taps of dlogits were not written' % (what, int(torch.isnan(taps).sum()))
    assert not bool(torch.isnan(db).any()), '%s: dbias was not written' % what
    pad = dl[..., kk:].float()
    assert bool((torch.isnan(pad) | (pad == 0)).all()), '%s: a pad tap of dlogits holds something other than its prefill or zero' % what
    return dl, db


# ----------------------------------------------------------------------------------------------- every path against float64
def case_dna_path(abi, name):
    """One row of PATH_CASES: forward, backward (dlogits, dbias) and backward with a second gradient home, against float64
    autograd of ``reference``; outputs prefilled with NaN between guards; a second launch bit-equal (dna.hip has no atomics).
    k = 1: softmax over one tap is 1 whatever the logit and the bias, so the kernels' arithmetic (e = 1, inv = 1, g - dot = 0) gives
    out == image and dlogits == dbias == 0 EXACTLY; close() would divide by a zero scale there."""
    _, shape, half, want = BY_NAME[name]
    b, h, w, c, k = shape
    got = dna_paths(b, h, w, c, k, half)
    assert want <= got, '%s: the shape no longer reaches %s (it takes %s): move the row' % (name, sorted(want - got), sorted(got))
    kk, dev = k * k, abi.device
    seed = 2000 + 10 * PATH_NAMES.index(name)
    logits = randn((b, h, w, kk), seed, 2.0)
    logits = r16(logits) if half else logits
    bias, img = randn((kk,), seed + 3, 1.0), uniform((b, h, w, c), seed + 1)
    dout = randn((b, h, w, c), seed + 2)
    pitch, off = 8, 8 - c
    dt2 = torch.bfloat16 if half else torch.float32
    d2 = torch.full((b, h, w, pitch), 5.0)                            # channels outside the window must not be read
    d2[..., off:off + c] = randn((b, h, w, c), seed + 4)
    d2 = d2.to(dt2)
    ld, bd = logits.double().requires_grad_(True), bias.double().requires_grad_(True)
    out_ref = reference(ld, bd, img.double(), k)
    dl_ref, db_ref = torch.autograd.grad(out_ref, [ld, bd], dout.double(), retain_graph=True)
    dl_ref2, db_ref2 = torch.autograd.grad(out_ref, [ld, bd], dout.double() + d2[..., off:off + c].double())
    lg, imgd, doutd, biasd, d2d = store_logits(abi, logits, half), img.to(dev), dout.to(dev), bias.to(dev), d2.to(dev)
    tag = 'dna path %s %s %s' % (name, shape, 'bf16' if half else 'f32')
    tol_dl, tol_db = (TOL16, TOL16) if half else (4 * TOL, 8 * TOL)

    out = run_fwd(abi, lg, imgd, k, biasd, tag)
    dl, db = run_bwd(abi, lg, imgd, doutd, k, biasd, tag)
    dl2, db2 = run_bwd(abi, lg, imgd, doutd, k, biasd, tag + ' +dout2', dout2=d2d, dout2_off=off)
    if k == 1:
        assert torch.equal(out.cpu(), img), tag + ': k = 1 must return the image itself'
        for t, what in ((dl[..., 0], 'dlogits'), (dl2[..., 0], 'dlogits (+dout2)'), (db, 'dbias'), (db2, 'dbias (+dout2)')):
            assert bool((t == 0).all()), '%s: k = 1 %s must be exactly zero' % (tag, what)
    else:
        close(out, out_ref, TOL, tag + ' fwd')
        close(dl[..., :kk].float(), dl_ref, tol_dl, tag + ' dlogits')
        close(db, db_ref, tol_db, tag + ' dbias')
        close(dl2[..., :kk].float(), dl_ref2, tol_dl, tag + ' dlogits (+dout2)')
        close(db2, db_ref2, tol_db, tag + ' dbias (+dout2)')
    again = (run_fwd(abi, lg, imgd, k, biasd, tag), *run_bwd(abi, lg, imgd, doutd, k, biasd, tag))
    for a, o, what in zip(again, (out, dl, db), ('out', 'dlogits', 'dbias')):
        assert torch.equal(bits(a), bits(o)), '%s: a second launch gave another %s' % (tag, what)


# ----------------------------------------------------------------------------------------------- the tap map without an oracle
FAMILY_SHAPE = {'tile': (2, 5, 68, 3), 'rows': (2, 3, 70, 3)}       # ragged in x (and y), beyond one block, batch > 1


def family_shape(k):
    return FAMILY_SHAPE['tile' if k < ROWS_MIN else 'rows']


# (k, half, mode): 'hot' +40 on one tap per pixel, 'cold' -40 on one tap per pixel, 'extreme30' / 'extreme90': the pattern of
# op_cases.case_dna_extreme_logits (one tap far above the rest of its pixel, a whole pixel far below zero) at 30 and at that
# case's own 90, through the rows kernel and through bf16
ONE_HOT_CASES = ([(k, half, mode) for k in range(1, 12) for half in (False, True) for mode in ('hot', 'cold')]
                 + [(k, half, mode) for (k, half) in ((7, False), (7, True), (5, True)) for mode in ('extreme30', 'extreme90')])


def case_dna_one_hot(abi, k, half, shape, mode='hot'):
    """Saturated softmax.  The tap of pixel (b, y, x) is (3 y + 5 x + b) % (k*k): every tap occurs and neighbours differ.
    'hot': forward must return image[y + i - p, x + j - p] (zero outside the frame), p = (k - 1) // 2, computed here by indexing:
    the other k*k - 1 taps weigh e^-40 each, so the bound is k*k e^-40 plus one float32 rounding of a value below 1 (2^-24).
    Backward of 'hot' cannot be held to max |reference|: every true dlogit is of the order e^-40 = 4e-18, below the 2^-53 that
    float64 resolves next to the hot tap's weight of 1, so the reference's own hot-tap value (m (g - dot) with dot = g to 1e-16)
    is rounding noise of its own size (measured on these shapes, relative to max |reference|: the C oracle's double arithmetic is
    3e-8, 2.0, 1.0 and 0.67 off the float64 autograd at k = 2, 5, 7, 11, float32 torch 1.0 at each - four times that is no bar).
    It is held instead, tap by tap, to the forward error bound of dl_t = m_t (g_t - dot):
    |err_t| <= tol m_t (G_t + sum_s m_s G_s), G_t = sum_c |dout_c| |window_t,c| - tol the same 4 TOL (float32) / 6e-3 (bf16) as
    everywhere; dbias to the sum of that bound over the pixels.  A wrong tap or a sentinel slot leaking in moves dl_t by the order
    of m_t G_t, a thousand times the bound.
    'cold' and 'extreme': forward and backward against float64 at the usual bars (those softmaxes keep k*k - 1 ordinary taps)."""
    b, h, w, c = shape
    kk, dev = k * k, abi.device
    seed = 3000 + 20 * k + (10 if half else 0)
    assert math.exp(-40.0) < 2.0 ** -53
    if mode in ('hot', 'cold'):
        bi, yi, xi = torch.meshgrid(torch.arange(b), torch.arange(h), torch.arange(w), indexing='ij')
        tap = (3 * yi + 5 * xi + bi) % kk
        logits = torch.zeros(b, h, w, kk)
        logits.scatter_(3, tap.unsqueeze(-1), 40.0 if mode == 'hot' else -40.0)
    else:
        amp = float(mode[len('extreme'):])
        logits = randn((b, h, w, kk), seed, 1.0)
        logits = r16(logits) if half else logits
        logits[0, 2, 3, 7] = amp
        logits[0, h - 1, 1, :] = -amp
    img, dout = uniform((b, h, w, c), seed + 1), randn((b, h, w, c), seed + 2)
    lg, imgd, doutd = store_logits(abi, logits, half), img.to(dev), dout.to(dev)
    tag = 'dna %s k=%d %s %s' % (mode, k, shape, 'bf16' if half else 'f32')
    tol_dl, tol_db = (TOL16, TOL16) if half else (4 * TOL, 8 * TOL)
    out = run_fwd(abi, lg, imgd, k, None, tag)
    dl, db = run_bwd(abi, lg, imgd, doutd, k, None, tag)
    dl = dl[..., :kk].float()

    ld = logits.double().requires_grad_(True)
    out_ref = T.dna_gather(ld, img.double(), k)
    if mode == 'hot':
        p = (k - 1) // 2
        ti, tj = tap_ij(tap, k)
        ys, xs = yi + ti - p, xi + tj - p
        inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
        expect = img[bi, ys.clamp(0, h - 1), xs.clamp(0, w - 1)] * inside.unsqueeze(-1)
        err = float((out.cpu().double() - expect.double()).abs().max())
        assert err <= kk * math.exp(-40.0) + 2.0 ** -24, '%s fwd: %.3e off the hot tap\'s window element' % (tag, err)
        if k == 1:
            assert bool((dl == 0).all()) and bool((db == 0).all()), tag + ': k = 1 gradients must be exactly zero'
            return
        m = torch.softmax(logits.double(), dim=-1)
        patches = window_taps(img.double(), k)                                                  # [B, H, W, kk, C]
        g = (patches * dout.double().unsqueeze(3)).sum(-1)
        gabs = (patches.abs() * dout.double().abs().unsqueeze(3)).sum(-1)
        want = m * (g - (m * g).sum(-1, keepdim=True))
        bound = m * (gabs + (m * gabs).sum(-1, keepdim=True))
        got = dl.double().cpu()
        assert torch.isfinite(got).all() and torch.isfinite(db).all(), tag + ': non-finite gradient'
        bad = (got - want).abs() > tol_dl * bound
        assert not bool(bad.any()), '%s dlogits: %d of %d taps beyond %.1e of their forward error scale' % (tag, int(bad.sum()), bad.numel(), tol_dl)
        db_err = (db.double().cpu() - want.sum((0, 1, 2))).abs()
        assert bool((db_err <= tol_db * bound.sum((0, 1, 2))).all()), '%s dbias: beyond %.1e of its forward error scale' % (tag, tol_db)
        return
    dl_ref, = torch.autograd.grad(out_ref, [ld], dout.double())
    if k == 1:                                   # one tap: weight 1 at any logit
        assert torch.equal(out.cpu(), img) and bool((dl == 0).all()) and bool((db == 0).all()), tag + ': k = 1 is the identity'
        return
    close(out, out_ref, TOL, tag + ' fwd')
    close(dl, dl_ref, tol_dl, tag + ' dlogits')
    close(db, dl_ref.sum((0, 1, 2)), tol_db, tag + ' dbias')


# ----------------------------------------------------------------------------------------------- the second home at any C
SECOND_CASES = [(c, k, dt) for c in RUNTIME_C for k in (3, 7) for dt in ('f32', 'bf16')] + [(3, 6, 'f32'), (3, 6, 'bf16')]


def second_shape(c, k):
    """Ragged shapes beyond one block; C = 3 at k = 6: the one-vector-store pixel of the rows kernel."""
    return (2, 5, 68, c, k) if k < ROWS_MIN else (1, 3, 70, c, k)


def second_layouts(c):
    """(offset, pitch): one element past a 16-byte boundary, and flush with the end of the pixel ((4, 8) at C = 4).  C = 3 at
    (3, 8) is concat(image, frame): there the WHOLE pixel is written, image channels and zero pad included."""
    return [(3, 8), (1, 8)] if c == 3 else sorted({(1, 8), (8 - c, 8)})


def case_dna_second_any_c(abi, c, k, dt):
    """acg_dna_fwd out2 / acg_dna_bwd dout2 with C = 1, 2, 4 (second_store / second_load, scalar; in the rows kernel lane 4 of a
    pixel's 16 stores while lanes 0 .. C-1 store out): the frame channels equal out bit for bit after rounding to the second
    tensor's type, every other channel of the prefilled tensor and the guards around it stay, the frame itself does not change, and
    backward with a gradient window equals backward of the explicit sum."""
    dt = {'f32': torch.float32, 'bf16': torch.bfloat16}[dt]
    shape = second_shape(c, k)
    b, h, w, _, _ = shape
    dev = abi.device
    lg, img = randn((b, h, w, k * k), 3500 + 10 * k + c, 2.0).to(dev), uniform((b, h, w, c), 3501 + 10 * k + c).to(dev)
    bias = randn((k * k,), 3502 + 10 * k + c, 0.3).to(dev)
    ref = abi.dna_fwd(lg, img, k, bias=bias)
    for off, pitch in second_layouts(c):
        tag = 'dna second %s %s off %d pitch %d' % (shape, dt, off, pitch)
        buf, out2 = guarded((b, h, w, pitch), dt, dev, fill=7.0)
        out = abi.dna_fwd(lg, img, k, bias=bias, out2=out2, out2_off=off)
        abi.sync()
        guards_intact(buf, tag)
        assert torch.equal(out.cpu(), ref.cpu()), tag + ': the second output changed the frame'
        assert torch.equal(out2[..., off:off + c].float().cpu(), ref.to(dt).float().cpu()), tag + ': frame channels'
        if (c, off, pitch) == (3, 3, 8):
            assert torch.equal(out2[..., :3].float().cpu(), img.to(dt).float().cpu()) and bool((out2[..., 6:] == 0).all()), tag + ': concat(image, frame) pixel'
        else:
            assert bool((out2[..., :off] == 7).all()) and bool((out2[..., off + c:] == 7).all()), tag + ': wrote outside its channels'
        dout = randn((b, h, w, c), 3503 + 10 * k + c).to(dev)
        d2 = torch.full((b, h, w, pitch), 5.0, dtype=dt, device=dev)                               # must not be read
        d2[..., off:off + c] = randn((b, h, w, c), 3504 + 10 * k + c).to(dev).to(dt)
        got = abi.dna_bwd(lg, img, dout, k, bias=bias, dout2=d2, dout2_off=off)
        want = abi.dna_bwd(lg, img, dout + d2[..., off:off + c].float(), k, bias=bias)
        abi.sync()
        close(got, want.double().cpu(), 1e-5, tag + ' gradient')


# ----------------------------------------------------------------------------------------------- the three kernels against each other
def dimage_f64(logits, bias, g, k):
    """Brute force: dimage[y, x] = sum over taps (i, j) of softmax(logits + bias)[y', x'][i k + j] * g[y', x'],
    y' = y + p - i, x' = x + p - j, over in-range sources."""
    b, h, w, c = g.shape
    p = (k - 1) // 2
    z = logits + (bias if bias is not None else 0.0)
    wts = torch.softmax(z, dim=-1)                                         # [B, H, W, k*k]
    out = torch.zeros_like(g)
    for i in range(k):
        for j in range(k):
            t = i * k + j
            contrib = wts[..., t:t + 1] * g                                # at the source pixel
            for y in range(h):
                ys = y + p - i
                if not 0 <= ys < h:
                    continue
                x_lo, x_hi = max(0, j - p), min(w, w + j - p)               # x with 0 <= x + p - j < w
                if x_lo < x_hi:
                    out[:, y, x_lo:x_hi] += contrib[:, ys, x_lo + p - j:x_hi + p - j]
    return out


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dna_bwd_image(abi, logits, bias, dout, k):
    """acg_dna_bwd_image (include/acgan_rollout.h; the HIP library only) -> dimage."""
    b, h, w, c = dout.shape
    dimg = torch.full((b, h, w, c), float('nan'), device=abi.device)
    abi.lib.dna_bwd_image(_p(logits), _p(bias), _p(dout), None, 0, 0, L.ACG_F32, _p(dimg), 0.0, b, h, w, c, k, L.ACG_F32, abi.stream())
    return dimg


# per k one ragged shape: H % 4 != 0, W % 64 != 0 and W % 32 != 0 (dna_dimage_kernel owns 32 x 32 tiles), C through 3, 1, 2, 4; at k = 5 and
# k = 11 beyond one 64-pixel block of the forward kernels
ADJOINT_SHAPES = [(2, 7, 37, (3, 1, 2, 4)[k % 4], k) if k not in (5, 11) else (1, 5, 70, 3, k) for k in range(1, 12)]


def case_dna_adjoint(abi, shape):
    """acg_dna_bwd_image is the adjoint of acg_dna_fwd in the image: <dna_fwd(img), dout> == <img, dna_bwd_image(dout)>, both
    accumulated in float64 on the host, to 1e-5 ||fwd|| ||dout|| (the scale convention of the conv adjoint test in
    op_cases.case_full_size_properties at the 1e-5 of test_image_gradient_matches_float64)."""
    b, h, w, c, k = shape
    dev = abi.device
    lg, bias = randn((b, h, w, k * k), 3800 + k, 2.0).to(dev), randn((k * k,), 3801 + k, 1.0).to(dev)
    img, dout = uniform((b, h, w, c), 3802 + k), randn((b, h, w, c), 3803 + k)
    fwd = abi.dna_fwd(lg, img.to(dev), k, bias=bias)
    dimg = dna_bwd_image(abi, lg, bias, dout.to(dev), k)
    abi.sync()
    fwd, dimg = fwd.double().cpu(), dimg.double().cpu()
    assert torch.isfinite(fwd).all() and torch.isfinite(dimg).all(), 'dna adjoint %s: non-finite values' % (shape,)
    lhs, rhs = float((fwd * dout.double()).sum()), float((img.double() * dimg).sum())
    bar = 1e-5 * float(fwd.norm()) * float(dout.double().norm())
    assert abs(lhs - rhs) <= bar, 'dna adjoint %s: <fwd, dout> = %.9e, <img, dimage> = %.9e, apart by %.3e > %.3e' % (shape, lhs, rhs, abs(lhs - rhs), bar)


def launched():
    """-> (before, after): the sets of (ksize, storage, C, family, staging) of OLD_LAUNCHES and of the tables of this file."""
    before = {combo(*s, hf) for s, hf in OLD_LAUNCHES}
    after = {combo(*r[1], r[2]) for r in PATH_CASES}
    after |= {combo(*family_shape(k)[:3], family_shape(k)[3], k, hf) for k, hf, _ in ONE_HOT_CASES}
    after |= {combo(*second_shape(c, k), False) for c, k, _ in SECOND_CASES}
    return before, after

