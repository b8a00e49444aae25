"""BatchNorm at every kernel path of bn.hip, storage type and accumulate mode, against float64 (shared by the GPU suite, which
also asserts WHICH kernel family ran, and - float32 rows of moderate size - the CPU suite on the C oracle, which proves the
references, inputs, premises and bars without a GPU).

The host picks a kernel from the rows per group R, the channel count C, `groups`, pointer alignment, the storage types, the
slabs and ACG_BN_NO_GRID_EXCHANGE: bn.hip states that rule once, in fwd_path / bwd_path (tools/bn_path_sweep.hip prints it as
a table without a GPU).  Every row of PATH_ROWS and SLAB_ROWS states the family it is there for, in each direction; the test
reads the family back out of the workspace (abi_call.bn_path: what acgan_hip.h documents about it) and fails with the name
of the path that lost its case when a retune moves the shape - correct the table then from those two functions, and keep a
case on every path.  profiles/bn_host/README.md lists, for every launch statement of the dispatcher, the case that reaches
each of its (V, slabs, storage types) arms.

Inputs keep every pre-activation away from the kink of relu / lrelu (where float32 and float64 legitimately pick different
derivatives): per channel x = shift + scale * s * u with s = +-1 in antithetic pairs (so the column mean is the shift) and u
uniform in [0.5, 1.5], |beta| <= 0.25: |x-hat| >= 0.48, |x-hat + beta| >= 0.2, both branches taken.  Each case asserts
min |pre-activation| > 0.05 on the float64 reference before it looks at the kernel.

The resident kernels with more than 8 rows per thread and the apply kernels with 16 channel lanes exist in a tuning build only
(bn.hip pick_nr / pick_cl): the package's library has nothing here that these tables leave out on purpose."""
import torch

import op_cases as C
from abi_call import bn_grid_rows, bn_path
from action_conditioned_gans_amd import _lib as L
from op_cases import SENTINEL, _bn_ref, _guarded, _guards_intact, _rng, close, r16, randn

TOL = 2e-5                    # float32: y, mean, rstd, dx from LARGE_ROWS on; 4 * TOL: dx below, dbeta (tests/test_gpu_ops.py)
TOL16 = 6e-3                  # bf16-stored outputs (test_bn_bf16)
ACTS = (None, 'relu', 'lrelu')
NOMINAL_CUS = 256             # CU count the sizes in the comments are worked out for; the GPU suite passes the device's own

RES, TWO = ('resident', None), ('two_launch', None)


def grid(rows_per_block):
    return ('grid', rows_per_block)


def path_rows(ncu):
    """(name, R, C, groups, flags, align, forward path, backward path, activations, storage types).
    fused_shape: cap1 = min(CUs, 512) blocks of 1024 threads (512 or 1024 rows), cap2 = min(2 CUs, 512) blocks of 256 threads
    (128 rows, at most 16 row blocks per (group, chunk)); resident_nr: <= 2048 rows per group forward, <= 2048 rows over ALL
    groups backward; backward prefers the grid kernel from 2048 rows per group on.  V = 4 needs C % 4 == 0, pitches % 4 == 0,
    16-byte aligned pointers and one storage type; the grid kernels need V = 4."""
    cap1 = min(ncu, 512)
    r_1024 = 512 * (cap1 // 2) + 1      # groups = 2, one chunk: first R with ceil(R / 512) * 2 > cap1 (65537 x 2 at 256 CUs: 2 MB)
    r_nofit = 1024 * cap1 + 1           # groups = 1, one chunk: first R with ceil(R / 1024) > cap1 (262145 at 256 CUs: 4 MB)
    assert -(-r_1024 // 512) * 2 > cap1 >= -(-r_1024 // 1024) * 2 and -(-r_nofit // 1024) > cap1, 'test premise: sizes derived from the CU count'
    NG = L.BN_NO_GRID_EXCHANGE
    f, h, a = ('f32',), ('f32', 'bf16'), ('f32', 'bf16', 'bf16_f32', 'f32_bf16')
    hd = h + ('f32_bf16',)      # with the float32 head of a bf16 network (bf16 dx) on the V = 4 kernels of each family
    return [
        # register-resident, V = 4: NR = 1 / 2 / 4 / 8 at the last size of each and the first of the next
        ('res_v4_nr1', 256, 8, 1, 0, None, RES, RES, ACTS, f),
        ('res_v4_nr2_first', 257, 8, 2, 0, None, RES, RES, ACTS, f),
        ('res_v4_nr2', 512, 8, 1, 0, None, RES, RES, ACTS, f),
        ('res_v4_nr4_first', 513, 8, 3, 0, None, RES, RES, ACTS, hd),
        # backward: the resident limit counts the rows of ALL groups - 2 x 1024 is the last resident size, 2 x 1025 goes to the
        # 256-thread grid kernel (9 row blocks x 2 groups)
        ('res_v4_nr4_bwd_limit', 1024, 8, 2, 0, None, RES, RES, ACTS, f),
        ('res_v4_nr8_first', 1025, 8, 1, 0, None, RES, RES, ACTS, f),
        ('bwd_past_group_limit', 1025, 8, 2, 0, None, RES, grid(128), ACTS, h),
        ('res_v4_nr8_bwd_last', 2047, 8, 1, 0, None, RES, RES, ACTS, f),
        # 2048: the last resident forward; backward prefers the grid kernel from here (16 row blocks of 256 threads x 128 rows)
        ('res_fwd_last_grid128_bwd', 2048, 8, 1, 0, None, RES, grid(128), ACTS, hd),
        ('res_v1_nr8', 2048, 7, 1, 0, None, RES, RES, ACTS, a),
        ('res_v1_many_channels', 40, 1023, 2, 0, None, RES, RES, ACTS, h),
        # one-launch grid kernels; 40 channels: two chunks, the second ragged
        ('grid512', 2049, 40, 2, 0, None, grid(512), grid(512), ACTS, hd),
        ('grid1024', r_1024, 4, 2, 0, None, grid(1024), grid(1024), ACTS, h),
        # two launches
        ('two_v4_grid_does_not_fit', r_nofit, 4, 1, 0, None, TWO, TWO, ('relu',), h),
        ('two_v4_deep_several_batches', 2049, 1024, 1, NG, None, TWO, TWO, ('lrelu',), h),      # 8 MB
        ('two_v4_shallow', 2049, 8, 3, NG, None, TWO, TWO, ACTS, hd),
        ('two_v1', 2100, 7, 2, 0, None, TWO, TWO, ACTS, a),
        ('two_v1_channel_chunks', 2100, 259, 1, 0, None, TWO, TWO, ACTS, h),
        # V = 1 by alignment alone: C = 8, x (then dbeta) one float into its buffer.  Aligned, 2100 x 8 runs the grid kernel
        ('align_x_resident', 300, 8, 2, 0, 'x', RES, RES, ACTS, f),
        ('align_x_two', 2100, 8, 1, 0, 'x', TWO, TWO, ACTS, f),
        ('align_dbeta_resident', 300, 8, 2, 0, 'dbeta', RES, RES, ACTS, f),
        ('align_dbeta_two', 2100, 8, 1, 0, 'dbeta', grid(512), TWO, ACTS, f),
    ]


PATH_CASES = [(r[0], st) for r in path_rows(NOMINAL_CUS) for st in r[9]]
ORACLE_BYTES = 1 << 20        # float32 rows up to this size (and independent of the CU count) also run on the C oracle
ORACLE_CASES = [r[0] for r in path_rows(NOMINAL_CUS) if r[1] * r[2] * r[3] * 4 <= ORACLE_BYTES and r[0] not in ('grid1024', 'two_v4_grid_does_not_fit')]
LARGE_ROWS = 100000           # rows per group from which the `large tensor` bars of case_bn_large_tensor apply (float32 dx: 2e-5; bf16 dbeta: 3e-4)


def row_named(name, ncu=NOMINAL_CUS):
    return next(r for r in path_rows(ncu) if r[0] == name)


def kink_free(R, c, groups, seed):
    """float64 [groups * R, c]: see the module docstring."""
    g = _rng(seed)
    u = torch.rand((groups, R // 2, c), generator=g, dtype=torch.float64) + 0.5
    cols = [u, -u]
    if R % 2:
        cols.append(torch.rand((groups, 1, c), generator=g, dtype=torch.float64) + 0.5)
    su = torch.cat(cols, dim=1)[:, torch.randperm(R, generator=g)]
    ch = torch.arange(c, dtype=torch.float64)
    return ((0.7 + 0.5 * torch.cos(ch)) + (1.5 + 0.4 * torch.sin(ch)) * su).reshape(groups * R, c)


def reference(x, beta, dy, act, groups, what):
    """x, dy [rows, C], beta [C] as stored -> float64 (y, mean, rstd, dx, dbeta); asserts the kink premise."""
    xd = x.double().reshape(x.shape[0], 1, 1, x.shape[1]).requires_grad_(True)
    bd = beta.double().requires_grad_(True)
    pre = _bn_ref(xd.detach(), bd.detach(), None, groups)
    gap = pre.abs().min().item()
    assert gap > 0.05, '%s: test premise: a pre-activation lies %.3g from the kink' % (what, gap)
    if act is not None:
        assert bool((pre > 0).any()) and bool((pre < 0).any()), what + ': test premise: both branches of the activation'
    y = _bn_ref(xd, bd, act, groups)
    dx, db = torch.autograd.grad(y, [xd, bd], dy.double().reshape(y.shape))
    xg = xd.detach().reshape(groups, -1, x.shape[1])
    mean, var = xg.mean(1), xg.var(1, unbiased=False)
    return y.detach().reshape(x.shape), mean.reshape(-1), (1.0 / torch.sqrt(var + 1e-3)).reshape(-1), dx.reshape(x.shape), db


def _expect(path, got_ws, R, c, groups, tag):
    fam, slots = bn_path(got_ws)
    assert fam == path[0], '%s: the %s kernels ran where this case is there for the %s path - that path lost its case' % (tag, fam, path[0])
    if fam == 'grid':
        rows = bn_grid_rows(slots, R, c, groups)
        assert rows == path[1], '%s: a grid of %d blocks (%s rows per block) ran where this case is there for the %d-row grid kernel' % (
            tag, slots, rows, path[1])


def _store(t, cp, dtype, dev, pad=0.0, fill=None):
    """[rows, C] float -> [rows, cp] of ``dtype`` on ``dev``, pad channels ``pad`` (``fill``: the valid channels too)."""
    out = torch.full((t.shape[0], cp), pad, dtype=dtype, device=dev)
    out[:, :t.shape[1]] = (t if fill is None else torch.full_like(t, fill)).to(dev).to(dtype)
    return out


ACCUMULATE = (0.0, 1.0, 0.5)


def case_bn_path(abi, name, storage, ncu=None):
    """One row of PATH_ROWS in one storage layout - 'f32' dense float32; 'bf16' everything bf16 at the pitch round8(C);
    'bf16_f32' bf16 x / dx at round8(C), dense float32 y / dy; 'f32_bf16' float32 x at round8(C), dense float32 y / dy, bf16 dx.
    Forward: y, save_mean, save_rstd.  Backward from the float32-rounded reference statistics: dx and dbeta with accumulate 0
    (dbeta holding NaN before: it must not be read), 1 and 0.5 into a seeded vector; dx bit-identical across the three.
    ``ncu``: the device's CU count - the kernel family is asserted from the workspace; None (C oracle): no such assertion."""
    _, R, c, groups, flags, align, fpath, bpath, acts, _ = row_named(name, ncu or NOMINAL_CUS)
    dev = abi.device
    rows = R * groups
    half_x, half_y = storage in ('bf16', 'bf16_f32'), storage == 'bf16'
    cp = c if storage == 'f32' else (c + 7) // 8 * 8
    yp = cp if storage == 'bf16' else c
    tx, ty = (torch.bfloat16 if half_x else torch.float32), (torch.bfloat16 if half_y else torch.float32)
    td = torch.float32 if storage == 'f32' else torch.bfloat16
    seed = 4000 + 16 * [r[0] for r in path_rows(NOMINAL_CUS)].index(name)
    x = kink_free(R, c, groups, seed).float()
    beta = (torch.rand(c, generator=_rng(seed + 1), dtype=torch.float64) * 0.5 - 0.25).float()
    dy = randn((rows, c), seed + 2)
    x, dy = (r16(x) if half_x else x), (r16(dy) if half_y else dy)
    large = R >= LARGE_ROWS
    tol_y, tol_dx = (TOL16 if half_y else TOL), ((TOL if large else 4 * TOL) if storage == 'f32' else TOL16)
    tol_db = 4 * TOL if storage == 'f32' else (3e-4 if large else 2e-4)
    xs, dys, bg = _store(x, cp, tx, dev), _store(dy, yp, ty, dev), beta.to(dev)
    xbuf = dbuf = None
    if align == 'x':
        xbuf, v = _guarded(xs.reshape(-1), 1, dev)
        xs = v.view(rows, cp)
    abi.bn_flags = flags
    try:
        for act in acts:
            tag = 'bn path %s %s %s' % (name, storage, act)
            y_ref, mean_ref, rstd_ref, dx_ref, db_ref = reference(x, beta, dy, act, groups, tag)
            # ---- forward
            y0 = torch.zeros(rows, yp, dtype=ty, device=dev)
            y, mean, rstd, ws = abi.bn_act_fwd(xs, bg, act, groups, c=c, y=y0, want_ws=True)
            abi.sync()
            if ncu:
                _expect(fpath, ws, R, c, groups, tag + ' forward')
            close(y[:, :c].float(), y_ref, tol_y, tag + ' y')
            close(mean, mean_ref, TOL, tag + ' mean'); close(rstd, rstd_ref, TOL, tag + ' rstd')
            assert bool((y[:, c:] == 0).all()), tag + ': pad channels of y were written'
            # ---- backward, three accumulate modes on the same inputs
            prev = randn((c,), seed + 3, max(float(db_ref.abs().mean()), 1e-3))
            mg, rg = mean_ref.float().to(dev), rstd_ref.float().to(dev)
            first = None
            for acc in ACCUMULATE:
                start = torch.full((c,), float('nan')) if acc == 0 else prev.clone()
                if align == 'dbeta':
                    dbuf, dbeta = _guarded(start, 1, dev)
                else:
                    dbeta = start.to(dev)
                dx0 = torch.zeros(rows, cp, dtype=td, device=dev)
                dx, dbeta, ws = abi.bn_act_bwd(xs, dys, bg, mg, rg, act, groups, dbeta=dbeta, accumulate=acc, c=c, dx=dx0, want_ws=True)
                abi.sync()
                if ncu:
                    _expect(bpath, ws, R, c, groups, tag + ' backward')
                t2 = tag + ' accumulate %g' % acc
                close(dx[:, :c].float(), dx_ref, tol_dx, t2 + ' dx')
                close(dbeta, (acc * prev.double() if acc else 0.0) + db_ref, tol_db, t2 + ' dbeta')
                assert bool((dx[:, c:] == 0).all()), t2 + ': pad channels of dx were written'
                if dbuf is not None:
                    _guards_intact(dbuf, 1, t2 + ' dbeta')
                if first is None:
                    first = dx.clone()
                else:
                    assert torch.equal(dx, first), t2 + ': dx differs from the run with accumulate 0'
            if xbuf is not None:
                _guards_intact(xbuf, 1, tag + ' x')
    finally:
        abi.bn_flags = 0


# ---- slabs handed over by a split-K producer (acg_bn_act_fwd_slabs / acg_bn_act_bwd_slabs), called directly -------------------------
def slab_rows(ncu):
    """(name, R, C, groups, splits, flags, layout, forward path, backward path).  Rows layout: the grid kernels wherever their grid
    is resident - from two slabs on as 1024 threads x one row where 128-row blocks fit (fused_shape), else 256 threads x four
    rows - and, without V = 4 or a grid, whatever takes the tensor itself; quad layout: the resident kernels.  A backward path
    of None: acg_bn_slabs_layout answers -1 and acg_bn_act_bwd_slabs refuses (the two-launch kernels take no dy slabs)."""
    cap1 = min(ncu, 512)
    r_1024 = 512 * (cap1 // 2) + 1
    NG, RO, QU = L.BN_NO_GRID_EXCHANGE, L.SLABS_ROWS, L.SLABS_QUADS
    return [
        ('rows_grid128_wide', 256, 8, 1, 2, 0, RO, grid(128), grid(128)),
        ('rows_grid128_one_slab', 257, 8, 2, 1, 0, RO, grid(128), grid(128)),
        ('rows_grid512', 2049, 40, 2, 2, 0, RO, grid(512), grid(512)),
        ('rows_grid1024', r_1024, 4, 2, 2, 0, RO, grid(1024), grid(1024)),
        ('quads_resident', 256, 8, 1, 2, NG, QU, RES, RES),
        ('quads_resident_nr4', 513, 12, 3, 3, NG, QU, RES, RES),
        ('rows_v1_resident', 300, 7, 2, 2, 0, RO, RES, RES),
        ('rows_v4_two', 2049, 8, 1, 2, NG, RO, TWO, None),
        ('rows_v1_two', 2100, 7, 1, 2, 0, RO, TWO, None),
    ]


# (the mixed pair - bf16 x / dx, float32 y / dy - runs the scalar kernels: on the two rows that are there for them)
SLAB_CASES = [(r[0], st) for r in slab_rows(NOMINAL_CUS) for st in ('f32', 'bf16') + (('bf16_f32',) if r[0].startswith('rows_v1') else ())]


def _slabs_of(t, splits, cp, quads, seed, dev):
    """float32 [rows, C] -> (`splits` float32 slabs whose sum in slab order is close to t, that sum as float32 [rows, C]).  A slab is
    [rows][cp] (pad channels NaN: not read) or, ``quads``, [C / 4][rows][4]; slabs lie rows * cp floats apart."""
    rows, c = t.shape
    parts = [randn((rows, c), seed + z, 1.0) for z in range(splits - 1)]
    parts.append(t - sum(parts) if parts else t.clone())
    total = torch.zeros_like(t)
    for q in parts:
        total = total + q                                    # float32, slab order: what the kernels add up
    buf = torch.full((splits, rows * cp), float('nan'))
    for z, q in enumerate(parts):
        if quads:
            buf[z, :rows * c] = q.reshape(rows, c // 4, 4).permute(1, 0, 2).reshape(-1)
        else:
            buf[z].view(rows, cp)[:, :c] = q
    return buf.to(dev), total


def case_bn_slabs(abi, name, storage, ncu):
    """One row of SLAB_ROWS in the storage layouts of case_bn_path (bf16 at the pitch round8(C), float32 dense); the slabs are float32
    either way, pitched like the tensor they sum to.  Forward: x
    written back bit-identical to the slab sum rounded to its storage type, y / mean / rstd against float64 BatchNorm of that x.
    Backward: dx, dbeta against float64 with dy = the slab sum rounded to the storage type.  The family from the workspace."""
    from abi_call import ACT, _p
    _, R, c, groups, splits, flags, layout, fpath, bpath = next(r for r in slab_rows(ncu) if r[0] == name)
    dev, lib = abi.device, abi.lib
    rows, half, half_y = R * groups, storage != 'f32', storage == 'bf16'
    cp = (c + 7) // 8 * 8 if half else c
    yp = cp if half_y else c
    tt, ty = (torch.bfloat16 if half else torch.float32), (torch.bfloat16 if half_y else torch.float32)
    code = L.dtype2(L.code(tt), L.code(ty))
    quads = layout == L.SLABS_QUADS
    seed = 7000 + 16 * [r[0] for r in slab_rows(NOMINAL_CUS)].index(name)
    act = ACTS[seed // 16 % 3]
    tag = 'bn slabs %s %s %s' % (name, storage, act)
    for backward in (0, 1):
        want = -1 if (backward and bpath is None) else layout
        assert lib.bn_slabs_layout(rows, c, cp, yp, groups, code, backward, flags) == want, tag + ': test premise: acg_bn_slabs_layout'
    xslabs, x = _slabs_of(kink_free(R, c, groups, seed).float(), splits, cp, quads, seed + 4, dev)
    dslabs, dy = _slabs_of(randn((rows, c), seed + 2), splits, yp, quads, seed + 8, dev)
    x, dy = (r16(x) if half else x), (r16(dy) if half_y else dy)
    beta = (torch.rand(c, generator=_rng(seed + 1), dtype=torch.float64) * 0.5 - 0.25).float()
    y_ref, mean_ref, rstd_ref, dx_ref, db_ref = reference(x, beta, dy, act, groups, tag)
    bg = beta.to(dev)
    # ---- forward
    xs = torch.zeros(rows, cp, dtype=tt, device=dev)
    y = torch.zeros(rows, yp, dtype=ty, device=dev)
    mean, rstd = abi.empty(groups * c), abi.empty(groups * c)
    ws, n = abi.bn_ws(rows, c, groups)
    lib.bn_act_fwd_slabs(_p(xslabs), splits, _p(xs), _p(bg), _p(y), _p(mean), _p(rstd), rows, c, cp, yp, groups, 1e-3, ACT[act], 0.2, code, layout, flags,
                         _p(ws), n, abi.stream())
    abi.sync()
    abi.no_timeout(ws)
    _expect(fpath, ws, R, c, groups, tag + ' forward')
    assert torch.equal(xs[:, :c].float().cpu(), x), tag + ': x written back is not the slab sum rounded to its storage type'
    assert bool((xs[:, c:] == 0).all()) and bool((y[:, c:] == 0).all()), tag + ': pad channels were written'
    close(y[:, :c].float(), y_ref, TOL16 if half_y else TOL, tag + ' y')
    close(mean, mean_ref, TOL, tag + ' mean'); close(rstd, rstd_ref, TOL, tag + ' rstd')
    # ---- backward from the float32-rounded reference statistics, accumulating into a seeded dbeta
    xg = _store(x, cp, tt, dev)
    mg, rg = mean_ref.float().to(dev), rstd_ref.float().to(dev)
    prev = randn((c,), seed + 3, max(float(db_ref.abs().mean()), 1e-3))
    dbeta, dx = prev.clone().to(dev), torch.zeros(rows, cp, dtype=tt, device=dev)
    ws, n = abi.bn_ws(rows, c, groups)
    call = lambda: lib.bn_act_bwd_slabs(_p(xg), _p(dslabs), splits, _p(bg), _p(mg), _p(rg), _p(dx), _p(dbeta), 0.5, rows, c, cp, yp, groups, ACT[act], 0.2,
                                        code, layout, flags, _p(ws), n, abi.stream())
    if bpath is None:
        try:
            call()
        except L.AcgError as e:
            assert '(code 4)' in str(e) and 'bn_act_bwd_slabs:' in str(e), tag + ': ' + str(e)
        else:
            raise AssertionError(tag + ': acg_bn_act_bwd_slabs took a tensor no one-launch kernel fits')
        return
    call()
    abi.sync()
    abi.no_timeout(ws)
    _expect(bpath, ws, R, c, groups, tag + ' backward')
    large = R >= LARGE_ROWS
    close(dx[:, :c].float(), dx_ref, TOL16 if half else (TOL if large else 4 * TOL), tag + ' dx')
    close(dbeta, 0.5 * prev.double() + db_ref, (3e-4 if large else 2e-4) if half else 4 * TOL, tag + ' dbeta')
    assert bool((dx[:, c:] == 0).all()), tag + ': pad channels of dx were written'


# ---- statistics out of a producer's tile partials (acg_bn_act_fwd_partials), called directly -----------------------------------------
# (name, R, C, groups, block_rows, run_rows): more than 512 partial blocks per group - bn_partials_finalize merges them before the
# apply pass - with four channels per lane and with one; a ragged last block per run; and few blocks (merged in the apply prologue)
PARTIAL_ROWS = [
    ('finalize_v4', 1026, 8, 1, 2, 1026),
    ('finalize_v1_ragged', 1540, 7, 2, 3, 1540),
    ('prologue_v4', 96, 8, 2, 16, 48),
]
PARTIAL_CASES = [r[0] for r in PARTIAL_ROWS]


def case_bn_partials(abi, name):
    """float32 y, mean, rstd of acg_bn_act_fwd_partials against float64, from per-tile (sum, M2) partials computed in float64."""
    from abi_call import ACT, _p
    i, (_, R, c, groups, brows, rrows) = next((i, r) for i, r in enumerate(PARTIAL_ROWS) if r[0] == name)
    assert R % rrows == 0, 'test premise: whole runs'
    bpr = -(-rrows // brows)
    nblk = R // rrows * bpr
    assert (nblk > 512) == name.startswith('finalize'), 'test premise: %d partial blocks per group (bn.hip kFinalizeBlocks)' % nblk
    dev, seed, act = abi.device, 8000 + 16 * i, 'lrelu'
    rows = R * groups
    x = kink_free(R, c, groups, seed).float()
    beta = (torch.rand(c, generator=_rng(seed + 1), dtype=torch.float64) * 0.5 - 0.25).float()
    tag = 'bn partials ' + name
    y_ref, mean_ref, rstd_ref, _, _ = reference(x, beta, torch.zeros(rows, c), act, groups, tag)
    part = torch.zeros(groups, nblk, 2, c, dtype=torch.float64)
    xd = x.double().reshape(groups, R // rrows, rrows, c)
    for b in range(nblk):
        t = xd[:, b // bpr, (b % bpr) * brows:min((b % bpr + 1) * brows, rrows)]
        part[:, b, 0] = t.sum(1)
        part[:, b, 1] = ((t - t.mean(1, keepdim=True)) ** 2).sum(1)
    xs, bg, pg = x.to(dev), beta.to(dev), part.float().reshape(-1).to(dev)
    y = torch.zeros(rows, c, device=dev)
    mean, rstd = abi.empty(groups * c), abi.empty(groups * c)
    abi.lib.bn_act_fwd_partials(_p(xs), _p(bg), _p(pg), nblk, brows, rrows, _p(y), _p(mean), _p(rstd), rows, c, c, c, groups, 1e-3, ACT[act], 0.2,
                                L.dtype2(L.ACG_F32, L.ACG_F32), abi.stream())
    abi.sync()
    close(y, y_ref, TOL, tag + ' y')
    close(mean, mean_ref, TOL, tag + ' mean'); close(rstd, rstd_ref, TOL, tag + ' rstd')


# ---- pad channels: "neither read nor written" (acgan_hip.h) --------------------------------------------------------------------
# (name, R, C, pitch, groups, flags, forward path, backward path, storage).  C = 5 cannot take a grid kernel (V = 1).
PAD_ROWS = [
    ('pad12_resident', 300, 12, 16, 2, 0, RES, RES),
    ('pad12_grid512', 2049, 12, 16, 1, 0, grid(512), grid(512)),
    ('pad12_two', 2049, 12, 16, 2, L.BN_NO_GRID_EXCHANGE, TWO, TWO),
    ('pad5_resident', 300, 5, 8, 2, 0, RES, RES),
    ('pad5_two', 2100, 5, 8, 1, 0, TWO, TWO),
]
PAD_CASES = [(r[0], st) for r in PAD_ROWS for st in ('f32', 'bf16')]


def case_bn_pads(abi, name, storage, check_path=True):
    """Rows pitched wider than C.  The pad channels of x and dy hold NaN: every result must be finite and right (a pad that is
    read poisons a sum).  The pad channels of y and dx start at SENTINEL and must still hold it (zero-initialised pads cannot
    tell `not written` from `written with zero`); one row of sentinels before and after each tensor must survive too."""
    i, (_, R, c, cp, groups, flags, fpath, bpath) = next((i, r) for i, r in enumerate(PAD_ROWS) if r[0] == name)
    dev = abi.device
    rows = R * groups
    half = storage == 'bf16'
    tt = torch.bfloat16 if half else torch.float32
    act, acc, seed = 'lrelu', 0.5, 5000 + 16 * i
    x = kink_free(R, c, groups, seed).float()
    beta = (torch.rand(c, generator=_rng(seed + 1), dtype=torch.float64) * 0.5 - 0.25).float()
    dy = randn((rows, c), seed + 2)
    x, dy = (r16(x), r16(dy)) if half else (x, dy)
    tag = 'bn pads %s %s' % (name, storage)
    y_ref, mean_ref, rstd_ref, dx_ref, db_ref = reference(x, beta, dy, act, groups, tag)
    xs, dys = _store(x, cp, tt, dev, pad=float('nan')), _store(dy, cp, tt, dev, pad=float('nan'))
    lead = cp                                                   # one row of sentinels in front (keeps the 16-byte alignment)
    ybuf, yv = _guarded(torch.full((rows * cp,), SENTINEL, dtype=tt), lead, dev)
    dbuf, dv = _guarded(torch.full((rows * cp,), SENTINEL, dtype=tt), lead, dev)
    prev = randn((c,), seed + 3, max(float(db_ref.abs().mean()), 1e-3))
    abi.bn_flags = flags
    try:
        y, mean, rstd, ws = abi.bn_act_fwd(xs, beta.to(dev), act, groups, c=c, y=yv.view(rows, cp), want_ws=True)
        abi.sync()
        if check_path:
            _expect(fpath, ws, R, c, groups, tag + ' forward')
        close(y[:, :c].float(), y_ref, TOL16 if half else TOL, tag + ' y')
        close(mean, mean_ref, TOL, tag + ' mean'); close(rstd, rstd_ref, TOL, tag + ' rstd')
        assert bool((y[:, c:] == SENTINEL).all()), tag + ': pad channels of y were written'
        _guards_intact(ybuf, lead, tag + ' y')
        dx, dbeta, ws = abi.bn_act_bwd(xs, dys, beta.to(dev), mean_ref.float().to(dev), rstd_ref.float().to(dev), act, groups,
                                       dbeta=prev.clone().to(dev), accumulate=acc, c=c, dx=dv.view(rows, cp), want_ws=True)
        abi.sync()
        if check_path:
            _expect(bpath, ws, R, c, groups, tag + ' backward')
        close(dx[:, :c].float(), dx_ref, TOL16 if half else 4 * TOL, tag + ' dx')
        close(dbeta, acc * prev.double() + db_ref, 2e-4 if half else 4 * TOL, tag + ' dbeta')
        assert bool((dx[:, c:] == SENTINEL).all()), tag + ': pad channels of dx were written'
        _guards_intact(dbuf, lead, tag + ' dx')
    finally:
        abi.bn_flags = 0


# ---- accumulate on the neighbours ----------------------------------------------------------------------------------------------
def three_runs(run, prev, ref, tol, tag, dev):
    """``run(dbeta, accumulate) -> (dx or None, dbeta)`` three times on the same inputs: accumulate 0 into NaN (the output must
    not be read), 1 and 0.5 into ``prev``; each against accumulate * prev + ref, dx bit-identical across the three."""
    first = None
    for acc in ACCUMULATE:
        start = torch.full_like(prev, float('nan')) if acc == 0 else prev.clone()
        dx, got = run(start.to(dev), acc)
        close(got, (acc * prev.double() if acc else 0.0) + ref.double().cpu(), tol, tag + ' accumulate %g' % acc)
        if dx is not None:
            if first is None:
                first = dx.clone()
            else:
                assert torch.equal(dx, first), tag + ' accumulate %g: dx differs from the run with accumulate 0' % acc


def case_slab_accumulate(abi, tol, quads):
    """acg_bn_act_bwd_slabs on the HANDOFF_LAYERS tensors, accumulate 0 / 1 / 0.5: rows slabs into the one-launch grid kernels, or
    (``quads``: ACG_BN_NO_GRID_EXCHANGE) quad slabs into the register-resident ones.  dbeta reference as in case_slab_handoff:
    acg_bn_act_bwd on the separately reduced input gradient."""
    dev = abi.device
    done = 0
    abi.bn_flags = L.BN_NO_GRID_EXCHANGE if quads else 0
    try:
        for i, (xs, ws_, stride, padding, transposed, groups, act) in enumerate(C.HANDOFF_LAYERS):
            c = ws_[3]
            if transposed or c % 8:
                continue
            x, w = C.uniform(xs, 700 + i).to(dev), randn(ws_, 710 + i, 0.1).to(dev)
            beta = randn((c,), 720 + i, 0.5).to(dev)
            conv = abi.conv2d_fwd(x, w, stride, padding)
            if conv.shape[1] % 2:
                continue
            st = abi.to16(conv) if abi.half else conv
            _, mean, rstd = abi.bn_act_fwd(st, beta, act, groups=groups, c=c)
            w2 = randn((5, 5, c, 2 * c), 730 + i, 0.05).to(dev)
            dy2 = randn((conv.shape[0], conv.shape[1] // 2, conv.shape[2] // 2, 2 * c), 740 + i).to(dev)
            probe = abi.dgrad_bn_bwd_handoff(conv, beta, mean, rstd, act, dy2, w2, 2, 'SAME', groups, want_ws=True)
            if probe is None:
                continue
            layout, bws = probe[2], probe[3]
            tag = 'slab accumulate layer %d layout %d' % (i, layout)
            if abi.device.type == 'cuda':
                assert layout == (L.SLABS_QUADS if quads else L.SLABS_ROWS), tag + ': acg_bn_slabs_layout asked for the other layout'
                fam = bn_path(bws)[0]
                assert fam == ('resident' if quads else 'grid'), '%s: the %s kernels ran - the %s path lost this case' % (tag, fam, 'resident' if quads else 'grid')
            dyb = abi.conv2d_dgrad(dy2, w2, tuple(conv.shape), 2, 'SAME')
            xs_, dys_ = (abi.to16(conv), abi.to16(dyb)) if abi.half else (conv, dyb)
            _, db_ref = abi.bn_act_bwd(xs_, dys_, beta, mean, rstd, act, groups=groups)
            prev = randn((c,), 750 + i, max(float(db_ref.abs().mean()), 1e-3))

            def run(dbeta, acc):
                dx, dbeta, _ = abi.dgrad_bn_bwd_handoff(conv, beta, mean, rstd, act, dy2, w2, 2, 'SAME', groups, dbeta=dbeta, accumulate=acc)
                return dx, dbeta
            three_runs(run, prev, db_ref, 2e-3 if abi.half else tol * 8, tag, dev)
            done += 1
    finally:
        abi.bn_flags = 0
    assert done >= 2, 'slab accumulate: %d layers took the hand-off' % done


def case_bias_accumulate(abi, tol):
    """acg_bias_act_bwd, accumulate 0 / 1 / 0.5: one partial block, a count that leaves row lanes of colsum_finalize ragged, and
    the cap of 512 partial blocks (partial_blocks: rows / (8 * rows per pass)); dx NULL; float32 y from bf16 x (HIP only)."""
    dev = abi.device
    acts = {'tanh': torch.tanh, 'relu': C.T.relu, 'lrelu': C.T.lrelu, None: lambda t: t}
    for rows, c, act, want_dx, nblk in [(30, 7, 'lrelu', True, 1), (1000, 25, 'relu', True, 12), (4100, 300, 'tanh', True, 512), (1000, 25, None, False, 12)]:
        cb = min(c, 256)
        assert min(max(rows // (256 // cb * 8), 1), 512) == nblk, 'test premise: partial blocks of bias_act_bwd (bn.hip partial_blocks)'
        x, bias = randn((rows, c), 1700), randn((c,), 1701, 0.5)
        xd, bd = x.double().requires_grad_(True), bias.double().requires_grad_(True)
        dy = randn((rows, c), 1702)
        dx_ref, db_ref = torch.autograd.grad(acts[act](xd + bd), [xd, bd], dy.double())
        y = abi.bias_act_fwd(x.to(dev), bias.to(dev), act)
        tag = 'bias accumulate %d x %d %s%s' % (rows, c, act, '' if want_dx else ' (dx NULL)')
        prev = randn((c,), 1703, float(db_ref.abs().mean()))

        def run(dbias, acc):
            dx, dbias = abi.bias_act_bwd(y, dy.to(dev), act, want_dx=want_dx, dbias=dbias, accumulate=acc)
            if dx is not None:
                close(dx, dx_ref, tol * 4, tag + ' dx')
            return dx, dbias
        three_runs(run, prev, db_ref, tol * 4, tag, dev)
    if dev.type != 'cuda':
        return
    for rows, c, act in [(512, 3, 'tanh'), (700, 5, None)]:
        x, bias = r16(randn((rows, c), 1710)), randn((c,), 1711, 0.5)
        xd, bd = x.double().requires_grad_(True), bias.double().requires_grad_(True)
        dy = randn((rows, c), 1712)
        dx_ref, db_ref = torch.autograd.grad(acts[act](xd + bd), [xd, bd], dy.double())
        y = abi.bias_act_fwd(_store(x, 8, torch.bfloat16, dev), bias.to(dev), act, c=c, y_dtype=torch.float32)
        tag = 'bias accumulate bf16 x -> float32 y %d x %d %s' % (rows, c, act)
        prev = randn((c,), 1713, float(db_ref.abs().mean()))

        def run16(dbias, acc):
            dx, dbias = abi.bias_act_bwd(y, dy.to(dev), act, x_pitch=8, x_dtype=torch.bfloat16, dbias=dbias, accumulate=acc)
            close(dx[..., :c].float(), dx_ref, TOL16, tag + ' dx')
            return dx, dbias
        three_runs(run16, prev, db_ref, 1e-4, tag, dev)


# (B, H, W, C, k, partial rows): both kernel families (k < 6: 64 x 4 pixel tiles; k >= 6: one block per 64 pixels of a row) on both
# sides of the 1024 partial rows from which dna_bwd sums dbias in two stages, and the switch point itself: 1024 rows are the last
# one-stage launch, 1025 the first two-stage one (33 rows per segment: the last of the 32 segments holds 2)
DNA_ACC_SHAPES = [(2, 7, 5, 3, 5, 4), (130, 32, 3, 3, 5, 1040), (1, 9, 70, 3, 7, 18), (50, 21, 5, 1, 6, 1050),
                  (16, 64, 3, 1, 6, 1024), (25, 41, 2, 1, 7, 1025)]


def case_dna_accumulate(abi, shape, tol, half):
    b, h, w, c, k, nblk = shape
    assert nblk == (-(-w // 64) * (h if k >= 6 else -(-h // 4)) * b), 'test premise: dbias partial rows (dna.hip dna_grid)'
    kk, dev = k * k, abi.device
    logits = randn((b, h, w, kk), 1800, 2.0)
    logits = r16(logits) if half else logits
    bias, img = randn((kk,), 1803, 1.0), C.uniform((b, h, w, c), 1801)
    ld, bd = logits.double().requires_grad_(True), bias.double().requires_grad_(True)
    out_ref = C.T.dna_gather(ld + bd, img.double(), k)
    dout = randn(tuple(out_ref.shape), 1802)
    dl_ref, db_ref = torch.autograd.grad(out_ref, [ld, bd], dout.double())
    lg = logits.to(dev)
    if half:
        lg = torch.zeros(b, h, w, (kk + 7) // 8 * 8, dtype=torch.bfloat16, device=dev)
        lg[..., :kk] = logits.to(dev).to(torch.bfloat16)
    tag = 'dna accumulate %s %s' % (shape, 'bf16' if half else 'f32')
    prev = randn((kk,), 1804, float(db_ref.abs().mean()))

    def run(dbias, acc):
        dl, dbias = abi.dna_bwd(lg, img.to(dev), dout.to(dev), k, bias=bias.to(dev), dbias=dbias, accumulate=acc)
        close(dl[..., :kk].float(), dl_ref, TOL16 if half else tol * 4, tag + ' dlogits')
        return dl, dbias
    three_runs(run, prev, db_ref, TOL16 if half else tol * 8, tag, dev)
