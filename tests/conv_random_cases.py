"""A seeded random sample of the convolution descriptor space: the rows nobody picked by hand (the sibling of conv_path_cases.py,
whose table has one directed shape per kernel variant).

``rows()`` returns conv_path_cases.Row entries with an EMPTY ``expect``: a random row has no premise.  The tests ask the planner what
the row reaches (acg_conv2d_path / acg_conv2d_pair_path) and run that: test_conv_random_cpu.py on the host build of the planner and
on the C oracle, test_gpu_conv_random.py on the GPU.

The sample is a list of QUOTAS followed by free draws.  A quota row is a free draw with some fields forced, so that the classes a
uniform draw reaches by luck at best are there BY CONSTRUCTION (``classes_of`` says which classes a row is in; the CPU test counts
them): degenerate geometries - a 1 x 1 image, a filter larger than the image, a one-pixel output extent, a stride larger than the
filter (whole stride classes of the input gradient receive no tap and must come back as zeros), an even filter under stride 3,
one channel, batch 1 - a channel limit on an input gradient that splits, and the planner's thin corners: the non-LIN dense forward
(few channels at a padded pitch), compact tiles, the merged input gradient.

Every descriptor is valid as acgan_hip.h defines it (``valid`` mirrors validate() of conv_f32.hip; the CPU test holds it against the
planner itself).  bf16 rows carry no explicit pitches (conv_path_cases.desc_of).  A channel limit is dgrad_c on a conv row and
adj_dgrad_c on a transposed row: the header reserves each for that entry.

The printed table's SHA-256 is DIGEST below.  random.Random's integer and float draws are stable across Python 3 versions, and the
CPU test compares the digest, so the sample cannot drift with an interpreter or an innocent edit: whoever changes the distribution,
a quota or the seed changes DIGEST on purpose - and then the coverage conditions of test_conv_random_cpu.py say whether the new
sample still reaches what the old one did.

Run as a script, this file prints the sample as the queries tools/conv_path_sweep.hip reads."""
import hashlib
import random

import conv_path_cases as P

SEED = 20261021
N = 400
# The cost cap of a row, 2 * batch * out_h * out_w * kh * kw * in_c * out_c.  Chosen for the GPU test: a chunk of CHUNK rows - each
# row about 30 small launches with a synchronisation, a float64 reference on the CPU and sentinel scans after each - has to stay
# at a few seconds, and for the C oracle (three nested loops in double precision), which runs every fp32 row in the CPU suite.
# profiles/conv_random/figures.txt has the measured chunk times.
MAX_FLOP = 48e6
CHUNK = 25
PAIR_FLAGS = (0, 1, 2)

CHANNELS = (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 25, 32, 33, 36, 37, 40, 41, 48, 64, 65, 72, 96, 128)

DIGEST = '1b7ff94305cc1700618f30797de3680c1b7732943cac7fc8509ed9743d18a217'


def valid(desc):
    """validate() of conv_f32.hip on the 17 fields."""
    b, h, w, cin, oh, ow, cout, kh, kw, sh, sw, pt, pl, ip, op, dc, adc = desc
    return (min(b, h, w, cin, oh, ow, cout, kh, kw, sh, sw) > 0 and pt >= 0 and pl >= 0 and (ip == 0 or ip >= cin) and (op == 0 or op >= cout)
            and 0 <= dc <= cin and 0 <= adc <= cout and kh * kw <= 64 and pt < kh and pl < kw
            and (oh - 1) * sh - pt < h and (ow - 1) * sw - pl < w)


def _pitch(rng, c):
    """A padded channel pitch: the next multiples of 4 (16-byte gathers stay possible), or any pitch up to 7 beyond the count."""
    return (c // 4 + rng.randint(1, 2)) * 4 if rng.random() < 0.5 else c + rng.randint(1, 7)


def _draw(rng):
    """One free draw: every field of a row, as a dict.  All random numbers of a row are drawn here, whatever a quota forces later."""
    f = dict(b=rng.randint(1, 16), h=rng.randint(1, 40), w=rng.randint(1, 40), cin=rng.choice(CHANNELS), cout=rng.choice(CHANNELS))
    f['kh'] = rng.randint(1, 7)
    kw = rng.randint(1, 7)
    f['kw'] = kw if rng.random() < 0.5 else f['kh']
    f['sh'] = rng.randint(1, 3)
    sw = rng.randint(1, 3)
    f['sw'] = sw if rng.random() < 0.4 else f['sh']
    u = rng.random()
    f['pad'] = 'SAME' if u < 0.5 else ('VALID' if u < 0.7 else 'explicit')
    f['pads'] = tuple(rng.random() for _ in range(4))      # explicit padding as fractions of the filter extent: scaled once kh, kw are final
    f['transposed'] = rng.random() < 0.4
    f['storage'] = 'bf16' if rng.random() < 0.25 else 'f32'
    f['in_pitch'] = rng.random() < 0.3
    f['out_pitch'] = rng.random() < 0.3
    f['limit'] = rng.random() < 0.2
    f['u'] = tuple(rng.random() for _ in range(8))          # spare numbers for the quotas and the limit
    f['rng'] = random.Random(rng.getrandbits(32))           # and a generator of the row's own for the pitches
    return f


def _row(name, why, f):
    """The Row of a draw, or None where the draw is no valid descriptor or costs more than MAX_FLOP."""
    kh, kw = f['kh'], f['kw']
    if f['pad'] == 'VALID':
        kh, kw = min(kh, f['h']), min(kw, f['w'])
    pad = f['pad']
    if pad == 'explicit':
        pad = tuple(int(x * k) for x, k in zip(f['pads'], (kh, kh, kw, kw)))
        if f['h'] + pad[0] + pad[1] < kh or f['w'] + pad[2] + pad[3] < kw:
            return None
    cin, cout, half, rng = f['cin'], f['cout'], f['storage'] != 'f32', f['rng']
    kw_ = {}
    if not half:
        if f['in_pitch']:
            kw_['in_pitch'] = f['in_pitch'] if f['in_pitch'] is not True else _pitch(rng, cin)
        if f['out_pitch']:
            kw_['out_pitch'] = f['out_pitch'] if f['out_pitch'] is not True else _pitch(rng, cout)
    if f['limit']:
        c = cout if f['transposed'] else cin
        lim = f['limit'] if f['limit'] is not True else 1 + int(f['u'][0] * (c - 1))
        if c > 1:
            kw_['adj_dgrad_c' if f['transposed'] else 'dgrad_c'] = min(lim, c - 1)
    desc = P.conv(f['b'], f['h'], f['w'], cin, cout, kh, kw, f['sh'], f['sw'], pad, **kw_)
    r = P.row(name, why, desc, {}, transposed=f['transposed'], storage=f['storage'])
    if not valid(desc) or P.flop(r) > MAX_FLOP:
        return None
    return r


def _pick(u, seq):
    return seq[int(u * len(seq))]


# ---- the quotas: (tag, rows, what it is there for, force(draw, i) -> None) ---------------------------------------------------------
def _img1(f, i):
    f.update(h=1, w=1)
    if f['pad'] == 'VALID' and i % 2:
        f['pad'] = 'SAME'


def _big_filter(f, i):
    f.update(pad='SAME', h=1 + int(f['u'][1] * 5), w=1 + int(f['u'][2] * 5))
    f.update(kh=f['h'] + 1 + int(f['u'][3] * (6 - f['h'])), kw=f['w'] + 1 + int(f['u'][4] * (6 - f['w'])))


def _out1(f, i):
    a, o = ('h', 'w') if i % 2 else ('w', 'h')
    if i % 4 < 2:      # SAME under a stride that is at least the extent
        f.update(pad='SAME', **{a: 1 + int(f['u'][1] * 3), 's' + a: 3})
    else:              # VALID with the filter as large as the image
        f.update(pad='VALID', **{a: f['k' + a]})
    f[o] = max(f[o], 2 * f['s' + o] + f['k' + o])


def _stride_gt_filter(f, i):
    a = 'h' if i % 2 else 'w'
    f['s' + a] = 2 + int(f['u'][1] * 2)
    f['k' + a] = 1 + int(f['u'][2] * (f['s' + a] - 1))
    if i % 3 == 0:
        f.update(sh=f['s' + a], sw=f['s' + a], kh=f['k' + a], kw=f['k' + a])
    f.update(h=max(f['h'], 4), w=max(f['w'], 4))


def _even_s3(f, i):
    k = _pick(f['u'][1], (2, 4, 6))
    f.update(kh=k, sh=3, h=max(f['h'], 5))
    if i % 2:
        f.update(kw=_pick(f['u'][2], (2, 4, 6)), sw=3, w=max(f['w'], 5))


def _limit_split(f, i):
    """A channel limit on an input gradient that splits: few tiles (a small map) under a long K (64 channels or more on the gathered side)."""
    f.update(storage='f32' if i % 3 else 'bf16', b=1 + i % 2, h=4 + int(f['u'][1] * 5), w=4 + int(f['u'][2] * 5), kh=3 + 2 * (i % 2), kw=3, sh=1, sw=1, pad='SAME')
    gathered, other = _pick(f['u'][3], (64, 72, 96, 128)), _pick(f['u'][4], (24, 37, 40, 42, 65))
    if f['transposed']:      # its input gradient is the descriptor's FWD: in_c channels gathered, adj_dgrad_c of out_c computed
        f.update(cin=gathered, cout=other)
    else:
        f.update(cin=other, cout=gathered)
    f['limit'] = max(1, int(other * (0.3 + 0.6 * f['u'][5])))


def _dense_nonlin(wide):
    def force(f, i):
        """The descriptor's FWD, float4-able on both sides, with a gathered channel count that is no multiple of 4."""
        cin = _pick(f['u'][1], (1, 2, 3, 5, 6, 7))
        f.update(storage='f32', transposed=i % 3 == 2, cin=cin, in_pitch=(cin // 4 + 1 + i % 2) * 4, limit=False, out_pitch=False,
                 cout=_pick(f['u'][2], (36, 40, 64, 72) if wide else (12, 16, 24, 32)), b=max(f['b'], 2), h=max(f['h'], 6), w=max(f['w'], 6))
    return force


def _compact(f, i):
    f.update(storage='f32', b=8 + int(f['u'][1] * 9), h=1 + int(f['u'][2] * 4), w=1 + int(f['u'][3] * 4), sh=2, sw=2, pad='SAME',
             kh=max(f['kh'], 2), kw=max(f['kw'], 2), cin=_pick(f['u'][4], (16, 32, 36, 64)), cout=_pick(f['u'][5], (16, 40, 64, 72)))


def _merged(f, i):
    k = 3 + int(f['u'][1] * 5)
    f.update(transposed=False, h=2 * (2 + int(f['u'][2] * 8)), w=2 * (2 + int(f['u'][3] * 8)), sh=2, sw=2, kh=k, kw=k if i % 2 else 3 + int(f['u'][4] * 5),
             pad='SAME', cin=_pick(f['u'][5], (3, 4, 5, 6, 8)), cout=_pick(f['u'][6], (16, 24, 33, 64)), limit=False, b=max(f['b'], 2))


def _uniform_fwd(f, i):
    """The descriptor's FWD as a LIN contraction that gathers a multiple of the 32-channel K-step (every fourth row at a padded pitch)."""
    cin = _pick(f['u'][1], (32, 64, 96, 128))
    f.update(storage='f32', cin=cin, cout=_pick(f['u'][2], (12, 16, 24, 32, 40, 64, 72)), in_pitch=cin + 8 if i % 4 == 3 else False, out_pitch=False,
             limit=False, h=max(f['h'], 3), w=max(f['w'], 3))


QUOTAS = [
    ('img1x1', 6, 'a 1 x 1 image', _img1),
    ('bigfilter', 6, 'a filter larger than the image in both directions, SAME padding', _big_filter),
    ('out1', 8, 'an output extent of 1 in one direction only', _out1),
    ('stridegtk', 8, 'a stride larger than the filter: stride classes without a tap', _stride_gt_filter),
    ('evens3', 8, 'an even filter under stride 3', _even_s3),
    ('cin1', 6, 'one input channel', lambda f, i: f.update(cin=1)),
    ('cout1', 6, 'one output channel', lambda f, i: f.update(cout=1)),
    ('batch1', 6, 'batch 1', lambda f, i: f.update(b=1)),
    ('limitsplit', 9, 'a channel limit on an input gradient that splits', _limit_split),
    ('nonlin_narrow', 6, 'the non-LIN dense forward on the 128x32 tile: few channels at a padded pitch', _dense_nonlin(False)),
    ('nonlin_wide', 6, 'the non-LIN dense forward on the 64x64 tile', _dense_nonlin(True)),
    ('compact', 6, 'compact tiles: batch 8 or more on a map of at most 2 x 2 output pixels', _compact),
    ('merged', 6, 'the merged input gradient of a stride-2 layer with few input channels', _merged),
    ('uniformfwd', 8, 'a forward contraction that takes the uniform_k loaders', _uniform_fwd),
]


def rows(seed=SEED, n=N):
    """The sample: the quotas, then free draws, ``n`` rows in all.  Deterministic in (seed, n); random.Random only."""
    rng = random.Random(seed)
    out = []

    def add(tag, why, force, i):
        while True:      # rejection: a draw that is no valid descriptor, or costs too much, is drawn again
            f = _draw(rng)
            if force is not None:
                force(f, i)
            r = _row('r%03d_%s' % (len(out), tag), why, f)
            if r is not None:
                out.append(r)
                return

    for tag, count, why, force in QUOTAS:
        for i in range(count):
            if len(out) < n:
                add(tag, why, force, i)
    while len(out) < n:
        add('free', 'a free draw', None, 0)
    return out


def classes_of(r):
    """The by-construction classes a row is in, from its descriptor alone ('limit': a channel limit is set - whether the input gradient
    splits is the planner's answer, which the CPU test adds)."""
    b, h, w, cin, oh, ow, cout, kh, kw, sh, sw, pt, pl, ip, op, dc, adc = r.desc
    same = oh == -(-h // sh) and ow == -(-w // sw) and pt == max((oh - 1) * sh + kh - h, 0) // 2 and pl == max((ow - 1) * sw + kw - w, 0) // 2
    out = set()
    for name, yes in (('img1x1', h == 1 and w == 1), ('bigfilter', same and kh > h and kw > w), ('out1', (oh == 1) != (ow == 1)),
                      ('stridegtk', sh > kh or sw > kw), ('evens3', (sh == 3 and kh % 2 == 0) or (sw == 3 and kw % 2 == 0)),
                      ('cin1', cin == 1), ('cout1', cout == 1), ('batch1', b == 1), ('limit', dc > 0 or adc > 0)):
        if yes:
            out.add(name)
    return out


def chunks(rs=None, size=CHUNK):
    rs = rows() if rs is None else rs
    return [rs[i:i + size] for i in range(0, len(rs), size)]


def sweep_queries(rs=None):
    """The sample as the lines tools/conv_path_sweep.hip reads: the three contractions, the pair entry at PAIR_FLAGS, and the
    epilogue / statistics queries the GPU test takes its premises from."""
    out = []
    for r in (rows() if rs is None else rs):
        ints = ' '.join(str(v) for v in r.desc)
        for c in ('fwd', 'dgrad', 'wgrad'):
            out.append('path %s:%s %d %d 0 %s' % (r.name, c, P.which_of(r, c), P.dtype_of(r), ints))
        for flags in PAIR_FLAGS:
            out.append('pair %s %d %d %d %s' % (r.name, 1 if r.transposed else 0, P.dtype_of(r), flags, ints))
        if r.transposed:
            out.append('epi %s %d %s' % (r.name, P.dtype_of(r), ints))
        if r.storage == 'f32':
            out.append('stats %s %d %d 1 %s' % (r.name, P.which_of(r, 'fwd'), P.dtype_of(r), ints))
    return out


def digest(rs=None):
    return hashlib.sha256(('\n'.join(sweep_queries(rs)) + '\n').encode()).hexdigest()


PATH_INTS = ('tiles', 'classes', 'nk', 'splits', 'ragged', 'nvec', 'lin', 'compact', 'merged', 'nb', 'uk', 'uw')


def parse_answers(lines):
    """The output of conv_path_sweep for ``sweep_queries``: ('path', row, contraction) -> {field: value} or {'error': code};
    ('pair', row, flag word) -> kind; ('epi', row) -> 0 / 1; ('stats', row) -> blocks."""
    got = {}
    for line in lines:
        t = line.split()
        kv = dict(x.split('=') for x in t[2:] if '=' in x)
        if t[0] == 'path':
            name, c = t[1].rsplit(':', 1)
            if 'error' not in kv:
                kv.update({k: int(kv[k]) for k in PATH_INTS})
                kv['tile_rows'], kv['tile_cols'] = (int(v) for v in kv['tile'].split('x'))
            got['path', name, c] = kv
        elif t[0] == 'pair':
            got['pair', t[1], int(kv['flags'])] = kv['kind']
        else:
            got[t[0], t[1]] = int(kv['ok' if t[0] == 'epi' else 'blocks'])
    return got


def path_words(kv):
    """A parsed path answer as conv_path_cases.path_str writes an acg_conv_path."""
    from action_conditioned_gans_amd import _lib as L
    return P.path_str(dict(kv, family=L.ConvPath.FAMILIES.index(kv['family']), reduce=L.ConvPath.REDUCES.index(kv['reduce']), direct_nb=kv['nb']))


def variants_of(r, got):
    """The launch statements the planner's answers say a row reaches, one entry per launch: the kernel instantiation of each
    contraction as conv_path_cases._variant names it - with ' uk' / ' uw' where the uniform_k / uniform_w loaders are taken, ' split'
    where the plan splits - the reduction behind it, and 'pair <kind>' of the paired entry at flag word 0."""
    out = []
    for c in ('fwd', 'dgrad', 'wgrad'):
        kv = got['path', r.name, c]
        v = P._variant(r, c, path_words(kv))
        tags = [k for k in ('compact', 'merged', 'uk', 'uw') if kv[k]] + (['split'] if kv['splits'] > 1 else [])
        out += [' '.join([v[0]] + tags)] + v[1:]
    out.append('pair ' + got['pair', r.name, 0])
    return out


def histogram(rs, got):
    """'variant, then count', one line per launch statement the sample reaches, sorted by name."""
    import collections
    n = collections.Counter(v for r in rs for v in variants_of(r, got))
    return ''.join('%-60s %4d\n' % kv for kv in sorted(n.items()))


if __name__ == '__main__':
    import sys
    if sys.argv[1:] == ['--histogram']:      # ... tests/conv_random_cases.py | conv_path_sweep | ... tests/conv_random_cases.py --histogram
        sys.stdout.write(histogram(rows(), parse_answers(sys.stdin.read().splitlines())))
    elif sys.argv[1:] == ['--digest']:
        print(digest())
    else:
        print('\n'.join(sweep_queries()))
