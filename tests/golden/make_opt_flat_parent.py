"""Records tests/golden/opt_flat_parent.npz: what the flat optimizer kernels (acg_adam_step, acg_rmsprop_step) of the commit
BEFORE they were folded into one body leave after three steps, on a GPU.  tests/test_gpu_opt_flat.py holds the kernels of
the working tree to these bits: the other bit-for-bit tests compare the carried and the prepared launches with the flat ones,
which proves nothing if the flat ones drift themselves.

The file was recorded from a build of PARENT.  It is never re-recorded from the tree under test: check PARENT out somewhere
else, build it there, and name its library.  Usage (from the repo root, on a GPU):

    python tests/golden/make_opt_flat_parent.py --lib <checkout of PARENT>/action_conditioned_gans_amd/csrc/libacgan_hip.so
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

PARENT = '1ed83da95e6a9b9b3f9481c54a31d2f2dbc3f62c'
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'opt_flat_parent.npz')
N, STEPS = 1031, 3          # five blocks' worth of float4 and a scalar tail of three
CASES = [(kind, clip) for kind in ('adam', 'rmsprop') for clip in (False, True)]


def _f32(*values):
    return tuple(float(np.float32(v)) for v in values)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def inputs(kind, clip, device):
    gen = torch.Generator().manual_seed(N + 2 * CASES.index((kind, clip)))
    param = (torch.randn(N, generator=gen) * 0.02).to(device)
    grads = [(torch.randn(N, generator=gen) * 0.3).to(device) for _ in range(STEPS)]
    return param, grads


def run(lib, kind, clip, device='cuda:0'):
    """STEPS steps of one flat entry -> {'param', 'slot1'[, 'slot2']} as numpy float32."""
    param, grads = inputs(kind, clip, device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tail = _f32(0.5) + (1 if clip else 0,) + _f32(-0.01, 0.01)
    if kind == 'adam':
        m, v = torch.zeros(N, device=device), torch.zeros(N, device=device)
        step = torch.zeros(1, dtype=torch.int32, device=device)
        for t, g in enumerate(grads):
            step.fill_(t + 1)
            lib.adam_step(_p(param), _p(g), _p(m), _p(v), _p(step), N, *_f32(1e-3, 0.9, 0.999, 1e-8), *tail, stream)
        out = {'param': param, 'slot1': m, 'slot2': v}
    else:
        ms = torch.ones(N, device=device)
        for g in grads:
            lib.rmsprop_step(_p(param), _p(g), _p(ms), N, *_f32(5e-5, 0.9, 1e-10), *tail, stream)
        out = {'param': param, 'slot1': ms}
    return {k: t.cpu().numpy() for k, t in out.items()}


def key(kind, clip, name):
    return '%s/%s/%s' % (kind, 'clip' if clip else 'noclip', name)


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from action_conditioned_gans_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True, help='libacgan_hip.so built from a checkout of ' + PARENT)
    ap.add_argument('--out', default=PATH)
    args = ap.parse_args()
    if os.path.realpath(args.lib) == os.path.realpath(_lib.LIB_PATH):
        raise SystemExit('--lib is the library of this tree: the file pins the kernels of %s, not the code under test' % PARENT)
    lib = _lib.Library(args.lib, require=tuple(_lib.EXTENSIONS))
    out = {'parent': np.array(PARENT)}
    for kind, clip in CASES:
        for name, a in run(lib, kind, clip).items():
            out[key(kind, clip, name)] = a
    np.savez(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes from', args.lib)


if __name__ == '__main__':
    main()
