#!/usr/bin/env python
"""Registers, scratch, LDS and occupancy of every kernel of two builds, side by side, from the compiler's own remarks.

  make -C action_conditioned_gans_amd/csrc -O -j8 CXXFLAGS="<the Makefile's flags> -Rpass-analysis=kernel-resource-usage" 2> build.log
  python tools/resource_usage_diff.py PARENT.log PR.log [--kernels REGEX] > profiles/<topic>/resource_usage.txt

(-O: make keeps the output of one compilation together; the remarks of parallel compilations must not interleave.)

Needs no GPU.  Exit status 1 if the two builds do not hold the same kernels, or a kernel of the second build has scratch, another
LDS size or fewer waves per SIMD than in the first."""
import argparse
import re
import subprocess
import sys

FIELDS = {'VGPRs': 'vgpr', 'AGPRs': 'agpr', 'ScratchSize [bytes/lane]': 'scratch', 'Occupancy [waves/SIMD]': 'waves', 'LDS Size [bytes/block]': 'lds'}


def parse(path, pattern):
    kernels, cur = {}, None
    for line in open(path, errors='replace'):
        m = re.match(r'(\S+?):\d+:\d+: remark:\s+(.*?) \[-Rpass-analysis', line)
        if not m:
            continue
        src, text = m.group(1).split('/')[-1], m.group(2)
        if text.startswith('Function Name: '):
            name = text[len('Function Name: '):]
            cur = kernels.setdefault((src, name), {}) if re.search(pattern, name) else None
        elif cur is not None:
            key, _, val = text.partition(': ')
            if key.strip() in FIELDS:
                cur[FIELDS[key.strip()]] = int(val)
    return kernels


def short(name):
    try:
        name = subprocess.run(['c++filt', name], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    except (OSError, subprocess.CalledProcessError):
        pass
    return re.sub(r'^void acgconv::', '', name).split('(')[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parent')
    ap.add_argument('pr')
    ap.add_argument('--kernels', default='conv_(mfma|pair|glds)_', help='regular expression a (mangled) kernel name must contain')
    args = ap.parse_args()
    a, b = parse(args.parent, args.kernels), parse(args.pr, args.kernels)
    bad = 0
    if set(a) != set(b):
        bad += 1
        print('DIFFERENT KERNELS: only parent %s; only pr %s' % (sorted(set(a) - set(b)), sorted(set(b) - set(a))))
    print('# %d kernels; VGPRs, waves/SIMD, LDS bytes and scratch bytes/lane, parent -> pr' % len(b))
    for key in sorted(set(a) & set(b)):
        x, y = a[key], b[key]
        ok = y['scratch'] == 0 and y['lds'] == x['lds'] and y['waves'] >= x['waves']
        bad += not ok
        print('%-22s %-95s vgpr %3d -> %3d  waves %d -> %d  lds %6d -> %6d  scratch %d -> %d  %s' % (
            key[0], short(key[1]), x['vgpr'], y['vgpr'], x['waves'], y['waves'], x['lds'], y['lds'], x['scratch'], y['scratch'], 'ok' if ok else 'NOT MET'))
    both = sorted(set(a) & set(b))
    print('# max VGPRs %d -> %d; kernels with more VGPRs: %d, with fewer: %d; %s' % (
        max(a[k]['vgpr'] for k in both), max(b[k]['vgpr'] for k in both), sum(b[k]['vgpr'] > a[k]['vgpr'] for k in both),
        sum(b[k]['vgpr'] < a[k]['vgpr'] for k in both), 'all conditions met' if not bad else '%d conditions NOT met' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
