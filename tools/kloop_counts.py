#!/usr/bin/env python3
"""Instruction counts of the conv K-loops out of a cross-compiled .s (hipcc --offload-arch=gfx950 --cuda-device-only -S).

For every kernel whose mangled name contains one of the given substrings: registers, LDS, scratch and occupancy from the
kernel's resource comments, and for every barrier-to-barrier segment that holds 16 MFMAs (one unrolled K-step): VALU (v_* other
than v_mfma), VMEM (buffer_load), LDS (ds_*), SALU (s_* other than waits, barriers, branches and nops), the labels and branches
inside the segment (a K-step that is one basic block has no label and at most the loop-exit branch) and its `s_waitcnt vmcnt`
values.  `w2` counts the two-dword LDS stores (ds_write2_b32: the transposed half quads, issued from inline assembly, which the
compiler's wait counting does not see); `ordered` says whether an `s_waitcnt lgkmcnt(0)` stands between the last of them and the
segment's barrier.  The line `w2 segments` holds the same for EVERY barrier-to-barrier segment of the kernel, prologue included.  `side` is the part of VALU that sits in the segment's first s_and_saveexec region (up to the label its s_cbranch_execz
names): the generic weight gradient's row-table refill, which is in every unrolled copy but runs once per 8 K-steps.

    python3 tools/kloop_counts.py wgrad.s conv_mfma_f32ILi2ELi64ELi64
"""
import re
import sys


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line)
            if line.startswith('; Occupancy'):      # the last of the resource comments behind .Lfunc_end
                yield name, body
                name = None


def segments(body):
    seg = []
    for line in body:
        t = line.strip()
        if not t or t.startswith(';') or t.startswith('.') and not re.match(r'^\.LBB\w+:', t):
            continue
        seg.append(t.split(";")[0].strip())
        if t.startswith('s_barrier'):
            yield seg
            seg = []


def count(seg):
    c = dict(mfma=0, valu=0, valu_side=0, vmem=0, lds=0, salu=0, labels=0, branches=0, vmcnt=[], w2=0, ordered=True)
    first = next((i for i, t in enumerate(seg) if t.startswith('s_and_saveexec')), None)
    if first is not None:
        m = next((re.match(r's_cbranch_execz\s+(\.LBB\w+)', t) for t in seg[first:] if t.startswith('s_cbranch_execz')), None)
        end = seg.index(m.group(1) + ':') if m and (m.group(1) + ':') in seg else first
        c['valu_side'] = sum(1 for t in seg[first:end] if t.startswith('v_') and not t.startswith('v_mfma'))
    for t in seg:
        op = t.split()[0]
        if re.match(r'^\.LBB\w+:', t):
            c['labels'] += 1
        elif op.startswith('v_mfma'):
            c['mfma'] += 1
        elif op.startswith('v_'):
            c['valu'] += 1
        elif op.startswith('buffer_') or op.startswith('global_') or op.startswith('flat_'):
            c['vmem'] += 1
        elif op.startswith('ds_'):
            c['lds'] += 1
            if op == 'ds_write2_b32':
                c['w2'] += 1
                c['ordered'] = False
        elif op.startswith('s_cbranch') or op == 's_branch':
            c['branches'] += 1
        elif op == 's_waitcnt':
            m = re.search(r'vmcnt\((\d+)\)', t)
            if m:
                c['vmcnt'].append(int(m.group(1)))
            if 'lgkmcnt(0)' in t:
                c['ordered'] = True
        elif op.startswith('s_') and op not in ('s_barrier', 's_nop', 's_endpgm', 's_sleep'):
            c['salu'] += 1
    return c


def main():
    path, keys = sys.argv[1], sys.argv[2:]
    for name, body in kernels(path):
        if keys and not any(k in name for k in keys):
            continue
        text = ''.join(body)
        res = {k: re.search(r'; %s: (\d+)' % k, text) for k in ('NumVgprs', 'TotalNumSgprs', 'ScratchSize', 'Occupancy')}
        lds = re.search(r'; LDSByteSize: (\d+)', text)
        print(name)
        print('  vgpr %s sgpr %s scratch %s lds %s occupancy %s' % tuple([res[k].group(1) if res[k] else '?' for k in ('NumVgprs', 'TotalNumSgprs', 'ScratchSize')]
                                                                        + [lds.group(1) if lds else '?', res['Occupancy'].group(1) if res['Occupancy'] else '?']))
        every = list(map(count, segments(body)))
        steps = [c for c in every if c['mfma'] == 16]
        for i, c in enumerate(steps):
            print('  K-step %d: valu %3d (side %3d) vmem %2d lds %2d salu %3d labels %d branches %d vmcnt %s w2 %d%s' % (
                i, c['valu'], c['valu_side'], c['vmem'], c['lds'], c['salu'], c['labels'], c['branches'], c['vmcnt'], c['w2'],
                '' if not c['w2'] else (' ordered' if c['ordered'] else ' NOT ORDERED')))
        w2 = [c for c in every if c['w2']]
        if w2:
            print('  w2 segments: %d, ordered before their barrier: %d' % (len(w2), sum(1 for c in w2 if c['ordered'])))
        if steps:
            n = float(len(steps))
            print('  mean of %d: valu %.1f vmem %.1f salu %.1f' % (len(steps), sum(c['valu'] for c in steps) / n, sum(c['vmem'] for c in steps) / n,
                                                                 sum(c['salu'] for c in steps) / n))


if __name__ == '__main__':
    main()
