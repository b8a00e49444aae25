#!/usr/bin/env python3
"""Compare the device code of two builds of one .hip file, kernel by kernel, without a GPU.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only --no-gpu-bundle-output -c bn.hip -o a.elf      (once per tree)
    tools/bn_device_diff.py a.elf b.elf [--gone FILE]

For every kernel (a function symbol with a `.kd` descriptor) of either ELF: the disassembly with addresses stripped, the 64
descriptor bytes and the kernel's entry in the metadata note (registers, LDS, scratch, arguments).  Prints the kernels only one
side has, the kernels that differ, the .text sizes; exit status 1 when a kernel both sides have differs.  --gone FILE: the
kernels of a.elf that b.elf lacks, one mangled name per line (for a commit that removes instantiations on purpose)."""
import argparse
import re
import shutil
import subprocess
import sys

LLVM = '/opt/rocm/llvm/bin/'


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout


def kernels(elf):
    """name -> (text, descriptor, metadata), and the size of .text."""
    syms = run(LLVM + 'llvm-readelf', '-sW', elf)
    names = sorted(m.group(1)[:-3] for m in re.finditer(r'OBJECT\s+\S+\s+\S+\s+\S+\s+(\S+\.kd)\s*$', syms, re.M))
    text = {}
    cur = None
    for line in run(LLVM + 'llvm-objdump', '-d', '--no-show-raw-insn', elf).splitlines():
        m = re.match(r'^[0-9a-f]+ <(\S+)>:$', line)
        if m:
            cur = text.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            # "\ts_load_dword s0, s[4:5], 0x0   // 000000001000: ..." -> the instruction; branch targets keep their label + offset
            cur.append(re.sub(r'\s*//.*$', '', line).strip())
    rodata = run(LLVM + 'llvm-objdump', '-s', '-j', '.rodata', elf)
    blob = {}
    for line in rodata.splitlines():
        m = re.match(r'^\s*([0-9a-f]+)((?: [0-9a-f]{2,8}){1,4})\s', line)
        if m:
            data = bytes.fromhex(m.group(2).replace(' ', ''))
            for i, b in enumerate(data):
                blob[int(m.group(1), 16) + i] = b
    desc = {}
    for m in re.finditer(r'^\s*\d+:\s+([0-9a-f]+)\s+64\s+OBJECT\s+\S+\s+\S+\s+\S+\s+(\S+)\.kd\s*$', syms, re.M):
        a = int(m.group(1), 16)
        d = bytes(blob.get(a + i, 0) for i in range(64))
        desc[m.group(2)] = d[:16] + d[24:]          # bytes 16..23: the entry's offset from the descriptor - an address
    notes = run(LLVM + 'llvm-readelf', '--notes', elf)
    meta = {}
    for chunk in re.split(r'\n\s*- \.agpr_count:', notes)[1:]:
        m = re.search(r'\.name:\s+(\S+)', chunk)
        if m:
            meta[m.group(1)] = re.sub(r'\s+', ' ', chunk.split('\namdhsa.target')[0]).strip()
    size = int(re.search(r'\]\s+\.text\s+PROGBITS\s+\S+\s+\S+\s+([0-9a-f]+)', run(LLVM + 'llvm-readelf', '-SW', elf)).group(1), 16)
    return {n: ('\n'.join(text.get(n, [])), desc.get(n), meta.get(n)) for n in names}, size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--gone')
    args = ap.parse_args()
    (ka, sa), (kb, sb) = kernels(args.a), kernels(args.b)
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt', path=LLVM)
    demangle = lambda n: run(filt, n).strip() if filt else n
    gone, new = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    bad = 0
    for n in sorted(set(ka) & set(kb)):
        assert ka[n][0] and ka[n][1] and ka[n][2], 'nothing read for ' + n
        what = [w for w, x, y in zip(('instructions', 'descriptor', 'metadata'), ka[n], kb[n]) if x != y]
        if what:
            bad += 1
            print('DIFFERS (%s): %s' % (', '.join(what), demangle(n)))
    for n in gone:
        print('only in a: ' + demangle(n))
    for n in new:
        print('only in b: ' + demangle(n))
    if args.gone:
        with open(args.gone, 'w') as fh:
            fh.write(''.join(n + '\n' for n in gone))
    print('kernels: %d -> %d (%d gone, %d new, %d of %d common differ); .text %d -> %d bytes' % (
        len(ka), len(kb), len(gone), len(new), bad, len(set(ka) & set(kb)), sa, sb))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
