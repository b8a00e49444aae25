#!/usr/bin/env python3
"""Per-launch times out of a rocprofv3 kernel trace, keyed by kernel AND grid: one template instantiation runs at several grids in a
step, and `--stats` sums them.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python3 bench.py --trace-run > LOG
    python3 tools/per_launch.py DIR/..._kernel_trace.csv [substring ...] > per_launch_<tag>.txt

One line per (kernel, grid), longest total first: launches, mean and total microseconds, the grid (work-items) and the demangled
name.  With substrings, only the kernels whose name holds one of them (default: conv_mfma_f32 and conv_pair_f32)."""
import collections
import csv
import sys


def main():
    path, keys = sys.argv[1], sys.argv[2:] or ['conv_mfma_f32', 'conv_pair_f32']
    d = collections.defaultdict(list)
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row['Kernel_Name']
            if not any(k in name for k in keys):
                continue
            grid = ','.join(row[k] for k in ('Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z')) if 'Grid_Size_X' in row else row.get('Grid_Size', '?')
            d[name.replace('void ', '').replace('acgconv::', ''), grid].append(int(row['End_Timestamp']) - int(row['Start_Timestamp']))
    for (name, grid), xs in sorted(d.items(), key=lambda kv: -sum(kv[1])):
        print('%8d launches  mean %9.2f us  total %10.1f us  grid %s  %s' % (len(xs), sum(xs) / len(xs) / 1e3, sum(xs) / 1e3, grid, name))


if __name__ == '__main__':
    main()
