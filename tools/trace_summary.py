"""Per kernel of a rocprofv3 --kernel-trace csv: launches, median / min / max / total microseconds.

    python3 tools/trace_summary.py DIR        (DIR: what rocprofv3 -d DIR --output-format csv wrote)
"""
import csv
import glob
import os
import sys

import numpy as np


def main(d):
    files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        sys.exit('no kernel_trace.csv under ' + d)
    rows = {}
    for path in files:
        with open(path, newline='') as f:
            for r in csv.DictReader(f):
                rows.setdefault(r['Kernel_Name'], []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    tot = sum(sum(v) for v in rows.values())
    print('kernel time of the whole trace: %.3f ms, %d launches' % (tot / 1e3, sum(len(v) for v in rows.values())))
    print('%8s %10s %10s %10s %12s  %s' % ('launches', 'median_us', 'min_us', 'max_us', 'total_us', 'kernel'))
    for k, v in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
        v = np.array(v)
        print('%8d %10.2f %10.2f %10.2f %12.1f  %s' % (len(v), np.median(v), v.min(), v.max(), v.sum(), k[:150]))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
