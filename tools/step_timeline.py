"""Kernel time line of ONE registration batch out of a rocprofv3 kernel trace of bench.py.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python3 bench.py --no-legs --no-cpu-baseline --steps 5
    python3 tools/step_timeline.py DIR > profiles/step_timeline_<which>.txt

The batch shown is the last complete one: from the last-but-one cold 1-NN launch (the pairs pass, `nn_compact_cold_kernel<true>`; `nn_compact_kernel<2, true, ...>` before it had a kernel of its own)
up to the kernel in front of the last one, so the kernels between two batches (retrieval, the next batch's preamble) are in it
too.  Per kernel: start (us from the batch's first kernel), duration, the idle gap to the NEXT kernel; then the sums per kernel
name.  Kernel trace only -- counters belong in a run of their own.
"""
import csv
import glob
import sys
from collections import OrderedDict


def short(name):
    n = name.replace("void ", "").replace("gloc::reg::", "").replace("gloc::", "")
    cut = n.find("(")
    return (n if cut < 0 else n[:cut])[:72]


def main(d):
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under " + d)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    cold = [i for i, r in enumerate(rows) if "nn_compact_kernel<2, true" in r[2] or "nn_compact_cold_kernel<true" in r[2]]
    if len(cold) < 2:
        sys.exit("fewer than two cold 1-NN launches in the trace")
    i0, i1 = cold[-2], cold[-1]
    batch = rows[i0:i1]
    t0 = batch[0][0]
    print(f"# one batch: kernels {i0}..{i1 - 1} of {len(rows)} in the trace; times in us")
    print(f"# {'start':>9} {'dur':>9} {'gap>next':>9}  kernel")
    fam = OrderedDict()
    busy = gaps = 0.0
    for k, (s, e, n) in enumerate(batch):
        nxt = rows[i0 + k + 1][0]
        gap = (nxt - e) / 1e3
        print(f"  {(s - t0) / 1e3:9.1f} {(e - s) / 1e3:9.1f} {gap:9.1f}  {short(n)}")
        a = fam.setdefault(short(n), [0, 0.0, 0.0])
        a[0] += 1
        a[1] += (e - s) / 1e3
        a[2] += gap
        busy += (e - s) / 1e3
        gaps += gap
    span = (rows[i1][0] - t0) / 1e3
    print(f"# span {span:.1f} us = kernels {busy:.1f} + gaps {gaps:.1f}")
    print(f"# {'launches':>8} {'sum dur':>10} {'mean dur':>9} {'sum gap':>9} {'mean gap':>9}  kernel")
    for n, (c, du, ga) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        print(f"  {c:8d} {du:10.1f} {du / c:9.1f} {ga:9.1f} {ga / c:9.2f}  {n}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
