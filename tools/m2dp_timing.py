"""M2DP timing (not bench.py): descriptors of one resident full-size scan and of a batch of them, each stage from the
handle's HIP-event profile (gloc_m2dp_profile); the projection's (point, plane) rate against the fp64 vector peak, and the
whole call against one read of the points at the copy rate DESIGN.md section 3 records and against Scan Context's
scatter of the same scans.

    python tools/m2dp_timing.py [--reps 10] [--scans 64] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29        # a plain copy on this pool
FP64_TFLOPS = 78.6     # fp64 vector peak (spec)
EVAL_FLOP = 20         # fp64 operations of the contract per (point, plane): two 3-term dot products, rho^2 and its
                       # scaling, 3 ring and 4 sector border tests (the bisections' bookkeeping is not arithmetic)
KERNELS = ("m2dp_frame", "m2dp_project", "m2dp_svd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gloc3d_amd import capi, synth
    traj, xy = synth.loop_trajectory(400, 328.0)
    world = synth.make_road_world(1001, xy)
    store = capi.ScanStore()
    ids = store.add_raycast(world, traj[:a.scans], np.arange(a.scans, dtype=np.uint64) + 1)   # 64 x 2000 rays each
    m = capi.M2dp()
    sc = capi.ScanContext()
    lines = []
    say = lambda s: (print(s), lines.append(s))

    def profiled(h, kernels, fn):
        fn()                                            # warm: buffers sized, code loaded
        h.set_profile(True)
        h.profile_reset()
        for _ in range(a.reps):
            fn()
        out = {k: h.profile(k)[0] / a.reps * 1e3 for k in kernels}       # microseconds per call
        h.set_profile(False)
        return out

    say(f"descriptor {m.n_planes} planes x {m.n_bins} bins = {m.dim} floats; {a.reps} repetitions")
    for group in (ids[:1], ids):
        pts = sum(store.points(i) for i in group)
        prof = profiled(m, KERNELS, lambda: m.describe_store_scans(store, group))
        scat = profiled(sc, ("sc_scatter",), lambda: sc.describe_store_scans(store, group))["sc_scatter"]
        total = sum(prof.values())
        evals = pts * m.n_planes
        read_us = pts * 12 / COPY_TBS / 1e6
        tf = evals * EVAL_FLOP / prof["m2dp_project"] / 1e6
        say(f"{len(group)} scan{'s' if len(group) > 1 else ''}, {pts / len(group):.0f} points each: frame {prof['m2dp_frame']:.1f} us, "
            f"projection {prof['m2dp_project']:.1f} us, svd {prof['m2dp_svd']:.1f} us, together {total:.1f} us")
        say(f"  projection: {evals / prof['m2dp_project'] / 1e3:.2f} G (point, plane) evaluations/s; at ~{EVAL_FLOP} fp64 operations each "
            f"{tf:.2f} TFLOP/s = {100 * tf / FP64_TFLOPS:.1f} % of the {FP64_TFLOPS} TFLOP/s fp64 vector peak")
        say(f"  one read of the points at {COPY_TBS} TB/s: {read_us:.2f} us (the frame reads them 3 times, the projection once); "
            f"Scan Context's scatter of the same scans: {scat:.1f} us")
    m.close()
    sc.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
