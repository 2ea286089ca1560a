"""Scan Context timing (not bench.py): descriptors of a batch of resident full-size scans, then one query and 64 queries
against 4541 rows, each from the handle's HIP-event profile (gloc_sc_profile), per kernel; the distance kernel's row
stream against the copy rate DESIGN.md section 3 records and its FMA rate against the fp32 vector peak.

    python tools/sc_timing.py [--reps 10] [--scans 64] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 4541            # KITTI odometry 00
COPY_TBS = 6.29        # a plain copy on this pool
FP32_TFLOPS = 157.3    # fp32 vector peak (spec)
KERNELS = ("sc_scatter", "sc_finish", "sc_dist", "sc_select")


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
    sc = capi.ScanContext()
    R, S = sc.shape
    lines = []
    say = lambda s: (print(s), lines.append(s))
    pts = sum(store.points(i) for i in ids)
    say(f"{a.scans} resident scans, {pts / a.scans:.0f} points each; descriptor {R} x {S}; {a.reps} repetitions")

    def profiled(fn):
        fn()                                            # warm: buffers sized, code loaded
        sc.set_profile(True)
        sc.profile_reset()
        for _ in range(a.reps):
            fn()
        out = {k: sc.profile(k) for k in KERNELS}
        sc.set_profile(False)
        return {k: (ms / a.reps * 1e3, n / a.reps) for k, (ms, n) in out.items()}       # microseconds, launches per call

    prof = profiled(lambda: sc.describe_store_scans(store, ids))
    us = prof["sc_scatter"][0]
    say(f"describe_store_scans, {a.scans} scans: scatter {us:.1f} us ({pts * 12 / us / 1e6:.2f} TB/s of points read, "
        f"{pts / us / 1e3:.2f} G points/s)")

    # the database: the scans' descriptors, rolled and perturbed up to 4541 distinct rows
    base = sc.describe_store_scans(store, ids)
    rng = np.random.default_rng(5)
    pick = rng.integers(0, a.scans, ROWS)
    rows = np.stack([np.roll(base[p], int(s), axis=1) for p, s in zip(pick, rng.integers(0, S, ROWS))])
    rows = (rows * rng.uniform(0.9, 1.1, rows.shape)).astype(np.float32)
    sc.add(rows)
    row_bytes = 4 * S * 4 * ((R + 3) // 4) + 8          # the unit columns and the mask: what the distance kernel streams
    for nq in (1, 64):
        q = rows[rng.integers(0, ROWS, nq)]
        prof = profiled(lambda: sc.search(q, 20))
        d_us, s_us = prof["sc_dist"][0], prof["sc_select"][0]
        groups = (nq + 3) // 4                         # a row is loaded once per group of 4 queries
        tbs = ROWS * row_bytes * groups / d_us / 1e6
        tf = 2.0 * nq * ROWS * S * S * R / d_us / 1e6
        say(f"search, {nq} quer{'y' if nq == 1 else 'ies'} x {ROWS} rows, k = 20: finish {prof['sc_finish'][0]:.1f} us, "
            f"distance {d_us:.1f} us, selection {s_us:.1f} us")
        say(f"  distance kernel: rows streamed at {tbs:.3f} TB/s = {100 * tbs / COPY_TBS:.1f} % of the {COPY_TBS} TB/s copy rate; "
            f"{tf:.2f} TFLOP/s = {100 * tf / FP32_TFLOPS:.1f} % of the {FP32_TFLOPS} TFLOP/s fp32 vector peak; "
            f"nearer to the {'compute' if tf / FP32_TFLOPS > tbs / COPY_TBS else 'memory'} bound")
    sc.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
