"""NDT timing on device ray-cast pairs (not bench.py): filtered source size, valid cells, evaluations per candidate,
milliseconds per query for 1 and for 20 candidates, and the per-kernel profile (gloc_reg_profile).

    python tools/ndt_timing.py [--reps 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gloc3d_amd import capi, synth
    traj, xy = synth.loop_trajectory(400, 328.0)
    world = synth.make_road_world(1001, xy)
    store = capi.ScanStore()
    # a query near pose 100 and 20 database places around it (bench.py's kind of scan: 64 x 2000 rays)
    q_pose = traj[100] @ synth.se3(1.0, (0.3, -0.2, 0.0))
    db_poses = [traj[100 + d] for d in range(-10, 10)]
    ids = store.add_raycast(world, [q_pose] + db_poses, np.arange(21, dtype=np.uint64) + 1)
    q, db = ids[0], ids[1:]
    init = np.stack([np.linalg.inv(T) @ q_pose for T in db_poses]).astype(np.float32)   # the true pose as the guess
    init = init @ synth.se3(0.5, (0.05, -0.05, 0.0)).astype(np.float32)                  # ... a little off
    reg = capi.Registrar(store=store)
    lines = []
    say = lambda s: (print(s), lines.append(s))
    say(f"query scan: {store.points(q)} points; filtered at 0.2 m: {store.points(store.add_approx_voxel(q, 0.2))} points")
    cells = reg.ndt_cells(db[10])
    say(f"target scan: {store.points(db[10])} points; valid 0.5 m cells: {len(cells['count'])}")
    for n in (1, 20):
        reg.ndt_batch(q, db[:n], init_T=init[:n])                 # warm
        reg.set_option(capi.REG_OPT_PROFILE, 1)
        reg.profile_reset()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            T, prob, iters, conv = reg.ndt_batch(q, db[:n], init_T=init[:n])
            t.append((time.perf_counter() - t0) * 1e3)
        reg.set_option(capi.REG_OPT_PROFILE, 0)
        ms = {k: reg.profile(k) for k in ("ndt_filter", "ndt_cells", "ndt_deriv", "ndt_state")}
        say(f"{n} candidate(s): {np.median(t):.2f} ms per query (median of {a.reps}, profiling on; min {min(t):.2f}); "
            f"iterations {iters.min()}..{iters.max()} (mean {iters.mean():.1f}), converged {int(conv.sum())}/{n}")
        ev = ms["ndt_deriv"][1] / a.reps
        say(f"  derivative launches per query {ev:.0f} (each evaluates every candidate still running)")
        for k, (tot, cnt) in ms.items():
            say(f"  {k:11s} {tot / a.reps:8.3f} ms per query  {cnt / a.reps:6.1f} launches")
    # without the profiler's events
    for n in (1, 20):
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            reg.ndt_batch(q, db[:n], init_T=init[:n])
            t.append((time.perf_counter() - t0) * 1e3)
        say(f"{n} candidate(s), profiling off: {np.median(t):.2f} ms per query (median of {a.reps})")
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
