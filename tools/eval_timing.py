"""The evaluation of registered pairs on one query against 20 places at full scan size (the road-scan setting of
tools/fgr_timing.py without the voxel filter: ~121 k points per scan, 10 same-world places and 10 of another world), at
poses 0.1 m / 0.5 degrees beside the truth:

  evaluate_pairs      gloc_reg_evaluate_pairs on the 20 rows: fitness, rmse, count, the 6 x 6 information matrix
  p2l_pairs_system    gloc_reg_p2l_pairs_system on the same rows: the point-to-plane normal equations
  20 x p2l_system     20 single gloc_reg_p2l_system calls: the only way to get those numbers without the list entries

    python tools/eval_timing.py [--reps 21] [--out FILE]

Medians of --reps runs on one box, host time of the synchronous calls (profiler off), the three alternating; then the
kernels of one evaluate_pairs call from the handle's HIP-event profiler (a run of its own).  The targets carry target
indices and normals before anything is timed.  No threshold is set anywhere.
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
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gloc3d_amd import capi, synth
    traj, xy = synth.loop_trajectory(400, 328.0)
    wa, wb = synth.make_road_world(1001, xy), synth.make_road_world(2002, xy)
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))  # noqa: E731
    rng = np.random.default_rng(11)
    wobble = lambda: synth.se3(rng.uniform(-2, 2), (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.03, 0.03)))  # noqa: E731
    at = 60
    q_pose = traj[at] @ synth.se3(rng.uniform(-3, 3), (rng.uniform(-0.4, 0.4), rng.uniform(-0.5, 0.5), 0.02))
    places = [traj[at + d] @ wobble() for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]
    others = [traj[at + d] @ wobble() for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]
    ids = store.add_raycast(wa, [q_pose] + places, np.arange(1, 12, dtype=np.uint64))
    ids += store.add_raycast(wb, others, np.arange(12, 22, dtype=np.uint64))
    q, db = ids[0], ids[1:]
    for t in db:
        store.build_target_index(t)
        store.build_normals(t, 10)
    off = synth.se3(0.5, (0.08, -0.06, 0.01))
    T = np.stack([np.linalg.inv(P) @ q_pose @ off for P in places + others]).astype(np.float32)
    n = len(db)
    say(f"1 query of {store.points(q)} points against {n} places of {min(store.points(t) for t in db)} .. {max(store.points(t) for t in db)} "
        f"(10 same-world, 10 different-world), poses 0.1 m / 0.5 deg beside the truth; default gloc_eval_params and gloc_p2l_params; "
        f"medians of {a.reps}, one box")
    prm = capi.default_p2l_params()
    calls = (("evaluate_pairs", lambda: reg.evaluate_pairs([q] * n, db, T=T)),
             ("p2l_pairs_system", lambda: reg.p2l_pairs_system([q] * n, db, T, prm)),
             ("20 x p2l_system", lambda: [reg.p2l_system(q, db[c], T[c], prm) for c in range(n)]))
    ev = calls[0][1]()
    say(f"fitness same-world {ev['fitness'][:10].min():.3f} .. {ev['fitness'][:10].max():.3f}, different-world "
        f"{ev['fitness'][10:].min():.3f} .. {ev['fitness'][10:].max():.3f}; rmse same-world {ev['rmse'][:10].min():.3f} .. {ev['rmse'][:10].max():.3f} m")
    lst, one = calls[1][1](), calls[2][1]()
    same = all((lst[k][c] == one[c][k]).all() if k < 2 else lst[k][c] == one[c][k] for c in range(n) for k in range(4))
    say(f"p2l_pairs_system rows equal the 20 single calls bit for bit: {same}")
    t = [[] for _ in calls]
    for _ in range(a.reps):
        for i, (_, call) in enumerate(calls):
            t0 = time.perf_counter()
            call()
            t[i].append((time.perf_counter() - t0) * 1e3)
    for (label, _), x in zip(calls, t):
        say(f"  {label:18s} median {np.median(x):8.2f} ms  (min {min(x):.2f}, max {max(x):.2f})")
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    names = ("nn_cold", "eval_accum", "eval_solve")
    calls[0][1]()
    per = {k: [] for k in names}
    for _ in range(a.reps):
        reg.profile_reset()
        calls[0][1]()
        for k in names:
            per[k].append(reg.profile(k))
    say(f"evaluate_pairs, profiler on, per call (median of {a.reps}):")
    for k in names:
        say(f"  {k:12s} {float(np.median([p[0] for p in per[k]])):8.3f} ms  {float(np.median([p[1] for p in per[k]])):5.1f} launches")
    reg.set_option(capi.REG_OPT_PROFILE, 0)
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
