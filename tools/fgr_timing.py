"""Fast Global Registration on the road-scan setting of tools/fpfh_timing.py and tools/pairgraph_timing.py (2 queries x 20
candidates of ~121 k points, 10 same-world places and 10 of another world per query, voxel-filtered at 0.5 m): the FGR
stage's two kernels per batch of 20, and on the SAME pair lists in the same run (same scans, same matcher, same handle) F4's
RANSAC stage and the correspondence-graph stage; end-to-end times of the three entry points, and how many same-world jobs
each stage locates within 1 m / 5 degrees.

    python tools/fgr_timing.py [--queries 2] [--reps 5] [--leaf 0.5] [--out FILE]

Medians of --reps runs on one box.  Kernel times are the handle's HIP-event profiler (a run of its own, profiler on); the
end-to-end times are host time of the synchronous calls with the profiler off.  No threshold is set anywhere: the run
records what one launch of all the updates costs beside the other two stages, whichever way it comes out.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OK_T, OK_R = 1.0, 5.0
FGR = ("fgr_tuple", "fgr_gnc")
GRAPH = ("pg_matrix", "pg_score", "pg_seeds", "pg_fit", "ransac_score", "accum", "solve")
RANSAC = ("ransac_hyp", "ransac_score", "accum", "solve")


def pose_error(T, truth):
    D = np.linalg.inv(np.asarray(truth, np.float64)) @ np.asarray(T, np.float64)
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(D[:3, 3])), float(np.degrees(np.arccos(c)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.5)
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
    seed = 1
    rows = []
    for qi in range(a.queries):                 # (the scans of tools/fpfh_timing.py, draw for draw)
        at = 60 + 90 * qi
        q_pose = traj[at] @ synth.se3(rng.uniform(-3, 3), (rng.uniform(-0.4, 0.4), rng.uniform(-0.5, 0.5), 0.02))
        same = [traj[at + d] @ wobble() for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]
        diff = [traj[at + d] @ wobble() for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]
        raw = store.add_raycast(wa, [q_pose] + same, np.arange(seed, seed + 11, dtype=np.uint64))
        raw += store.add_raycast(wb, diff, np.arange(seed + 11, seed + 21, dtype=np.uint64))
        seed += 21
        ids = [store.add_approx_voxel(i, a.leaf) for i in raw]
        for t in ids[1:]:
            store.build_target_index(t)
        for t in ids:
            store.build_fpfh(t, 10, 16)
        truth = np.stack([np.linalg.inv(T) @ q_pose for T in same])
        rows.append(dict(q=ids[0], db=ids[1:], truth=truth))
    r = rows[0]
    say(f"scans voxel-filtered at {a.leaf} m: {store.points(r['q'])} points (query), {min(store.points(t) for t in r['db'])} .. "
        f"{max(store.points(t) for t in r['db'])} (places); {a.queries} queries x 20 candidates (10 same-world, 10 different-world); "
        f"default gloc_fgr_params, gloc_fpfh_params and gloc_fpfh_graph_params; medians of {a.reps}, one box")
    stages = (("FGR stage (gloc_reg_fpfh_fgr_batch_ids)", FGR, lambda q, db: reg.fpfh_fgr_batch(q, db)),
              ("RANSAC stage (gloc_reg_fpfh_batch_ids)", RANSAC, lambda q, db: reg.fpfh_batch(q, db)),
              ("graph stage (gloc_reg_fpfh_graph_batch_ids)", GRAPH, lambda q, db: reg.fpfh_graph_batch(q, db)))
    g = stages[0][2](r["q"], r["db"])
    say(f"pair lists of the first query: M {int(g['n_pairs'].min())} .. {int(g['n_pairs'].max())}")

    # ---- kernels, profiler on: the three stages on the same pair lists -------------------------------------------------------------
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    for label, names, call in stages:
        call(r["q"], r["db"])
        per = {k: [] for k in names + ("fpfh_match",)}
        for _ in range(a.reps):
            reg.profile_reset()
            call(r["q"], r["db"])
            for k in per:
                per[k].append(reg.profile(k))
        say(f"20 candidates, {label}, profiler on, per batch (median of {a.reps}):")
        total = 0.0
        for k in names:
            ms, cnt = float(np.median([p[0] for p in per[k]])), float(np.median([p[1] for p in per[k]]))
            total += ms
            say(f"  {k:12s} {ms:8.3f} ms  {cnt:5.1f} launches")
        say(f"  the stage    {total:8.3f} ms;  the matcher in front of it (fpfh_match) {float(np.median([p[0] for p in per['fpfh_match']])):.3f} ms")
    # one job alone: what a single launch of all the updates costs when nothing runs beside it
    for label, names, call in stages:
        call(r["q"], r["db"][:1])
        per = []
        for _ in range(a.reps):
            reg.profile_reset()
            call(r["q"], r["db"][:1])
            per.append(sum(reg.profile(k)[0] for k in names))
        say(f"1 candidate, {label}: the stage {float(np.median(per)):.3f} ms")
    reg.set_option(capi.REG_OPT_PROFILE, 0)

    # ---- end to end, profiler off, the three entry points alternating ---------------------------------------------------------------
    t = [[] for _ in stages]
    for _, _, call in stages:
        call(r["q"], r["db"])
    for _ in range(a.reps):
        for i, (_, _, call) in enumerate(stages):
            t0 = time.perf_counter()
            call(r["q"], r["db"])
            t[i].append((time.perf_counter() - t0) * 1e3)
    say("end to end (features present), 20 candidates, alternating: " +
        ", ".join(f"{label.split(' ')[0]} median {np.median(x):.2f} ms (min {min(x):.2f})" for (label, _, _), x in zip(stages, t)))

    # ---- located within 1 m / 5 degrees ---------------------------------------------------------------------------------------------
    def located(T, ok, truth):
        return sum(bool(ok[c]) and pose_error(T[c], truth[c])[0] <= OK_T and pose_error(T[c], truth[c])[1] <= OK_R for c in range(10))

    tot, acc = [0] * len(stages), [0] * len(stages)
    for row in rows:
        res = [call(row["q"], row["db"]) for _, _, call in stages]
        for i, g in enumerate(res):
            tot[i] += located(g["T"], g["ok"], row["truth"])
            acc[i] += int(np.sum(g["ok"][10:]))
        say(f"  query: pairs {res[0]['n_pairs'].tolist()}")
        for (label, _, _), g in zip(stages, res):
            say(f"         {label.split(' ')[0]:6s} inliers {g['inliers'].tolist()}")
    n_same = 10 * a.queries
    say(f"located within {OK_T} m / {OK_R} deg, same-world jobs: " +
        "; ".join(f"{label.split(' ')[0]} {n} of {n_same}" for (label, _, _), n in zip(stages, tot)))
    say("different-world jobs reported ok (min_inlier_ratio 0 everywhere): " +
        "; ".join(f"{label.split(' ')[0]} {n} of {n_same}" for (label, _, _), n in zip(stages, acc)))
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
