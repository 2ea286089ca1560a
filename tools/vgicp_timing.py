"""Voxelized generalized ICP (neighbors 1, 7 and 27) against generalized ICP on bench.py's kind of scans (distinct
64 x 2000 ray-casts along the road world), all from the same starts: pose error after each pass, passes needed, time per
pass split into search, accumulate and solve, the voxel build per call, a 20-candidate batch end to end.

    python tools/vgicp_timing.py [--queries 2] [--reps 5] [--resolution 1.0] [--out FILE]

The scans, candidates and starts are tools/gicp_timing.py's (and tools/p2l_timing.py's): every query has 20 candidates,
10 same-world places around it and 10 places of another world; the refinements start from the pose the RANSAC stage hands
to ICP today (a batch with icp_iters = 0).  Generalized ICP's columns are the baseline, from the same build and run.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from p2l_timing import MAX_PASSES, STEP_R, STEP_T, passes_needed, pose_err  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gloc3d_amd import capi, synth
    traj, xy = synth.loop_trajectory(400, 328.0)
    wa, wb = synth.make_road_world(1001, xy), synth.make_road_world(2002, xy)
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    rng = np.random.default_rng(11)
    wobble = lambda: synth.se3(rng.uniform(-2, 2), (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.03, 0.03)))
    seed = 1
    rows = []
    for qi in range(a.queries):
        at = 60 + 90 * qi
        q_pose = traj[at] @ synth.se3(rng.uniform(-3, 3), (rng.uniform(-0.4, 0.4), rng.uniform(-0.5, 0.5), 0.02))
        same = [traj[at + d] @ wobble() for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]
        diff = [traj[at + d] @ wobble() for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]
        ids = store.add_raycast(wa, [q_pose] + same, np.arange(seed, seed + 11, dtype=np.uint64))
        ids += store.add_raycast(wb, diff, np.arange(seed + 11, seed + 21, dtype=np.uint64))
        seed += 21
        q, db = ids[0], ids[1:]
        for t in db:
            store.build_target_index(t)              # (generalized ICP's search wants it; the voxelized refinement ignores it)
        for t in ids:
            store.build_normals(t, 10)
        truth = np.stack([np.linalg.inv(T) @ q_pose for T in same])
        rs = reg.batch_ids(q, db, params=capi.default_reg_params(icp_iters=0))
        rows.append(dict(q=q, db=db, truth=truth, init=rs["T"].astype(np.float32)))
    say(f"scans: {store.points(rows[0]['q'])} points (query), {store.points(rows[0]['db'][0])} (a place); {a.queries} queries x 20 candidates "
        f"(10 same-world, 10 different-world); starts: the RANSAC stage's poses; normals k = 10 on every scan; plane_eps 1e-3; "
        f"voxels of {a.resolution:g} m")
    start = np.concatenate([[pose_err(r["truth"][c], r["init"][c])[0] for c in range(10)] for r in rows])
    say(f"starts, same-world jobs: translation error median {np.median(start) * 1e3:.0f} mm, max {start.max() * 1e3:.0f} mm")
    nv = [len(reg.vgicp_voxels(t, capi.default_vgicp_params(resolution=a.resolution))["count"]) for t in rows[0]["db"]]
    say(f"voxels per target: {min(nv)} .. {max(nv)}")

    def vg(nb):
        return lambda r, k, n=20: reg.vgicp_batch(r["q"], r["db"][:n], init_T=r["init"][:n],
                                                  params=capi.default_vgicp_params(max_iters=k, neighbors=nb, resolution=a.resolution))[0]

    methods = {
        "gicp": lambda r, k, n=20: reg.gicp_batch(r["q"], r["db"][:n], init_T=r["init"][:n], params=capi.default_gicp_params(max_iters=k))[0],
        "vg1": vg(1), "vg7": vg(7), "vg27": vg(27),
    }

    # ---- pose error after each pass, passes needed ----------------------------------------------------------------
    need = {m: [] for m in methods}
    need_far = {m: [] for m in methods}
    err = {m: [[] for _ in range(MAX_PASSES + 1)] for m in methods}
    rot = {m: [] for m in methods}
    for r in rows:
        for m, run in methods.items():
            seq = [r["init"]] + [run(r, k) for k in range(1, MAX_PASSES + 2)]
            nd = passes_needed(seq)
            need[m] += list(nd[:10])
            need_far[m] += list(nd[10:])
            for k in range(MAX_PASSES + 1):
                err[m][k] += [pose_err(r["truth"][c], seq[k][c])[0] for c in range(10)]
            rot[m] += [pose_err(r["truth"][c], seq[MAX_PASSES][c])[1] for c in range(10)]
    say(f"passes until one more moves the pose by < {STEP_T * 1e3:g} mm and < {STEP_R * 1e3:g} mrad ({MAX_PASSES + 1}: not within {MAX_PASSES}):")
    for name, d in (("same-world", need), ("different-world", need_far)):
        for m in methods:
            v = np.array(d[m])
            say(f"  {name:15s} {m:4s}: median {np.median(v):.0f}, mean {v.mean():.1f}, min {v.min()}, max {v.max()}  {sorted(v.tolist())}")
    say("translation error against ground truth after each pass, same-world jobs, median (max) in mm:")
    for k in list(range(0, 11)) + [12, 15, 20, 30]:
        say(f"  after {k:2d} passes: " + ", ".join(f"{m} {np.median(err[m][k]) * 1e3:7.1f} ({max(err[m][k]) * 1e3:7.1f})" for m in methods))
    say(f"rotation error after {MAX_PASSES} passes, same-world, median (max) in mrad: "
        + ", ".join(f"{m} {np.median(rot[m]) * 1e3:.2f} ({max(rot[m]) * 1e3:.2f})" for m in methods))

    # ---- time: per pass (profiler on: launch by launch) and end to end (profiler off) -----------------------------
    r = rows[0]
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    vfam = ("vgicp_voxels", "vgicp_accum", "vgicp_solve")
    fams = {"gicp": ("nn", "nn_cold", "gicp_accum", "gicp_solve"), "vg1": vfam, "vg7": vfam, "vg27": vfam}
    for m, run in methods.items():
        run(r, MAX_PASSES)
        reg.profile_reset()
        for _ in range(a.reps):
            run(r, MAX_PASSES)
        say(f"{m}, 20 candidates, {MAX_PASSES} passes, profiler on (one launch per kernel and pass), per batch:")
        per_pass = 0.0
        for k in fams[m]:
            tot, cnt = reg.profile(k)
            if cnt:
                say(f"  {k:12s} {tot / a.reps:8.3f} ms  {cnt / a.reps:6.1f} launches  {1e3 * tot / cnt:7.1f} us each")
                if k not in ("nn_cold", "vgicp_voxels"):
                    per_pass += 1e3 * tot / cnt
        say(f"  a pass ({'search + ' if m == 'gicp' else ''}accumulate + solve): {per_pass:.1f} us")
    reg.set_option(capi.REG_OPT_PROFILE, 0)
    for k in (30, 10, 5):
        for m in methods:
            methods[m](r, k)
            t = []
            for _ in range(max(a.reps, 5)):
                t0 = time.perf_counter()
                methods[m](r, k)
                t.append((time.perf_counter() - t0) * 1e3)
            say(f"end to end, 20 candidates, {m} {k} passes: median {np.median(t):.2f} ms, min {min(t):.2f} (host time of the call, "
                f"{len(t)} runs{'; the voxel build included' if m != 'gicp' else ''})")
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
