"""Point-to-plane against point-to-point ICP on bench.py's kind of scans (distinct 64 x 2000 ray-casts along the road
world): passes needed, final accuracy, time per pass, the normals' one-off cost, a 20-candidate batch end to end.

    python tools/p2l_timing.py [--queries 3] [--reps 5] [--out FILE]

Every query has 20 candidates: 10 same-world places around it (distinct casts, each with its own perturbation) and 10
places of another world.  Both refinements start from the pose the RANSAC stage hands to ICP today (a batch with
icp_iters = 0).  "Passes needed": the first k after which one more pass moves the pose by less than STEP_T metres and
STEP_R radians, read off the poses of runs with k = 0 .. 30 passes (both refinements are deterministic).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_T, STEP_R = 1e-3, 1e-4
MAX_PASSES = 30


def pose_err(A, B):
    E = np.linalg.inv(np.asarray(A, np.float64)) @ np.asarray(B, np.float64)
    return np.linalg.norm(E[:3, 3]), np.linalg.norm(E[:3, :3] - np.eye(3)) / np.sqrt(2.0)


def passes_needed(seq):
    """seq [k][n, 4, 4]: per job the first k whose next update is below the step (MAX_PASSES + 1: never)."""
    n = seq[0].shape[0]
    out = np.full(n, MAX_PASSES + 1)
    for c in range(n):
        for k in range(len(seq) - 1):
            dt, da = pose_err(seq[k][c], seq[k + 1][c])
            if dt < STEP_T and da < STEP_R:
                out[c] = k
                break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
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
    t_norm = []
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
            store.build_target_index(t)
        for t in db:                                             # the one-off cost, scan by scan
            t0 = time.perf_counter()
            store.build_normals(t, 10)
            t_norm.append((time.perf_counter() - t0) * 1e3)
        truth = np.stack([np.linalg.inv(T) @ q_pose for T in same])
        rs = reg.batch_ids(q, db, params=capi.default_reg_params(icp_iters=0))
        init = rs["T"].astype(np.float32)
        rows.append(dict(q=q, db=db, truth=truth, init=init, ok=rs["ok"]))
    say(f"scans: {store.points(rows[0]['q'])} points (query), {store.points(rows[0]['db'][0])} (a place); {a.queries} queries x 20 candidates "
        f"(10 same-world, 10 different-world); starts: the RANSAC stage's poses")
    say(f"normals (k = 10) of a whole place scan, host time of gloc_scan_store_build_normals: median {np.median(t_norm):.2f} ms, "
        f"min {min(t_norm):.2f}, max {max(t_norm):.2f} over {len(t_norm)} scans (the first includes the scratch allocations)")
    ge = capi.GroundEstimator()
    xyz = store.download(rows[0]["db"][0])
    near = np.ascontiguousarray(xyz[np.einsum("ij,ij->i", xyz, xyz) < 400])
    ge.normals(near, 10)
    tg = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ge.normals(near, 10)
        tg.append((time.perf_counter() - t0) * 1e3)
    say(f"for comparison gloc_ground_normals on the {len(near)} points within 20 m of the same scan (host buffers in and out): "
        f"median {np.median(tg):.2f} ms")
    ge.close()

    # ---- passes needed and final accuracy ------------------------------------------------------------------------
    need = {"p2l": [], "p2p": []}
    err = {"p2l": [], "p2p": [], "start": []}
    need_far = {"p2l": [], "p2p": []}
    for r in rows:
        seq_l, seq_p = [r["init"]], [r["init"]]
        for k in range(1, MAX_PASSES + 2):
            seq_l.append(reg.p2l_batch(r["q"], r["db"], init_T=r["init"], params=capi.default_p2l_params(max_iters=k))[0])
            seq_p.append(reg.batch_ids(r["q"], r["db"], init_T=r["init"], params=capi.default_reg_params(ransac_iters=0, icp_iters=k))["T"])
        nl, npp = passes_needed(seq_l), passes_needed(seq_p)
        need["p2l"] += list(nl[:10]); need["p2p"] += list(npp[:10])
        need_far["p2l"] += list(nl[10:]); need_far["p2p"] += list(npp[10:])
        for c in range(10):
            err["start"].append(pose_err(r["truth"][c], r["init"][c]))
            err["p2l"].append(pose_err(r["truth"][c], seq_l[MAX_PASSES][c]))
            err["p2p"].append(pose_err(r["truth"][c], seq_p[MAX_PASSES][c]))
    say(f"passes until one more moves the pose by < {STEP_T * 1e3:g} mm and < {STEP_R * 1e3:g} mrad ({MAX_PASSES + 1}: not within {MAX_PASSES}):")
    for name, d in (("same-world", need), ("different-world", need_far)):
        for m in ("p2p", "p2l"):
            v = np.array(d[m])
            say(f"  {name:15s} {m}: median {np.median(v):.0f}, mean {v.mean():.1f}, min {v.min()}, max {v.max()}  {sorted(v.tolist())}")
    for m in ("start", "p2p", "p2l"):
        e = np.array(err[m])
        say(f"  error against ground truth after {MAX_PASSES if m != 'start' else 0} passes, same-world, {m:5s}: translation median {np.median(e[:, 0]) * 1e3:.1f} mm "
            f"max {e[:, 0].max() * 1e3:.1f} mm; rotation median {np.median(e[:, 1]) * 1e3:.2f} mrad max {e[:, 1].max() * 1e3:.2f} mrad")
    # accuracy as a function of the pass count
    for k in (1, 2, 3, 5, 8, 12, 20, 30):
        el, ep = [], []
        for r in rows:
            Tl = reg.p2l_batch(r["q"], r["db"][:10], init_T=r["init"][:10], params=capi.default_p2l_params(max_iters=k))[0]
            Tp = reg.batch_ids(r["q"], r["db"][:10], init_T=r["init"][:10], params=capi.default_reg_params(ransac_iters=0, icp_iters=k))["T"]
            el += [pose_err(r["truth"][c], Tl[c])[0] for c in range(10)]
            ep += [pose_err(r["truth"][c], Tp[c])[0] for c in range(10)]
        say(f"  after {k:2d} passes: median translation error p2p {np.median(ep) * 1e3:6.1f} mm, p2l {np.median(el) * 1e3:6.1f} mm; "
            f"max p2p {max(ep) * 1e3:6.1f}, p2l {max(el) * 1e3:6.1f}")
    # poor starts: the RANSAC pose pushed 1.5 m and 8 degrees off
    off = synth.se3(8.0, (1.2, -0.9, 0.1)).astype(np.float32)
    el, ep = [], []
    for r in rows:
        bad = (off[None] @ r["init"][:10]).astype(np.float32)
        Tl = reg.p2l_batch(r["q"], r["db"][:10], init_T=bad, params=capi.default_p2l_params(max_iters=MAX_PASSES))[0]
        Tp = reg.batch_ids(r["q"], r["db"][:10], init_T=bad, params=capi.default_reg_params(ransac_iters=0, icp_iters=MAX_PASSES))["T"]
        el += [pose_err(r["truth"][c], Tl[c])[0] for c in range(10)]
        ep += [pose_err(r["truth"][c], Tp[c])[0] for c in range(10)]
    say(f"poor starts (1.5 m, 8 deg off), {MAX_PASSES} passes: within 5 cm of the truth p2p {int((np.array(ep) < 0.05).sum())}/{len(ep)}, "
        f"p2l {int((np.array(el) < 0.05).sum())}/{len(el)}; median error p2p {np.median(ep) * 1e3:.0f} mm, p2l {np.median(el) * 1e3:.0f} mm")

    # ---- time: per pass (profiler on: launch by launch) and end to end (profiler off) -------------------------------
    r = rows[0]
    prm_p = capi.default_reg_params(ransac_iters=0, icp_iters=MAX_PASSES)
    prm_l = capi.default_p2l_params(max_iters=MAX_PASSES)
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    for name, run, fams in (("p2p", lambda: reg.batch_ids(r["q"], r["db"], init_T=r["init"], params=prm_p), ("nn", "nn_cold", "accum", "solve")),
                            ("p2l", lambda: reg.p2l_batch(r["q"], r["db"], init_T=r["init"], params=prm_l), ("nn", "nn_cold", "p2l_accum", "p2l_solve"))):
        run()
        reg.profile_reset()
        for _ in range(a.reps):
            run()
        say(f"{name}, 20 candidates, {MAX_PASSES} passes, profiler on (one launch per kernel and pass), per batch:")
        for k in fams:
            tot, cnt = reg.profile(k)
            if cnt:
                say(f"  {k:10s} {tot / a.reps:8.3f} ms  {cnt / a.reps:6.1f} launches  {1e3 * tot / cnt:7.1f} us each")
    reg.set_option(capi.REG_OPT_PROFILE, 0)
    for name, run in (("p2p 30 passes (the chained launch)", lambda: reg.batch_ids(r["q"], r["db"], init_T=r["init"], params=prm_p)),
                      ("p2p 20 passes", lambda: reg.batch_ids(r["q"], r["db"], init_T=r["init"], params=capi.default_reg_params(ransac_iters=0, icp_iters=20))),
                      ("p2l 30 passes", lambda: reg.p2l_batch(r["q"], r["db"], init_T=r["init"], params=prm_l)),
                      ("p2l 10 passes", lambda: reg.p2l_batch(r["q"], r["db"], init_T=r["init"], params=capi.default_p2l_params(max_iters=10))),
                      ("p2l 5 passes", lambda: reg.p2l_batch(r["q"], r["db"], init_T=r["init"], params=capi.default_p2l_params(max_iters=5))),
                      ("p2l eps 1 mm / 0.1 mrad", lambda: reg.p2l_batch(r["q"], r["db"], init_T=r["init"],
                                                                       params=capi.default_p2l_params(trans_eps=STEP_T, rot_eps=STEP_R)))):
        run()
        t = []
        for _ in range(max(a.reps, 5)):
            t0 = time.perf_counter()
            run()
            t.append((time.perf_counter() - t0) * 1e3)
        say(f"end to end, 20 candidates, {name}: median {np.median(t):.2f} ms, min {min(t):.2f} (host time of the call, {len(t)} runs)")
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
