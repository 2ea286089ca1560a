"""Correspondence-graph global registration on the road-scan setting of tools/fpfh_timing.py (2 queries x 20 candidates of
~121 k points, 10 same-world places and 10 of another world per query, voxel-filtered at 0.5 m): the graph stage's kernels
per batch of 20, F4's RANSAC stage on the SAME pair lists in the same run (same scans, same matcher, same handle), the
score kernel's word-operations per second, end-to-end times of both entry points, and how many same-world jobs each stage
locates within 1 m / 5 degrees.

    python tools/pairgraph_timing.py [--queries 2] [--reps 5] [--leaf 0.5] [--out FILE]

Medians of --reps runs on one box.  Kernel times are the handle's HIP-event profiler (a run of its own, profiler on); the
end-to-end times are host time of the synchronous calls with the profiler off.  A word-operation is one 64-bit AND, its
population count and the add: two v_and_b32 and two v_bcnt_u32_b32 (which add as they count), four 32-bit vector
instructions; the count is sum over pairs i of degree_i x ceil(M / 64), from the degrees gloc_reg_pair_graph reports.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OK_T, OK_R = 1.0, 5.0
PEAK_INT32_VECTOR = 256 * 64 * 2.4e9    # MI355X: 256 CUs x 64 lanes per clock x 2.4 GHz, 32-bit integer vector instructions
OPS_PER_WORD = 4.0
NONE = 0xFFFFFFFF
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
        f"default gloc_fpfh_graph_params and gloc_fpfh_params; medians of {a.reps}, one box")

    # ---- the score kernel's work, from the pair lists themselves (the matcher on host features, the graph on host lists) ---------
    fq, xq = store.fpfh(r["q"]), store.download(r["q"])
    word_ops, dens, Ms = 0, [], []
    for t in r["db"]:
        idx, _ = reg.fpfh_match(fq, store.fpfh(t), mutual=True)
        keep = np.flatnonzero(idx != NONE)
        g = reg.pair_graph(xq[keep], store.download(t)[idx[keep]])
        m = len(keep)
        word_ops += int(g["degree"].astype(np.int64).sum()) * ((m + 63) // 64)
        dens.append(float(g["degree"].sum()) / max(m * (m - 1), 1))
        Ms.append(m)
    if Ms:
        say(f"pair lists of the first query: M {min(Ms)} .. {max(Ms)}, graph density {min(dens):.3f} .. {max(dens):.3f}, "
            f"{word_ops / 1e6:.1f} M word-operations in the score kernel per batch")

    # ---- kernels, profiler on: both stages on the same pair lists ----------------------------------------------------------------
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    for label, names, call in (("graph stage (gloc_reg_fpfh_graph_batch_ids)", GRAPH, lambda: reg.fpfh_graph_batch(r["q"], r["db"])),
                               ("RANSAC stage (gloc_reg_fpfh_batch_ids)", RANSAC, lambda: reg.fpfh_batch(r["q"], r["db"]))):
        call()
        per = {k: [] for k in names + ("fpfh_match",)}
        for _ in range(a.reps):
            reg.profile_reset()
            call()
            for k in per:
                per[k].append(reg.profile(k))
        say(f"20 candidates, {label}, profiler on, per batch (median of {a.reps}):")
        total = 0.0
        for k in names:
            ms, cnt = float(np.median([p[0] for p in per[k]])), float(np.median([p[1] for p in per[k]]))
            total += ms
            say(f"  {k:12s} {ms:8.3f} ms  {cnt:5.1f} launches")
        say(f"  the stage    {total:8.3f} ms;  the matcher in front of it (fpfh_match) {float(np.median([p[0] for p in per['fpfh_match']])):.3f} ms")
        if names is GRAPH and word_ops:
            ms = float(np.median([p[0] for p in per["pg_score"]]))
            rate = word_ops / (ms * 1e-3)
            say(f"  score kernel: {rate / 1e9:.1f} G word-operations/s = {100.0 * rate * OPS_PER_WORD / PEAK_INT32_VECTOR:.2f} % of the integer vector peak "
                f"({PEAK_INT32_VECTOR / 1e12:.1f} T 32-bit instructions/s, {OPS_PER_WORD:.0f} per word-operation)")
    reg.set_option(capi.REG_OPT_PROFILE, 0)

    # ---- end to end, profiler off, the two entry points alternating ----------------------------------------------------------------
    tg, tf = [], []
    reg.fpfh_graph_batch(r["q"], r["db"])
    reg.fpfh_batch(r["q"], r["db"])
    for _ in range(a.reps):
        t0 = time.perf_counter()
        reg.fpfh_graph_batch(r["q"], r["db"])
        t1 = time.perf_counter()
        reg.fpfh_batch(r["q"], r["db"])
        t2 = time.perf_counter()
        tg.append((t1 - t0) * 1e3)
        tf.append((t2 - t1) * 1e3)
    say(f"end to end (features present), 20 candidates, alternating: graph median {np.median(tg):.2f} ms (min {min(tg):.2f}), "
        f"RANSAC median {np.median(tf):.2f} ms (min {min(tf):.2f})")

    # ---- located within 1 m / 5 degrees ---------------------------------------------------------------------------------------------
    def located(T, ok, truth):
        return sum(bool(ok[c]) and pose_error(T[c], truth[c])[0] <= OK_T and pose_error(T[c], truth[c])[1] <= OK_R for c in range(10))

    tot = dict(graph=0, ransac=0)
    acc = dict(graph=0, ransac=0)
    for row in rows:
        g, f = reg.fpfh_graph_batch(row["q"], row["db"]), reg.fpfh_batch(row["q"], row["db"])
        tot["graph"] += located(g["T"], g["ok"], row["truth"])
        tot["ransac"] += located(f["T"], f["ok"], row["truth"])
        acc["graph"] += int(np.sum(g["ok"][10:]))
        acc["ransac"] += int(np.sum(f["ok"][10:]))
        say(f"  query: pairs {g['n_pairs'].tolist()}")
        say(f"         graph inliers  {g['inliers'].tolist()}")
        say(f"         RANSAC inliers {f['inliers'].tolist()}")
    n_same = 10 * a.queries
    say(f"located within {OK_T} m / {OK_R} deg, same-world jobs: graph {tot['graph']} of {n_same}; RANSAC {tot['ransac']} of {n_same}")
    say(f"different-world jobs reported ok (min_inlier_ratio 0 in both): graph {acc['graph']} of {n_same}; RANSAC {acc['ransac']} of {n_same}")
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
