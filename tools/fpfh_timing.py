"""FPFH feature-based global registration on bench.py's kind of scans (tools/gicp_timing.py's road scans: 2 queries x 20
candidates of ~121 k points, 10 same-world places and 10 of another world per query), voxel-filtered at the leaf the test
table commits (tests/fpfh_cases.py LEAF): feature build per scan, the matcher per job with mutual on and off, the RANSAC
stage, a 20-candidate batch end to end -- and how many of the 40 jobs are located within 1 m / 5 degrees of ground truth,
beside the RANSAC stage of gloc_reg_batch_ids on the same filtered scans from the identity guess.

    python tools/fpfh_timing.py [--queries 2] [--reps 5] [--leaf 0.5] [--out FILE] [--support] [--keypoints] [--build-only]

Medians of --reps runs on one box; host time of synchronous calls unless a line says "profiler".

--support adds the radius-support features (gloc_fpfh_radius_params) beside the k-NN ones, everything from the same run:
the feature build on a filtered scan at the default support and on a raw scan at SUPPORTS["raw"], each next to the k-mode
build of the same scan, and the 40 jobs under the supports of SUPPORTS through RANSAC and through the correspondence graph --
located within 1 m / 5 degrees, median error, inlier populations of the two groups -- beside k-mode's.  --build-only stops
after the builds: what a `rocprofv3 --kernel-trace --stats` run of its own wraps to split the build by kernel.

--keypoints adds the ISS keypoints (gloc_iss_params at their defaults), everything from the same run: the keypoint build on a
filtered scan beside the feature builds, K per scan, the matcher and the pair compaction per 20 candidates with and without
keypoints (profiler) and the batch end to end, and the six rows of the localization table -- k-mode and the two radius
supports, through RANSAC and through the graph -- each without and with keypoints.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OK_T, OK_R = 1.0, 5.0
# name -> gloc_fpfh_radius_params fields; "default" is gloc_fpfh_radius_default_params (2 x and 5 x the 0.5 m leaf)
SUPPORTS = {"default": {},
            "tight": dict(normal_radius=0.75, feature_radius=1.5, normal_max_nn=32, feature_max_nn=64),
            "raw": dict(normal_radius=0.5, feature_radius=1.0)}
PEAK_FP32_VECTOR = 157.3e12   # MI355X, fp32 vector, an fma counted as two operations


def pose_error(T, truth):
    D = np.linalg.inv(np.asarray(truth, np.float64)) @ np.asarray(T, np.float64)
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(D[:3, 3])), float(np.degrees(np.arccos(c)))


def med(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--support", action="store_true", help="add the radius-support measurements")
    ap.add_argument("--keypoints", action="store_true", help="add the ISS keypoint measurements")
    ap.add_argument("--build-only", action="store_true", help="with --support / --keypoints: the builds alone (for a kernel trace)")
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
    for qi in range(a.queries):
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
        truth = np.stack([np.linalg.inv(T) @ q_pose for T in same])
        rows.append(dict(raw=raw, q=ids[0], db=ids[1:], truth=truth))
    n_q, n_db = store.points(rows[0]["q"]), [store.points(t) for t in rows[0]["db"]]
    say(f"scans: {store.points(rows[0]['raw'][0])} points raw, voxel-filtered at {a.leaf} m: {n_q} (query), {min(n_db)} .. {max(n_db)} (places); "
        f"{a.queries} queries x 20 candidates (10 same-world, 10 different-world); default gloc_fpfh_params; medians of {a.reps}, one box")

    # ---- feature build per scan (normals + lists + SPFH + FPFH) ---------------------------------------------------
    r = rows[0]
    t_full, t_feat = [], []
    for i in r["raw"][:6]:
        s = store.add_approx_voxel(i, a.leaf)
        t0 = time.perf_counter()
        store.build_fpfh(s, 10, 16)
        t_full.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        store.build_fpfh(s, 10, 12)      # the normals stay: lists + SPFH + FPFH alone
        t_feat.append((time.perf_counter() - t0) * 1e3)
        store.release(s)
    say(f"feature build per filtered scan (host time, synchronous): normals + features median {np.median(t_full[1:]):.3f} ms, "
        f"features alone (normals present) {np.median(t_feat[1:]):.3f} ms")
    t_raw = []
    for i in r["raw"][:3]:
        s = store.add_variant(i)
        t0 = time.perf_counter()
        store.build_fpfh(s, 10, 16)
        t_raw.append((time.perf_counter() - t0) * 1e3)
        store.release(s)
    say(f"feature build on an unfiltered scan ({store.points(r['raw'][0])} points), normals + features: median {np.median(t_raw[1:]):.3f} ms")
    if a.support:
        radius_builds(a, capi, store, r, say)
    if a.keypoints:
        keypoint_builds(a, capi, store, r, say)
    if a.build_only:
        reg.close()
        store.close()
        return
    for row in rows:
        for t in [row["q"]] + row["db"]:
            store.build_fpfh(t, 10, 16)

    # ---- matcher, RANSAC (profiler on), end to end (profiler off) ------------------------------------------------------
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    for mutual in (1, 0):
        prm = capi.default_fpfh_params(mutual=mutual)
        reg.fpfh_batch(r["q"], r["db"], params=prm)
        reg.profile_reset()
        for _ in range(a.reps):
            reg.fpfh_batch(r["q"], r["db"], params=prm)
        say(f"20 candidates, mutual = {mutual}, profiler on, per batch:")
        for k in ("fpfh_match", "fpfh_pairs", "ransac_hyp", "ransac_score", "accum", "solve"):
            tot, cnt = reg.profile(k)
            if cnt:
                say(f"  {k:12s} {tot / a.reps:8.3f} ms  {cnt / a.reps:5.1f} launches")
        tot, _ = reg.profile("fpfh_match")
        pairs = sum(n_q * n for n in n_db) * (2 if mutual else 1)
        ops = pairs * 99.0                                        # 33 x (subtract, multiply, add), un-fused
        ms = tot / a.reps
        say(f"  matcher: {ms / 20:.4f} ms per job; {pairs / 1e6:.1f} M row pairs, {ops / (ms * 1e-3) / 1e12:.2f} Tflop/s un-fused = "
            f"{100.0 * ops / (ms * 1e-3) / PEAK_FP32_VECTOR:.1f} % of the fp32 vector peak ({PEAK_FP32_VECTOR / 1e12:.1f} Tflop/s, fma = 2)")
    reg.set_option(capi.REG_OPT_PROFILE, 0)
    for mutual in (1, 0):
        prm = capi.default_fpfh_params(mutual=mutual)
        m20, lo20 = med(lambda: reg.fpfh_batch(r["q"], r["db"], params=prm), a.reps)
        m1, lo1 = med(lambda: reg.fpfh_batch(r["q"], r["db"][:1], params=prm), a.reps)
        say(f"end to end (features present), mutual = {mutual}: 20 candidates median {m20:.2f} ms (min {lo20:.2f}), 1 candidate {m1:.2f} ms (min {lo1:.2f})")

    # ---- located within 1 m / 5 degrees: this stage against the nearest-neighbour RANSAC stage from the identity -------------
    def located(T, ok, truth):
        n = 0
        for c in range(10):
            e = pose_error(T[c], truth[c])
            n += bool(ok[c]) and e[0] <= OK_T and e[1] <= OK_R
        return n

    tot_f = tot_b = acc_f = acc_b = 0
    errs = []
    for row in rows:
        g = reg.fpfh_batch(row["q"], row["db"])
        b = reg.batch_ids(row["q"], row["db"], params=capi.default_reg_params(icp_iters=0))
        tot_f += located(g["T"], g["ok"], row["truth"])
        tot_b += located(b["T"], b["ok"], row["truth"])
        acc_f += int(np.sum(g["ok"][10:]))
        acc_b += int(np.sum(b["ok"][10:]))
        errs += [pose_error(g["T"][c], row["truth"][c]) for c in range(10)]
        say(f"  query: pairs {g['n_pairs'].tolist()} inliers {g['inliers'].tolist()}")
    n_same = 10 * a.queries
    say(f"located within {OK_T} m / {OK_R} deg, same-world jobs: fpfh {tot_f} of {n_same}; nearest-neighbour RANSAC stage from the identity {tot_b} of {n_same}")
    say(f"different-world jobs reported ok: fpfh {acc_f} of {n_same} (min_inlier_ratio 0: plausibility is left to the refinement); "
        f"nearest-neighbour stage {acc_b} of {n_same} (min_inlier_ratio 0.3)")
    say("fpfh pose error, same-world jobs, median (max): %.3f (%.3f) m, %.3f (%.3f) deg"
        % (np.median([e[0] for e in errs]), max(e[0] for e in errs), np.median([e[1] for e in errs]), max(e[1] for e in errs)))
    mb, lob = med(lambda: reg.batch_ids(rows[0]["q"], rows[0]["db"], params=capi.default_reg_params(icp_iters=0)), a.reps)
    say(f"baseline, the RANSAC stage of gloc_reg_batch_ids on the same filtered scans from the identity, 20 candidates: median {mb:.2f} ms (min {lob:.2f})")
    if a.support:
        radius_jobs(a, capi, store, reg, rows, located, say)
    if a.keypoints:
        keypoint_jobs(a, capi, store, reg, rows, located, say)
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def radius_builds(a, capi, store, r, say):
    """Build time, k-mode and radius support side by side on the same scans: a warm-up, then the median of --reps."""
    def timed(make, build):
        t = []
        for _ in range(a.reps + 1):
            s = make()
            t0 = time.perf_counter()
            build(s)
            t.append((time.perf_counter() - t0) * 1e3)
            store.release(s)
        return float(np.median(t[1:]))

    dflt, raw = capi.default_fpfh_radius_params(**SUPPORTS["default"]), capi.default_fpfh_radius_params(**SUPPORTS["raw"])
    filt = lambda: store.add_approx_voxel(r["raw"][1], a.leaf)  # noqa: E731
    full = lambda: store.add_variant(r["raw"][1])  # noqa: E731
    n_f, n_r = store.points(r["db"][0]), store.points(r["raw"][1])
    say(f"radius support, feature build (normals + lists + SPFH + FPFH, host time, synchronous), warm-up + median of {a.reps}:")
    k_f, r_f = timed(filt, lambda s: store.build_fpfh(s, 10, 16)), timed(filt, lambda s: store.build_fpfh_radius(s, dflt))
    say(f"  filtered scan ({n_f} points): k-mode (10, 16) {k_f:.3f} ms; radius default (1.0 m / 30, 2.5 m / 100) {r_f:.3f} ms = {r_f / k_f:.1f} x")
    k_r, r_r = timed(full, lambda s: store.build_fpfh(s, 10, 16)), timed(full, lambda s: store.build_fpfh_radius(s, raw))
    say(f"  raw scan ({n_r} points): k-mode (10, 16) {k_r:.3f} ms; radius raw (0.5 m / 30, 1.0 m / 100) {r_r:.3f} ms = {r_r / k_r:.1f} x")
    s = filt()
    idx, _, cnt = store.radius_neighbors(s, dflt.feature_radius, dflt.feature_max_nn)
    _, _, ncnt = store.radius_neighbors(s, dflt.normal_radius, dflt.normal_max_nn)
    say(f"  filtered scan, default support: neighbourhood sizes median (max) normals {int(np.median(ncnt))} ({int(ncnt.max())}), features "
        f"{int(np.median(cnt))} ({int(cnt.max())}); lists cut by max_nn: normals {100.0 * np.mean(ncnt > dflt.normal_max_nn):.1f} %, features "
        f"{100.0 * np.mean(cnt > dflt.feature_max_nn):.1f} %; points below normal_min_nn {100.0 * np.mean(ncnt < dflt.normal_min_nn):.1f} %")
    store.release(s)


def table_row(rows, located, n_same, say, label, call):
    """One row of the localization table: the 40 jobs through call(row)."""
    loc = acc = 0
    errs, inl_same, inl_diff, pairs = [], [], [], []
    for row in rows:
        g = call(row)
        loc += located(g["T"], g["ok"], row["truth"])
        acc += int(np.sum(g["ok"][10:]))
        errs += [pose_error(g["T"][c], row["truth"][c]) for c in range(10)]
        inl_same += g["inliers"][:10].tolist()
        inl_diff += g["inliers"][10:].tolist()
        pairs += g["n_pairs"].tolist()
    say(f"  {label:28s} located {loc:2d} of {n_same}; error median {np.median([e[0] for e in errs]):.3f} m {np.median([e[1] for e in errs]):.3f} deg; "
        f"inliers same-world median {int(np.median(inl_same))} ({min(inl_same)} .. {max(inl_same)}), different-world median "
        f"{int(np.median(inl_diff))} ({min(inl_diff)} .. {max(inl_diff)}); different-world ok {acc} of {n_same}; pairs median {int(np.median(pairs))}")


def radius_jobs(a, capi, store, reg, rows, located, say):
    """The 40 jobs under each support, through RANSAC and through the graph, beside k-mode from the same scans."""
    n_same = 10 * a.queries
    run = lambda label, call: table_row(rows, located, n_same, say, label, call)  # noqa: E731

    say(f"located within {OK_T} m / {OK_R} deg of the {n_same} same-world jobs, k-mode and radius supports, same scans, same run:")
    run("k-mode (10, 16), RANSAC", lambda row: reg.fpfh_batch(row["q"], row["db"]))
    run("k-mode (10, 16), graph", lambda row: reg.fpfh_graph_batch(row["q"], row["db"]))
    for name in ("default", "tight"):
        sup = capi.default_fpfh_radius_params(**SUPPORTS[name])
        tag = f"{sup.normal_radius:g} m / {sup.normal_max_nn}, {sup.feature_radius:g} m / {sup.feature_max_nn}"
        run(f"radius {tag}, RANSAC", lambda row: reg.fpfh_batch(row["q"], row["db"], support=sup))
        run(f"radius {tag}, graph", lambda row: reg.fpfh_graph_batch(row["q"], row["db"], support=sup))
        m20, lo20 = med(lambda: reg.fpfh_batch(rows[0]["q"], rows[0]["db"], support=sup), a.reps)
        say(f"  radius {tag}: end to end (features present), 20 candidates, RANSAC: median {m20:.2f} ms (min {lo20:.2f})")
    for row in rows:                                                      # (leave the scans as the tool's other lines expect them)
        for t in [row["q"]] + row["db"]:
            store.build_fpfh(t, 10, 16)
    m20, lo20 = med(lambda: reg.fpfh_batch(rows[0]["q"], rows[0]["db"]), a.reps)
    say(f"  k-mode: end to end (features present), 20 candidates, RANSAC: median {m20:.2f} ms (min {lo20:.2f})")


def keypoint_builds(a, capi, store, r, say):
    """The keypoint build on a filtered scan beside the feature builds of the same run: a warm-up, then the median of --reps."""
    def timed(make, build):
        t = []
        for _ in range(a.reps + 1):
            s = make()
            t0 = time.perf_counter()
            build(s)
            t.append((time.perf_counter() - t0) * 1e3)
            store.release(s)
        return float(np.median(t[1:]))

    iss, dflt = capi.default_iss_params(), capi.default_fpfh_radius_params()
    filt = lambda: store.add_approx_voxel(r["raw"][1], a.leaf)  # noqa: E731

    def with_features():
        s = filt()
        store.build_fpfh(s, 10, 16)
        return s

    n_f = store.points(r["db"][0])
    k_f, r_f = timed(filt, lambda s: store.build_fpfh(s, 10, 16)), timed(filt, lambda s: store.build_fpfh_radius(s, dflt))
    kp, kp_g = timed(filt, lambda s: store.build_keypoints(s, iss)), timed(with_features, lambda s: store.build_keypoints(s, iss))
    say(f"ISS keypoints (salient {iss.salient_radius:g} m / {iss.max_nn}, min {iss.min_nn}, non-max {iss.non_max_radius:g} m, gammas {iss.gamma_21:g} "
        f"{iss.gamma_32:g}), build on a filtered scan ({n_f} points), host time, synchronous, warm-up + median of {a.reps}:")
    say(f"  keypoints (search + saliency + suppression + list) {kp:.3f} ms; with features present (+ the gather of their rows) {kp_g:.3f} ms; "
        f"feature build of the same run: k-mode (10, 16) {k_f:.3f} ms, radius default {r_f:.3f} ms")
    s = filt()
    sal, _ = store.iss_saliency(s, iss)
    _, _, cnt = store.radius_neighbors(s, iss.salient_radius, iss.max_nn)
    store.build_keypoints(s, iss)
    say(f"  that scan: neighbourhood within {iss.salient_radius:g} m median {int(np.median(cnt))} (max {int(cnt.max())}), lists cut by max_nn "
        f"{100.0 * np.mean(cnt > iss.max_nn):.1f} %, below min_nn {100.0 * np.mean(cnt < iss.min_nn):.1f} %; salient {int((sal > 0).sum())} of {len(sal)}; "
        f"K = {len(store.keypoints(s))}")
    store.release(s)


def keypoint_jobs(a, capi, store, reg, rows, located, say):
    """Matcher and batch time with and without keypoints, and the six rows of the localization table each without and with."""
    n_same = 10 * a.queries
    iss = capi.default_iss_params()
    r = rows[0]
    for row in rows:
        for t in [row["q"]] + row["db"]:
            store.build_fpfh(t, 10, 16)
            store.build_keypoints(t, iss)
    ks = [[len(store.keypoints(t)) for t in [row["q"]] + row["db"]] for row in rows]
    say(f"keypoints per scan at the defaults: queries {[k[0] for k in ks]}, places {min(min(k[1:]) for k in ks)} .. {max(max(k[1:]) for k in ks)} "
        f"(median {int(np.median([x for k in ks for x in k[1:]]))}) of {store.points(r['q'])} / {min(store.points(t) for t in r['db'])} .. "
        f"{max(store.points(t) for t in r['db'])} points")
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    for label, kw in (("all points", {}), ("keypoints", dict(keypoints=iss))):
        reg.fpfh_batch(r["q"], r["db"], **kw)
        reg.profile_reset()
        for _ in range(a.reps):
            reg.fpfh_batch(r["q"], r["db"], **kw)
        parts = {k: reg.profile(k)[0] / a.reps for k in ("fpfh_match", "fpfh_pairs", "ransac_hyp", "ransac_score", "accum", "solve")}
        say(f"20 candidates, k-mode features, mutual = 1, profiler on, per batch, {label}: fpfh_match {parts['fpfh_match']:.3f} ms, fpfh_pairs "
            f"{parts['fpfh_pairs']:.3f} ms, ransac_hyp {parts['ransac_hyp']:.3f}, ransac_score {parts['ransac_score']:.3f}, refit "
            f"{parts['accum'] + parts['solve']:.3f}")
    reg.set_option(capi.REG_OPT_PROFILE, 0)
    for label, kw in (("all points", {}), ("keypoints", dict(keypoints=iss))):
        m20, lo20 = med(lambda: reg.fpfh_batch(r["q"], r["db"], **kw), a.reps)
        m1, lo1 = med(lambda: reg.fpfh_batch(r["q"], r["db"][:1], **kw), a.reps)
        g20, glo20 = med(lambda: reg.fpfh_graph_batch(r["q"], r["db"], **kw), a.reps)
        say(f"end to end (features and keypoints present), k-mode, {label}: RANSAC 20 candidates median {m20:.2f} ms (min {lo20:.2f}), 1 candidate "
            f"{m1:.2f} ms (min {lo1:.2f}); graph 20 candidates median {g20:.2f} ms (min {glo20:.2f})")
    say(f"located within {OK_T} m / {OK_R} deg of the {n_same} same-world jobs, each row without and with keypoints, same scans, same run:")
    run = lambda label, call: table_row(rows, located, n_same, say, label, call)  # noqa: E731
    for kp_label, kw in (("", {}), (" + keypoints", dict(keypoints=iss))):
        run("k-mode (10, 16), RANSAC" + kp_label, lambda row: reg.fpfh_batch(row["q"], row["db"], **kw))
        run("k-mode (10, 16), graph" + kp_label, lambda row: reg.fpfh_graph_batch(row["q"], row["db"], **kw))
    for name in ("default", "tight"):
        sup = capi.default_fpfh_radius_params(**SUPPORTS[name])
        tag = f"{sup.normal_radius:g} m / {sup.normal_max_nn}, {sup.feature_radius:g} m / {sup.feature_max_nn}"
        for kp_label, kw in (("", {}), (" + keypoints", dict(keypoints=iss))):
            run(f"radius {tag}, RANSAC" + kp_label, lambda row: reg.fpfh_batch(row["q"], row["db"], support=sup, **kw))
            run(f"radius {tag}, graph" + kp_label, lambda row: reg.fpfh_graph_batch(row["q"], row["db"], support=sup, **kw))
        m20, lo20 = med(lambda: reg.fpfh_batch(r["q"], r["db"], support=sup, keypoints=iss), a.reps)
        say(f"  radius {tag} + keypoints: end to end, 20 candidates, RANSAC: median {m20:.2f} ms (min {lo20:.2f})")
    for row in rows:                                                      # (leave the scans as the tool's other lines expect them)
        for t in [row["q"]] + row["db"]:
            store.build_fpfh(t, 10, 16)


if __name__ == "__main__":
    main()
