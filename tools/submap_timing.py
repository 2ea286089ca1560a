"""Local-submap timing on device ray-cast scans (not bench.py, not run by the suite): one MI355X, a warm-up, then the median
of >= 10 repetitions, each ending in a device synchronise (every call below returns after one).

  (a) one submap of 5 casts of about 121 000 points at leaf 0.2 m
  (b) a batch of 64 such submaps, with their build_target_index_batch
  (c) batch_ids of one query against 20 single-scan targets and against the 20 submaps of the same places

(a) and (b) stand next to the byte floor -- the members' 12 B/point read once plus the centroids written, at the 6.29 TB/s
copy rate of DESIGN section 3 -- and next to gloc_scan_store_add_approx_voxel over the same input points.  The share of
the sort comes from a kernel trace taken in a run of its own (tracing slows the host), of the single-submap calls alone:

    python tools/submap_timing.py [--reps 10] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o submap -- python tools/submap_timing.py --only s --reps 10
    python tools/submap_timing.py --kernel-trace DIR/.../submap_kernel_trace.csv [--out FILE]    (appends the shares)
"""
import argparse
import csv
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12       # B/s, DESIGN section 3
HALF_WINDOW = 2
N_SUBMAPS = 64


def timed(fn, reps):
    fn()                                                 # warm-up: code objects loaded, scratch grown
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t))


def kernel_shares(path, say):
    """The submap call's kernels in a rocprofv3 kernel_trace.csv of a run with --only s.  A call's pipeline is what runs from
    member_keys_kernel to compact_kernel on the store's one stream; what follows up to the next call indexes the result."""
    groups = {"sort (hist, scan, scatter)": ("segsort::",), "member_keys": ("member_keys_kernel",), "bounds_reduce, narrow_keys": ("bounds_reduce_kernel", "narrow_keys_kernel"),
              "run_stats": ("run_stats_kernel",),
              "flags and flag scans": ("cell_flags_kernel", "scan_sum_kernel", "scan_top_kernel", "scan_apply_kernel", "cell_first_kernel"),
              "compact": ("compact_kernel",)}
    with open(path) as f:
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    tot = {k: 0.0 for k in groups}
    calls, sort_launches, span, index, state = 0, 0, 0.0, 0.0, "before"
    for t0, t1, name in rows:
        if "member_keys_kernel" in name:
            state, calls, start = "in", calls + 1, t0
        if state == "in":
            for k, pats in groups.items():
                if any(p in name for p in pats):
                    tot[k] += t1 - t0
                    sort_launches += k.startswith("sort")
                    break
            if "compact_kernel" in name:
                state, span = "after", span + (t1 - start)
        elif state == "after":
            index += t1 - t0
    mine = sum(tot.values())
    say(f"kernel trace of {calls} single-submap calls, per call: {mine / calls / 1e3:.1f} us in the pipeline's kernels over a span of "
        f"{span / calls / 1e3:.1f} us from the first kernel's start to the last one's end ({sort_launches // calls} sort launches), then "
        f"{index / calls / 1e3:.1f} us of kernels indexing the result")
    for k, v in tot.items():
        say(f"  {k:28s} {v / calls / 1e3:9.1f} us  {100.0 * v / max(mine, 1.0):5.1f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="abc", help="which of the measurements a, b, c to run; s: the single-submap calls alone, for a trace")
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 kernel_trace.csv of a run with --only s: print the shares and stop")
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()

    def say(s):                                          # (line by line: a run that is cut short keeps what it had)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    if a.kernel_trace:
        return kernel_shares(a.kernel_trace, say)
    assert a.reps >= 10, "the report wants the median of >= 10 repetitions"
    from gloc3d_amd import capi, loop_detector, synth
    import torch
    say(f"box: {socket.gethostname()}, {torch.cuda.get_device_name(0)}; {a.reps} repetitions after a warm-up, median (min) of host "
        "times around calls that end in a device synchronise")
    traj, xy = synth.loop_trajectory(400, 328.0)                     # 0.82 m between places, as the benchmark's database
    world = synth.make_road_world(1001, xy)
    store = capi.ScanStore()
    n_places = N_SUBMAPS + 2 * HALF_WINDOW
    P = traj[100:100 + n_places]
    ids = store.add_raycast(world, P, np.arange(n_places, dtype=np.uint64) + 1)
    pts = [store.points(i) for i in ids]
    say(f"{n_places} places {np.linalg.norm(P[1, :3, 3] - P[0, :3, 3]):.2f} m apart, {min(pts)}..{max(pts)} points a cast (64 x 2000 rays)")
    prm = capi.default_submap_params(leaf=0.2)

    def members(i):
        js = range(i - HALF_WINDOW, i + HALF_WINDOW + 1)
        inv_i = np.linalg.inv(P[i])
        return [ids[j] for j in js], np.stack([inv_i @ P[j] for j in js]).astype(np.float32)

    centres = list(range(HALF_WINDOW, HALF_WINDOW + N_SUBMAPS))
    subs = [members(i) for i in centres]
    floor_ms = lambda n_in, n_out: (12.0 * n_in + 12.0 * n_out) / COPY_RATE * 1e3

    if a.only == "s":
        m_ids, m_T = subs[N_SUBMAPS // 2]
        for _ in range(a.reps + 1):
            store.release(store.add_submap(m_ids, m_T, prm))

    if "a" in a.only:
        m_ids, m_T = subs[N_SUBMAPS // 2]
        sid, info = store.add_submap(m_ids, m_T, prm, want_info=True)
        store.release(sid)
        med, mn = timed(lambda: store.release(store.add_submap(m_ids, m_T, prm)), a.reps)
        fl = floor_ms(info["points_in"], info["kept"])
        say(f"(a) one submap of 5 members: {info['points_in']} points in, {info['cells']} cells, {info['kept']} kept: "
            f"{med:.3f} ms ({mn:.3f}); byte floor {fl:.4f} ms = {100 * fl / med:.1f} % of it")
        med_av, mn_av = timed(lambda: [store.release(store.add_approx_voxel(i, 0.2)) for i in m_ids], a.reps)
        n_av = sum(store.points(s) for s in [store.add_approx_voxel(i, 0.2) for i in m_ids])
        say(f"    gloc_scan_store_add_approx_voxel of the same 5 scans, one call each: {med_av:.3f} ms ({mn_av:.3f}), {n_av} points out "
            "(unmerged: five filtered scans, not one map)")

    new = None
    if "b" in a.only or "c" in a.only:
        def build():
            out = store.add_submaps(subs, prm)
            for s in out:
                store.release(s)
        if "b" in a.only:
            new, infos = store.add_submaps(subs, prm, want_info=True)
            n_in, n_out = sum(i["points_in"] for i in infos), sum(i["kept"] for i in infos)
            for s in new:
                store.release(s)
            med, mn = timed(build, a.reps)
            fl = floor_ms(n_in, n_out)
            say(f"(b) batch of {N_SUBMAPS} submaps: {n_in} points in, {n_out} kept: {med:.2f} ms ({mn:.2f}) = {med / N_SUBMAPS:.3f} ms a "
                f"submap; byte floor {fl:.3f} ms = {100 * fl / med:.1f} % of it")

            def build_indexed():
                out = store.add_submaps(subs, prm)
                store.build_target_index_batch(out)
                for s in out:
                    store.release(s)
            med_i, mn_i = timed(build_indexed, a.reps)
            say(f"    with build_target_index_batch of the {N_SUBMAPS} results: {med_i:.2f} ms ({mn_i:.2f}) = {med_i / N_SUBMAPS:.3f} ms a submap")
            say(f"    EXTRAPOLATED, not measured: a database of 4541 places at this rate: {4541 * med_i / N_SUBMAPS / 1e3:.2f} s "
                f"({4541 * med / N_SUBMAPS / 1e3:.2f} s without the target indices)")
            med_av, _ = timed(lambda: [store.release(store.add_approx_voxel(i, 0.2)) for m, _ in subs for i in m], max(a.reps // 3, 3))
            say(f"    gloc_scan_store_add_approx_voxel over the same {n_in} input points ({5 * N_SUBMAPS} calls): {med_av:.2f} ms")

    if "c" in a.only:
        places = centres[20:40]
        new = store.add_submaps([subs[i - HALF_WINDOW] for i in places], prm)
        store.build_target_index_batch(new)
        store.build_target_index_batch([ids[i] for i in places])
        reg = capi.Registrar(store=store)
        qi = places[10]
        q_pose = P[qi] @ synth.se3(3.0, (0.41, 0.35, 0.0))           # between two places, off the lane's centre
        q = store.add_raycast(world, [q_pose], np.array([977], np.uint64))[0]
        rp = capi.default_reg_params()
        gt = [np.linalg.inv(P[i]) @ q_pose for i in places]
        for name, tg in (("single scans", [ids[i] for i in places]), ("submaps", new)):
            res = reg.batch_ids(q, tg, params=rp)
            med, mn = timed(lambda: reg.batch_ids(q, tg, params=rp), a.reps)
            err = [loop_detector.pose_error(g, T) for g, T in zip(gt, res["T"])]
            ok = sum(1 for er, ep in err if ep < 1.0 and er < 5.0)
            say(f"(c) batch_ids of one query ({store.points(q)} points) against 20 {name} ({int(np.mean([store.points(t) for t in tg]))} "
                f"points each on average): {med:.2f} ms ({mn:.2f}); mean position error {np.mean([e[1] for e in err]):.3f} m, "
                f"median {np.median([e[1] for e in err]):.3f} m, rotation {np.mean([e[0] for e in err]):.3f} deg, "
                f"{ok}/20 within 1 m and 5 deg, ok flags {int(res['ok'].sum())}/20")
        reg.close()
    store.close()


if __name__ == "__main__":
    main()
