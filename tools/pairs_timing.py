"""What the pair-list entries buy: 25 sources x 20 targets of headline-size ray-casts (gloc_scan_store_add_raycast_batch,
~122 k points each) refined as ONE gloc_reg_<m>_pairs call of 500 rows, against 25 gloc_reg_<m>_batch_ids calls of 20 on
the same handle and build -- point-to-plane and generalized ICP, max_iters = 20, max_corr_dist = 1.0.

    python tools/pairs_timing.py [--sources 25] [--targets 20] [--reps 5] [--out FILE]

The two forms alternate, --reps times each after a warm-up of both; the time is a host clock around the synchronous calls,
with the profiler off.  One more run of each with the profiler on gives the nn, accumulate and solve totals
(gloc_reg_profile).  The rows of the two forms are compared bit for bit on the way."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=25)
    ap.add_argument("--targets", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gloc3d_amd import capi, synth

    world = synth.make_world(1001)
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    S, N = a.sources, a.targets
    src_pose = [synth.se3(1.0 * i, (0.3 * i, -0.1 * i, 0.0)) for i in range(S)]
    tgt_pose = [synth.se3(-1.0 * j, (0.4 * j, 0.2 * j, 0.0)) for j in range(N)]
    src = store.add_raycast(world, src_pose, np.arange(7000, 7000 + S, dtype=np.uint64))
    tgt = store.add_raycast(world, tgt_pose, np.arange(8000, 8000 + N, dtype=np.uint64))
    for t in tgt:
        store.build_target_index(t)
    for s in src + tgt:
        store.build_normals(s, 10)
    off = synth.se3(0.5, (0.1, 0.05, 0.01))
    init = np.stack([[np.linalg.inv(tgt_pose[j]) @ src_pose[i] @ off for j in range(N)] for i in range(S)]).astype(np.float32)   # [S, N, 4, 4]
    pts = [store.points(s) for s in src]
    print("scans: %d sources of %d .. %d points, %d targets" % (S, min(pts), max(pts), N))
    src_ids = np.repeat(np.asarray(src, np.uint32), N)
    tgt_ids = np.tile(np.asarray(tgt, np.uint32), S)
    res = {}
    for method in ("p2l", "gicp"):
        prm = getattr(capi, "default_%s_params" % method)(max_iters=a.iters, max_corr_dist=1.0)
        pairs = lambda: getattr(reg, method + "_pairs")(src_ids, tgt_ids, init_T=init.reshape(S * N, 4, 4), params=prm)
        singles = lambda: [getattr(reg, method + "_batch")(src[i], tgt, init_T=init[i], params=prm) for i in range(S)]
        one, many = pairs(), singles()                                        # the warm-up of both, and the rows compared
        same = all((np.concatenate([m[k] for m in many]).view(np.uint32) == one[k].view(np.uint32)).all() for k in range(4))
        t_pairs, t_singles = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pairs()
            t1 = time.perf_counter()
            singles()
            t2 = time.perf_counter()
            t_pairs.append((t1 - t0) * 1e3)
            t_singles.append((t2 - t1) * 1e3)
        prof = {}
        reg.set_option(capi.REG_OPT_PROFILE, 1)
        for name, f in (("pairs", pairs), ("singles", singles)):
            reg.profile_reset()
            f()
            prof[name] = {k: dict(zip(("ms", "launches"), reg.profile(k))) for k in ("nn", "nn_cold", method + "_accum", method + "_solve")}
        reg.set_option(capi.REG_OPT_PROFILE, 0)
        r = dict(rows_equal_bit_for_bit=bool(same), iters_mean=float(one[2].mean()), status=np.bincount(one[3], minlength=3).tolist(),
                 pairs_ms=sorted(t_pairs), singles_ms=sorted(t_singles), pairs_median_ms=float(np.median(t_pairs)),
                 singles_median_ms=float(np.median(t_singles)), profile=prof)
        res[method] = r
        print("%s: one call of %d rows  median %.2f ms (min %.2f, max %.2f);  %d calls of %d  median %.2f ms (min %.2f, max %.2f);  rows equal: %s"
              % (method, S * N, r["pairs_median_ms"], min(t_pairs), max(t_pairs), S, N, r["singles_median_ms"], min(t_singles), max(t_singles), same))
        for name in ("pairs", "singles"):
            print("   profiler, %-7s: " % name + ",  ".join("%s %.2f ms in %d" % (k, v["ms"], v["launches"]) for k, v in prof[name].items()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    reg.close()
    store.close()


if __name__ == "__main__":
    main()
