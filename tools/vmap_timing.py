"""Resident voxel maps against the per-call voxel build, on tools/vgicp_timing.py's kind of scans (distinct 64 x 2000
ray-casts along the road world, a query and 20 places):

  (a) gloc_reg_vgicp_pairs (builds the 20 targets' voxels in the call: the baseline, measured in this run) against
      gloc_reg_vgicp_vmap on 20 maps built once, 5 and 10 passes, neighbors 1 and 7, the two alternating, medians;
  (b) one insert of a full scan into a map that already holds 1, 10 and 50 scans: host time of the call and its split by
      the handle's HIP-event profiler (the contribution's build, the count of new keys, the merge);
  (c) a prune by age of about half of such a map (the age the voxels' median stamp has passed), with its split.

    python tools/vmap_timing.py [--reps 21] [--map-reps 3] [--resolution 1.0] [--out FILE]
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
    ap.add_argument("--map-reps", type=int, default=3)
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

    def ms(f):
        """host time of the call f() in milliseconds"""
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    # ---- (a) 20 places: voxels built in the call against maps built once --------------------------------------------
    at = 60
    q_pose = traj[at] @ synth.se3(rng.uniform(-3, 3), (rng.uniform(-0.4, 0.4), rng.uniform(-0.5, 0.5), 0.02))
    same = [traj[at + d] @ wobble() for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]
    diff = [traj[at + d] @ wobble() for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]
    ids = store.add_raycast(wa, [q_pose] + same, np.arange(1, 12, dtype=np.uint64))
    ids += store.add_raycast(wb, diff, np.arange(12, 22, dtype=np.uint64))
    q, db = ids[0], ids[1:]
    for t in ids:
        store.build_normals(t, 10)
    # starts a tracker would have: 0.1 m and 1 degree off the truth for the same-world places, the same offset elsewhere
    off = synth.se3(1.0, (0.10, -0.05, 0.02))
    init = np.stack([(np.linalg.inv(T) @ q_pose @ off).astype(np.float32) for T in same + diff])
    mp = capi.default_vmap_params(resolution=a.resolution, capacity=1 << 15)
    t0 = time.perf_counter()
    maps = [reg.vmap_create(mp) for _ in db]
    for m, t in zip(maps, db):
        reg.vmap_insert(m, [t])
    built = (time.perf_counter() - t0) * 1e3
    nv = [reg.vmap_info(m)["n_voxels"] for m in maps]
    say(f"scans: {store.points(q)} points (query), {store.points(db[0])} (a place); 20 places, voxels of {a.resolution:g} m: {min(nv)} .. {max(nv)} "
        f"per place; the 20 maps made once in {built:.1f} ms (create + insert, normals there already)")
    for passes in (5, 10):
        for nb in (1, 7):
            prm = capi.default_vgicp_params(max_iters=passes, neighbors=nb, resolution=a.resolution)
            per_call = lambda: reg.vgicp_pairs([q] * 20, db, init, prm)
            resident = lambda: reg.vgicp_vmap([q] * 20, maps, init, prm)
            x, y = per_call(), resident()
            equal = all(np.array_equal(u, v) for u, v in zip(x, y))
            tp, tr = [], []
            for _ in range(a.reps):                                        # alternating: both see the same machine
                tp.append(ms(per_call))
                tr.append(ms(resident))
            say(f"(a) {passes:2d} passes, neighbors {nb}: vgicp_pairs median {np.median(tp):.3f} ms (min {min(tp):.3f}), vgicp_vmap median "
                f"{np.median(tr):.3f} ms (min {min(tr):.3f}); difference {np.median(tp) - np.median(tr):.3f} ms; {a.reps} runs each, alternating; "
                f"outputs {'bit-identical' if equal else 'DIFFERENT'}")
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    prm = capi.default_vgicp_params(max_iters=5, neighbors=7, resolution=a.resolution)
    for name, call, fams in (("vgicp_pairs", lambda: reg.vgicp_pairs([q] * 20, db, init, prm), ("vgicp_voxels", "vgicp_accum", "vgicp_solve")),
                             ("vgicp_vmap", lambda: reg.vgicp_vmap([q] * 20, maps, init, prm), ("vgicp_voxels", "vgicp_accum", "vgicp_solve"))):
        call()
        reg.profile_reset()
        for _ in range(5):
            call()
        say(f"    {name}, 5 passes, neighbors 7, profiler on, per call: " + ", ".join(f"{k} {reg.profile(k)[0] / 5:.3f} ms" for k in fams))
    reg.set_option(capi.REG_OPT_PROFILE, 0)

    # ---- (b), (c) a map that grows along the road ------------------------------------------------------------------------
    n_scans = 52
    poses = [traj[100 + k] for k in range(n_scans)]
    road = store.add_raycast(wa, poses, np.arange(100, 100 + n_scans, dtype=np.uint64))
    for t in road:
        store.build_normals(t, 10)
    into = np.stack([(np.linalg.inv(poses[0]) @ P).astype(np.float32) for P in poses])
    big = capi.default_vmap_params(resolution=a.resolution, capacity=1 << 19)
    fams = ("vmap_contrib", "vmap_count", "vmap_merge")
    host = {1: [], 10: [], 50: []}
    split = {k: {f: [] for f in fams} for k in host}
    grown = {}
    reg.set_option(capi.REG_OPT_PROFILE, 1)
    for rep in range(a.map_reps):
        m = reg.vmap_create(big)
        for k in range(n_scans - 1):
            if k in host:                                                  # the map holds k scans: time the next insert
                reg.profile_reset()
                host[k].append(ms(lambda: reg.vmap_insert(m, [road[k]], into[k:k + 1])))
                for f in fams:
                    split[k][f].append(reg.profile(f)[0])
                grown[k] = (reg.vmap_info(m)["n_voxels"], store.points(road[k]))
            else:
                reg.vmap_insert(m, [road[k]], into[k:k + 1])
        if rep + 1 < a.map_reps:
            reg.vmap_destroy(m)
    for k in sorted(host):
        say(f"(b) insert of a scan of {grown[k][1]} points into a map of {k} scans ({grown[k][0]} voxels after it): host time of the call median "
            f"{np.median(host[k]):.3f} ms, of which on the device " + ", ".join(f"{f} {np.median(split[k][f]):.3f} ms" for f in fams)
            + f" (profiler on; {a.map_reps} maps); between count and merge the host waits once for the number of new keys")
    info = reg.vmap_info(m)
    pf = ("vmap_prune_flags", "vmap_prune_compact", "vmap_prune_table")
    reg.profile_reset()
    # the age of the voxels' median stamp (from the exported stamps): what is older than the median goes
    age = max(1, int(info["n_inserts"] - np.median(reg.vmap_voxels(m)["stamp"])))
    removed = [0]
    t = ms(lambda: removed.__setitem__(0, reg.vmap_prune(m, max_age=age)))
    say(f"(c) prune by age ({age} inserts) of a map of {info['n_inserts']} scans, {info['n_voxels']} voxels: {removed[0]} removed "
        f"({100.0 * removed[0] / max(info['n_voxels'], 1):.0f} %), host time {t:.3f} ms, on the device "
        + ", ".join(f"{f} {reg.profile(f)[0]:.3f} ms" for f in pf) + " (profiler on, one run)")
    reg.set_option(capi.REG_OPT_PROFILE, 0)
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
