"""What the robust weighting costs: the accumulate and solve kernels of point-to-plane, generalized and voxelized
generalized ICP through the plain entries and through the robust entries of every kind, from the handle's profile
(gloc_reg_profile: HIP events around every launch), on the headline scan size -- tests/gn_cases.py's `full_s` (~122 k
points) against 20 copies of `full_t`.

    python tools/robust_timing.py [--passes 10] [--tree DIR] [--out FILE]

A warm-up call, then 5 calls: per kernel the median over the 5 of the mean time per launch, and the spread (min .. max).
--tree DIR measures another checkout's build (its gloc3d_amd package and library) with this script: the parent commit's,
to compare the plain entries across a change.  A build without the robust entries is measured on the plain ones alone.
The end-to-end line (host time of a call, profiler off) shows what the accumulate kernel is beside: the 1-NN search of the
same pass."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
KINDS = ("huber", "cauchy", "tukey", "geman_mcclure")
# a scale per method at which the weights are neither all 1 nor all 0: 0.1 m, in the method's units (include/gloc3d.h)
SCALE = {"p2l": 0.1, "gicp": 2.24, "vgicp": 2.24}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gn_cases as GC
    from gloc3d_amd import capi
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    robust = hasattr(capi, "RobustParams")
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    src = store.add(GC.cloud("full_s"))
    tgts = [store.add(GC.cloud("full_t")) for _ in range(20)]
    for t in [src] + tgts:
        store.build_normals(t, GC.NORMAL_K)
    init = np.tile((GC._se3(1.5, (0.3, -0.1, 0.0)) @ GC._se3(0.5, (0.1, 0.05, 0.01))).astype(np.float32), (20, 1, 1))
    say(f"package: {os.path.dirname(capi.__file__)}; robust entries: {'yes' if robust else 'no'}")
    say(f"{store.points(src)} source points against 20 targets of {store.points(tgts[0])}; {a.passes} passes, gate 1 m, no stop test; "
        f"a warm-up and {REPS} calls, per launch: median of the calls' means (min .. max)")

    def call(m, kind):
        prm = getattr(capi, "default_%s_params" % m)(max_iters=a.passes, max_corr_dist=1.0)
        kw = {}
        if kind != "plain":
            kw["robust"] = capi.default_robust_params(kind=1 + KINDS.index(kind), scale=SCALE[m])
        return getattr(reg, m + "_batch")(src, tgts, init_T=init, params=prm, **kw)

    fams = {"p2l": ("p2l_accum", "p2l_solve", "nn"), "gicp": ("gicp_accum", "gicp_solve", "nn"), "vgicp": ("vgicp_accum", "vgicp_solve")}
    for m in ("p2l", "gicp", "vgicp"):
        for kind in ("plain",) + (KINDS if robust else ()):
            reg.set_option(capi.REG_OPT_PROFILE, 1)
            call(m, kind)
            per = {k: [] for k in fams[m]}
            for _ in range(REPS):
                reg.profile_reset()
                call(m, kind)
                for k in fams[m]:
                    tot, cnt = reg.profile(k)
                    per[k].append(1e3 * tot / max(cnt, 1))
            reg.set_option(capi.REG_OPT_PROFILE, 0)
            call(m, kind)
            t = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                call(m, kind)
                t.append((time.perf_counter() - t0) * 1e3)
            say(f"{m:5s} {kind:13s} " + "  ".join(f"{k} {np.median(v):8.1f} us ({min(v):.1f} .. {max(v):.1f})" for k, v in per.items())
                + f"  | end to end {np.median(t):.2f} ms ({min(t):.2f} .. {max(t):.2f})")
    reg.close()
    store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
