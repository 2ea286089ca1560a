"""The pose graph's closure selection (gloc_pgo_consistency) beside the optimisation it protects, at L = 1024, 4096 and 16384
candidate closures:

  consistency   one call on the closed-form family of tests/pcm_cases.py (groups of closures that agree among themselves,
                the largest 48 % of L), default parameters: host time of the synchronous call, then its kernels by family
                from the handle's HIP-event profiler (pgo_consistency and its parts _pairs, _score, _clique), a run of
                its own
  optimize      one gloc_pgo_optimize call, default parameters, on pgo_cases.graph(L / 8 nodes, L closures, noise 1): the
                optimisation of a graph with that many closures

    python tools/pcm_timing.py [--reps 5] [--sizes 1024,4096,16384] [--out FILE]

Medians of --reps calls after a warm one, one box, host arrays in and out.  The clique search takes a step per member of
the clique it grows, so the family's 48 % group is its hard case, not its typical one; the second consistency line per
size is the same L with every closure in a group of 16.  No threshold is set anywhere.
"""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FAMILIES = ("pgo_consistency", "pgo_consistency_pairs", "pgo_consistency_score", "pgo_consistency_clique")
OPT_FAMILIES = ("pgo_setup", "pgo_linearize", "pgo_gather", "pgo_pcg", "pgo_step")


def small_groups(c, size=16):
    """The family's closures regrouped into groups of `size` by position (Z recut): cliques of a realistic size."""
    import pgo_cases as G
    L = len(c["src"])
    rng = np.random.default_rng(5)
    group = np.arange(L) // size
    motions = [np.eye(4)] + [G.se3(rng.normal(size=3) * 0.2, [20.0 * g, 7.0 * (g % 13), 0.0]) for g in range(1, int(group.max()) + 1)]
    P = c["poses"]
    Z = np.array([np.linalg.inv(P[j]) @ motions[g] @ P[i] for i, j, g in zip(c["src"], c["tgt"], group)]).astype(np.float32)
    return dict(c, Z=Z, group=group)


def timed(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pcm_cases as PC
    import pgo_cases as G
    from gloc3d_amd import capi
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    opt = capi.PoseGraphOptimizer()
    say(f"gloc_pgo_consistency and gloc_pgo_optimize, default parameters, host arrays in and out; medians of {a.reps} calls after a warm one; "
        f"one box ({socket.gethostname()})")
    for L in [int(x) for x in a.sizes.split(",")]:
        big = PC.cliques(L)
        for label, c in (("largest group %d" % big["sizes"][0], big), ("groups of 16", small_groups(big))):
            call = lambda: opt.consistency(c["poses"], c["src"], c["tgt"], c["Z"], c["info"], None)   # noqa: E731
            d = call()
            t = timed(call, a.reps)
            say(f"L = {L:5d} consistency, {label}: clique {d['clique_size']}, median {np.median(t):9.2f} ms  (min {min(t):.2f}, max {max(t):.2f})")
            opt.set_profile(1)
            call()
            per = {k: [] for k in FAMILIES}
            for _ in range(a.reps):
                opt.profile_reset()
                call()
                for k in FAMILIES:
                    per[k].append(opt.profile(k))
            opt.set_profile(0)
            for k in FAMILIES:
                say(f"    {k:24s} {float(np.median([p[0] for p in per[k]])):10.3f} ms  {float(np.median([p[1] for p in per[k]])):4.1f} scopes")
        g = G.graph(max(L // 8, 16), L, seed=31, noise=1.0)
        run = lambda: opt.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"])   # noqa: E731
        res = run()[3]
        t = timed(run, a.reps)
        say(f"L = {L:5d} optimize, {len(g['init'])} nodes, {len(g['src'])} edges: status {res.status}, {res.iters} attempts ({res.accepted} accepted), "
            f"{res.pcg_iters} PCG iterations in the last, median {np.median(t):9.2f} ms  (min {min(t):.2f}, max {max(t):.2f})")
        opt.set_profile(1)
        opt.profile_reset()
        run()
        say("    " + ", ".join(f"{k} {opt.profile(k)[0]:.2f} ms" for k in OPT_FAMILIES))
        opt.set_profile(0)
    opt.close()


if __name__ == "__main__":
    main()
