"""Inputs shared by tests/test_pairs_cases_cpu.py and tests/test_pairs_gpu.py: the list of (source, target) pairs the
pair-list entries (gloc_reg_{p2l,gicp,vgicp}_pairs) are run on, its two parameter blocks, and the float64 restatements'
verdict on every pair (tests/p2l_ref.py, tests/gicp_ref.py, tests/vgicp_ref.py, run two ways by the rule of
tests/gn_cases.py: the pairs summed forward and reversed, M by numpy.linalg.inv and by the adjugate).  Clouds, ground truth
and the size of the offsets are tests/gn_cases.py's: a guess is truth x offset, at most 2 degrees and 0.3 m off.

The list is ragged on purpose: sources of one point (one lane) to 12.8 k (47 work-groups of 256 slots), every size around
a wave and a work-group, scans that appear as source, as target and as both, a scan against itself, non-finite rows and
duplicates on either side, a target whose normals are all zero, an empty target, a pair out of reach, another world.
Under P1 the jobs stop at different passes -- at the cap, converged at passes 1 to 6, degenerate at once -- so that rows
freeze while others run on; P2 runs every job that is not degenerate to its cap of 4.

Nothing here looks at a device."""
import numpy as np

import gn_cases as GC
import robust_cases as RC
import robust_ref as RR
import vgicp_ref as V

METHODS = RC.METHODS
BLOCKS = {"P1": dict(max_iters=6, max_corr_dist=1.0, trans_eps=2e-3, rot_eps=2e-4), "P2": dict(max_iters=4)}
SIZES = (1, 5, 6, 63, 64, 65, 255, 256, 257)
EYE = "identity"


def _pair(src, tgt, yaw=0.0, t=(0.0, 0.0, 0.0), pitch=0.0, roll=0.0, at=None, only=None):
    return dict(src=src, tgt=tgt, off=(yaw, t, pitch, roll), at=at, only=only)


# (source, target, the guess's offset from the truth); `at`: the guess is that pose x offset instead; `only`: under that block alone
PAIRS = [
    _pair("a2", "a0", yaw=1.0, t=(0.10, -0.05, 0.02)),
    _pair("a3", "a1", yaw=-1.8, t=(-0.15, 0.10, -0.03), roll=0.4),
    _pair("b2", "b0", yaw=0.5, t=(0.20, 0.15, 0.05)),
    _pair("b3", "b1", yaw=-1.5, t=(0.15, -0.20, 0.0)),
    _pair("c2", "c0", yaw=1.8, t=(-0.15, 0.2, 0.05), pitch=0.5),
    _pair("c3", "c1", yaw=-1.0, t=(0.05, 0.02, 0.0)),
] + [_pair("a2_n%d" % k, "a0", yaw=(-1.0) ** i * (0.4 + 0.15 * i), t=(0.02 * i, 0.05 - 0.01 * i, 0.01)) for i, k in enumerate(SIZES)] + [
    _pair("a2_odd", "a0_odd", yaw=0.5, t=(0.05, 0.1, 0.02)),
    _pair("a0_dup", "a0", yaw=1.0, t=(0.1, 0.0, 0.0)),
    _pair("a2", "a0_zn", yaw=1.0, t=(0.1, 0.0, 0.0)),
    _pair("a2", "empty", yaw=1.0, t=(0.1, 0.0, 0.0)),
    _pair("a2", "a0", t=GC.FAR, only="P1"),
    _pair("a2", "b0", at=EYE),
    _pair("a0", "a0", at=EYE),
]
assert len(PAIRS) == 22

# What the comparison against the restatements leaves out -- (method, source, target) -- and no more: six points make an exactly
# determined point-to-plane system, whose two summation orders part at 1e-6 (under P2; under P1 the job is degenerate after
# one update either way).  tests/test_pairs_cases_cpu.py proves that the restatements call every other pair stable, for
# every method and block; the pair stays in every bit-equality test.
LEFT_OUT = {("p2l", "a2_n6", "a0")}
# The jobs that are degenerate at once -- (source, target) -- whatever the block: too few pairs for six unknowns, no target
# point with a normal, no target point, no pair inside the gate.  A voxelized job pairs a point with up to 7 voxels, so five
# points are enough for it, and a target without normals still has voxels (as generalized ICP still has its points).
DEGENERATE = {"p2l": {("a2_n1", "a0"), ("a2_n5", "a0"), ("a2", "a0_zn"), ("a2", "empty"), "far"},
              "gicp": {("a2_n1", "a0"), ("a2_n5", "a0"), ("a2", "empty"), "far"},
              "vgicp": {("a2_n1", "a0"), ("a2", "empty"), "far"}}


def is_far(pair):
    return pair["off"][1] == GC.FAR


def pairs(block):
    """The pairs of a block, in list order."""
    return [p for p in PAIRS if p["only"] in (None, block)]


def guess(pair):
    yaw, t, pitch, roll = pair["off"]
    base = GC.truth(pair["src"], pair["tgt"]) if pair["at"] is None else np.eye(4)
    return (base @ GC._se3(yaw, t, pitch_deg=pitch, roll_deg=roll)).astype(np.float32)


def guesses(prs):
    return np.stack([guess(p) for p in prs])


def robust(method):
    """The robust block of the tests: Cauchy at robust_cases.SCALES, annealed from 4 x the scale by 0.5 per update."""
    return RC.robust(method, RR.CAUCHY, 4.0, 0.5)


def params(method, block):
    """The method's parameter block, every float rounded to the float32 the device holds (robust_cases.params)."""
    return RC.params(dict(method=method, params=BLOCKS[block]))


def case(pair, method, block, rb=None):
    """The pair as a case of gn_cases.run / robust_cases.run."""
    return dict(name="%s_%s_%s_%s" % (pair["src"], pair["tgt"], method, block), method=method, src=pair["src"], tgt=pair["tgt"],
                off=pair["off"], at=None if pair["at"] is None else np.eye(4), params=BLOCKS[block], robust=rb)


def _run_vgicp(pair, block, oracle, second, events):
    prm = params("vgicp", block)
    s, t = pair["src"], pair["tgt"]
    return V.align(GC.cloud(s), GC.normals(s, oracle), GC.cloud(t), GC.normals(t, oracle), init_T=guess(pair),
                   order="reversed" if second else "forward", how="adj" if second else "inv", events=events, **prm)


def run(pair, method, block, oracle, rb=None, second=False, events=None):
    """The restatement's run of a pair; second: the other summation order and the other inverse."""
    if rb is not None:
        return RC.run(case(pair, method, block, rb), oracle, second, events)
    if method == "vgicp":
        return _run_vgicp(pair, block, oracle, second, events)
    return GC.run(case(pair, method, block), oracle, second, events)


_REFS = {}


def reference(pair, method, block, oracle, rb=None):
    """dict(ref, events, floor (m, rad), stable) by the rule of gn_cases.reference; computed once per process."""
    key = (pair["src"], pair["tgt"], pair["off"], method, block, None if rb is None else tuple(sorted(rb.items())))
    if key not in _REFS:
        ev, ev2 = [], []
        r, r2 = run(pair, method, block, oracle, rb, events=ev), run(pair, method, block, oracle, rb, second=True, events=ev2)
        ft, fa = RR.P.pose_err(r["T"], r2["T"])
        stable = bool(ev == ev2 and r["iters"] == r2["iters"] and r["status"] == r2["status"] and np.isfinite(r["T"]).all()
                      and np.isfinite(r2["T"]).all() and 10 * ft <= GC.POSE_CAP and 10 * fa <= GC.POSE_CAP)
        _REFS[key] = dict(ref=r, events=ev, floor=(float(ft), float(fa)), stable=stable)
    return _REFS[key]
