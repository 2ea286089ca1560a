"""Inputs shared by tests/test_robust_ref_cpu.py and tests/test_robust_gpu.py: the whole-alignment cases of the robust
refinements with the float64 restatement's verdict on each (tests/robust_ref.py run two ways, by the rule of
tests/gn_cases.py: the pairs summed forward and reversed, M by numpy.linalg.inv and by the adjugate), and the
moved-object scene.  Clouds, guesses and ground truth are tests/gn_cases.py's.  Nothing here looks at a device.

The moved-object scene: the source scan "a2" with every point above the ground (z > -1.2 m in the sensor's frame) within
60 degrees of the x axis -- 1151 of its 12788 points, the walls and boxes of one side -- displaced by 0.6 m along y:
an object that has moved between the two visits.  It finds partners inside the 1 m gate that the offset guesses of
gn_cases need, and pulls the plain refinements 3 .. 10 cm off the truth (tests/test_robust_ref_cpu.py prints the figures).

Scales: point-to-plane residuals are metres, so its scales are 0.1 .. 0.3 m; generalized and voxelized ICP's are
e^T M e, 22.4 per metre of normal distance at plane_eps = 1e-3 (include/gloc3d.h), so theirs are those times 22.4."""
import numpy as np

import gn_cases as GC
import robust_ref as RR

METHODS = ("p2l", "gicp", "vgicp")
UNITS = {"p2l": 1.0, "gicp": 22.4, "vgicp": 22.4}                     # of a scale, per metre
SCALES = {RR.HUBER: 0.1, RR.CAUCHY: 0.1, RR.TUKEY: 0.3, RR.GEMAN_MCCLURE: 0.2}    # metres
MOVED = "a2_moved"
MOVED_SHIFT = (0.0, 0.6, 0.0)
VGICP = dict(resolution=1.0, neighbors=7, min_points=1)

_CLOUDS, _NORMALS = {}, {}


def moved_mask(xyz):
    az = np.degrees(np.arctan2(xyz[:, 1], xyz[:, 0]))
    return (np.abs(az) < 60.0) & (xyz[:, 2] > -1.2)


def cloud(name):
    if name != MOVED:
        return GC.cloud(name)
    if name not in _CLOUDS:
        xyz = GC.cloud("a2").copy()
        xyz[moved_mask(xyz)] += np.asarray(MOVED_SHIFT, np.float32)
        _CLOUDS[name] = np.ascontiguousarray(xyz)
    return _CLOUDS[name]


def normals(name, oracle):
    if name != MOVED:
        return GC.normals(name, oracle)
    if name not in _NORMALS:
        xyz = cloud(name)
        _NORMALS[name] = oracle.ground_normals(xyz, oracle.ground_knn(xyz, GC.NORMAL_K)[0])[0]
    return _NORMALS[name]


def truth(src, tgt):
    return GC.truth("a2" if src == MOVED else src, tgt)


def robust(method, kind, start=0.0, anneal=0.0, scale=None):
    """The block of a kind at this file's scale for the method (start: a multiple of the scale, 0 = no schedule)."""
    if kind == RR.NONE:
        return RR.block()
    c = (SCALES[kind] if scale is None else scale) * UNITS[method]
    return RR.block(kind, c, c * start, anneal)


def _case(name, method, src, tgt, rb, yaw=1.0, t=(0.10, -0.05, 0.02), **params):
    return dict(name="%s_%s" % (name, method), method=method, src=src, tgt=tgt, off=(yaw, t, 0.0, 0.0), at=None, params=params, robust=rb)


CASES = []
for _m in METHODS:
    # every kind at a fixed scale, no stop test
    for _k in RR.KINDS:
        CASES.append(_case("a20_" + RR.NAMES[_k], _m, "a2", "a0", robust(_m, _k), max_iters=6, max_corr_dist=1.0))
    # a schedule that settles at update 3 (8 c, 4 c, 2 c, c), the stop test on: a job may stop from update 3 on
    CASES.append(_case("a20_gnc_eps", _m, "a2", "a0", robust(_m, RR.CAUCHY, 8.0, 0.5), max_iters=20, max_corr_dist=1.0, trans_eps=2e-3, rot_eps=2e-4))
    # a schedule that has not settled by the cap: the stop test never counts
    CASES.append(_case("a20_gnc_slow", _m, "a2", "a0", robust(_m, RR.TUKEY, 4.0, 0.9), max_iters=5, max_corr_dist=1.0, trans_eps=1.0, rot_eps=1.0))
    # the moved-object scene: no weights (kind NONE through the robust entries), Cauchy, Tukey
    for _k in (RR.NONE, RR.CAUCHY, RR.TUKEY):
        CASES.append(_case("moved_" + RR.NAMES[_k], _m, MOVED, "a0", robust(_m, _k), max_iters=12, max_corr_dist=1.0))


def guess(case):
    yaw, t, pitch, roll = case["off"]
    return (truth(case["src"], case["tgt"]) @ GC._se3(yaw, t, pitch_deg=pitch, roll_deg=roll)).astype(np.float32)


def params(case):
    """The method's parameter block of a case, every float rounded to the float32 the device holds."""
    p = dict(max_iters=30, max_corr_dist=0.0, trans_eps=0.0, rot_eps=0.0)
    if case["method"] != "p2l":
        p["plane_eps"] = 1e-3
    if case["method"] == "vgicp":
        p.update(VGICP)
    p.update(case["params"])
    return {k: (int(v) if k in ("max_iters", "neighbors", "min_points") else float(np.float32(v))) for k, v in p.items()}


def run(case, oracle, second=False, events=None):
    """The restatement's run of a case; second: the other summation order (and the other inverse)."""
    prm, rb = params(case), case["robust"]
    src, tgt = cloud(case["src"]), cloud(case["tgt"])
    kw = dict(init_T=guess(case), order="reversed" if second else "forward", events=events, **prm)
    if case["method"] == "p2l":
        return RR.p2l_align(src, tgt, normals(case["tgt"], oracle), GC.finite_nn(oracle), rb, **kw)
    kw["how"] = "adj" if second else "inv"
    if case["method"] == "gicp":
        return RR.gicp_align(src, normals(case["src"], oracle), tgt, normals(case["tgt"], oracle), GC.finite_nn(oracle), rb, **kw)
    return RR.vgicp_align(src, normals(case["src"], oracle), tgt, normals(case["tgt"], oracle), rb, **kw)


def reference(case, oracle):
    """dict(ref, events, floor (m, rad), stable), as gn_cases.reference."""
    ev, ev2 = [], []
    r, r2 = run(case, oracle, events=ev), run(case, oracle, second=True, events=ev2)
    ft, fa = RR.P.pose_err(r["T"], r2["T"])
    stable = bool(ev == ev2 and r["iters"] == r2["iters"] and r["status"] == r2["status"] and np.isfinite(r["T"]).all()
                  and np.isfinite(r2["T"]).all() and 10 * ft <= GC.POSE_CAP and 10 * fa <= GC.POSE_CAP)
    return dict(ref=r, events=ev, floor=(float(ft), float(fa)), stable=stable)


_REFS = {}


def references(oracle):
    """name -> reference(case) for every case (computed once per process)."""
    if not _REFS:
        for c in CASES:
            _REFS[c["name"]] = reference(c, oracle)
    return _REFS


def by_name(name):
    return next(c for c in CASES if c["name"] == name)
