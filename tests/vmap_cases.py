"""Cases of the resident voxel maps shared by tests/test_vmap_cases_cpu.py and tests/test_vmap_gpu.py: the two-scan map of
world a, the scan-to-map alignments against it with the restatement's verdict on each (tests/vmap_ref.py, run two ways as
tests/vgicp_cases.py runs its own), and the inserts of the multi-scan map.  Clouds, poses and caps are tests/gn_cases.py's.
Nothing here looks at a device; normals(name) -> [n, 3] is handed in."""
import numpy as np

import gn_cases as GC
import vgicp_ref as V
import vmap_ref as M

MAX_UNSTABLE = 0.10   # of the cases (vgicp_cases.reference's rule)


def bits(a):
    """The array's bit patterns (floats of either width as unsigned integers; integers as they are)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    """Two tuples of arrays (or two dicts with the same keys), equal bit for bit."""
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(a)]
    return len(a) == len(b) and all(np.asarray(x).shape == np.asarray(y).shape and np.asarray(x).dtype == np.asarray(y).dtype
                                    and bool((bits(x) == bits(y)).all()) for x, y in zip(a, b))


def pose_into_a0(name):
    """scan -> a0's frame, fp32 (None for a0 itself: inserted as it is)."""
    base = name.split("_")[0]
    return None if base == "a0" else GC.truth(base, "a0").astype(np.float32)


# the map every alignment case runs against: a0 as it is, a1 under P0^-1 P1 (at 1 m most of a0's voxels are merged into)
TWO_SCANS = [("a0", None), ("a1", pose_into_a0("a1"))]
# the multi-scan map of the merge test: three scans, one of them with non-finite rows, and the first once more
INSERTS = [("a0", None), ("a1", pose_into_a0("a1")), ("a2_odd", pose_into_a0("a2")), ("a0", None)]

# capacity -> the resolution at which the corner scene k6_t has exactly that many voxels (found with vgicp_ref.voxels;
# tests/test_vmap_gpu.py asserts the counts): maps filled to the last voxel, their tables at their fullest
EXACT_FIT = {8: 1.89, 16: 1.59, 64: 0.682}
GRID = [(1.0, 7), (0.5, 27), (2.0, 1)]       # (resolution, neighbors)
SOURCES = [("a2", 1.0, (0.10, -0.05, 0.02)), ("a3", -2.0, (-0.15, 0.10, -0.03)), ("a2_n257", -1.5, (0.12, -0.06, 0.02))]


def _case(src, yaw, t, res, nb):
    return dict(name=f"{src}_r{res:g}_n{nb}", src=src, off=(yaw, t), resolution=res,
                params=dict(max_iters=9, trans_eps=2e-3, rot_eps=2e-4, resolution=res, neighbors=nb))


CASES = [_case(s, yaw, t, res, nb) for s, yaw, t in SOURCES for res, nb in GRID]


def guess(case):
    """The source's pose in the map's frame, 0.1 - 0.15 m and 1 - 2 degrees off the truth."""
    from gloc3d_amd import synth
    yaw, t = case["off"]
    return (GC.truth(case["src"].split("_")[0], "a0") @ synth.se3(yaw, t)).astype(np.float32)


def params(case):
    """vgicp_cases.params' block: every float rounded to the float32 the device holds."""
    p = dict(max_iters=30, max_corr_dist=0.0, trans_eps=0.0, rot_eps=0.0, plane_eps=1e-3, resolution=1.0, neighbors=7, min_points=1)
    p.update(case["params"])
    return {k: (int(v) if k in ("max_iters", "neighbors", "min_points") else float(np.float32(v))) for k, v in p.items()}


def build_map(inserts, resolution, normals, order="forward", capacity=1 << 18):
    m = M.Map(resolution, capacity, order)
    for name, T in inserts:
        assert m.insert(GC.cloud(name), normals(name), T)
    return m


_MAPS = {}


def two_scan_map(resolution, normals, order="forward"):
    """(made once per process and left alone)"""
    key = (float(resolution), order)
    if key not in _MAPS:
        _MAPS[key] = build_map(TWO_SCANS, resolution, normals, order)
    return _MAPS[key]


def run(case, normals, second=False):
    prm = params(case)
    vm = two_scan_map(case["resolution"], normals, "reversed" if second else "forward")
    return M.align(GC.cloud(case["src"]), normals(case["src"]), vm, init_T=guess(case), how="adj" if second else "inv",
                   order="reversed" if second else "forward", **prm)


def reference(case, normals):
    """dict(ref, floor (m, rad), stable), by vgicp_cases.reference's rule."""
    r, r2 = run(case, normals), run(case, normals, second=True)
    ft, fa = V.pose_err(r["T"], r2["T"])
    stable = bool(r["iters"] == r2["iters"] and r["status"] == r2["status"] and np.isfinite(r["T"]).all() and np.isfinite(r2["T"]).all()
                  and 10 * ft <= GC.POSE_CAP and 10 * fa <= GC.POSE_CAP)
    return dict(ref=r, floor=(float(ft), float(fa)), stable=stable)


def by_name(name):
    return next(c for c in CASES if c["name"] == name)
