"""Whole-alignment cases of the voxelized generalized ICP refinement, shared by tests/test_vgicp_cases_cpu.py and
tests/test_vgicp_gpu.py: clouds, guesses and ground truth are tests/gn_cases.py's, the restatement is tests/vgicp_ref.py.

Voxel membership is discrete: a pose that differs in the last bit can move a point across a face, and from there the two
trajectories part.  So, by the rule of gn_cases.reference, a case is held to the restatement's trajectory only if the
restatement's own two evaluations (voxel sums and pairs summed forward with numpy.linalg.inv; reversed with the
adjugate) agree on iters and status and end within POSE_CAP / 10 of each other.  Nothing here looks at a device."""
import numpy as np

import gn_cases as GC
import vgicp_ref as V

MAX_UNSTABLE = 0.10   # of the cases


def _case(name, src, tgt, yaw=0.0, t=(0.0, 0.0, 0.0), pitch=0.0, roll=0.0, at=None, **params):
    return dict(name=name, method="vgicp", src=src, tgt=tgt, off=(yaw, t, pitch, roll), at=at, params=params)


FAR = GC.FAR
CASES = [
    # scans of three worlds, guesses from 0.05 m / 0.5 deg to 0.9 m / 8 deg off; every neighbourhood; resolutions 0.5 .. 2 m;
    # caps on both sides of the host's look every 4 passes; the stop test off and on
    _case("a20_near", "a2", "a0", yaw=1.0, t=(0.10, -0.05, 0.02), max_iters=10, neighbors=7),
    _case("a31_eps", "a3", "a1", yaw=-2.0, t=(-0.15, 0.10, -0.03), roll=0.4, max_iters=30, trans_eps=2e-3, rot_eps=2e-4, neighbors=7),
    _case("b20_it3_n1", "b2", "b0", yaw=0.5, t=(0.25, 0.20, 0.05), max_iters=3, neighbors=1),
    _case("b31_it4_n27", "b3", "b1", yaw=-4.0, t=(0.3, -0.4, 0.0), max_iters=4, max_corr_dist=2.0, neighbors=27),
    _case("c20_it5", "c2", "c0", yaw=3.0, t=(-0.2, 0.3, 0.05), pitch=0.5, max_iters=5, neighbors=7),
    _case("c31_it8_n1", "c3", "c1", yaw=-1.0, t=(0.05, 0.02, 0.0), max_iters=8, max_corr_dist=1.0, neighbors=1),
    _case("a21_it9_r2", "a2", "a1", yaw=6.0, t=(0.6, -0.5, 0.1), max_iters=9, resolution=2.0, neighbors=7),
    _case("b30_it9_n27", "b3", "b0", yaw=-8.0, t=(-0.9, 0.4, -0.05), roll=1.0, max_iters=9, neighbors=27),
    _case("a20_eps_r05", "a2", "a0", yaw=1.0, t=(0.10, -0.05, 0.02), max_iters=9, resolution=0.5, neighbors=27, trans_eps=5e-3, rot_eps=5e-4),
    _case("c21_min3", "c2", "c1", yaw=1.5, t=(0.2, 0.1, 0.0), max_iters=4, min_points=3, neighbors=7),
    _case("a0_self", "a0", "a0", max_iters=5, neighbors=1, trans_eps=1e-6, rot_eps=1e-6),
    # edge inputs
    _case("odd_both", "a2_odd", "a0_odd", yaw=0.5, t=(0.05, 0.1, 0.02), max_iters=5, max_corr_dist=1.0, neighbors=7),
    _case("dup_tgt", "a2", "a0_dup", yaw=1.0, t=(0.1, 0.0, 0.0), max_iters=4, neighbors=7),
    _case("zero_nrm_tgt", "a2", "a0_zn", yaw=1.0, t=(0.1, 0.0, 0.0), max_iters=4, resolution=4.0, neighbors=27),
    _case("empty_tgt", "a2", "empty", yaw=1.0, t=(0.1, 0.0, 0.0), max_iters=5, neighbors=7),
    _case("n5", "a2_n5", "a0", yaw=1.0, max_iters=3, neighbors=27),
    _case("n257", "a2_n257", "a0", yaw=-1.0, t=(0.1, -0.05, 0.02), max_iters=9, trans_eps=1e-3, rot_eps=1e-4, neighbors=7),
    _case("out_of_reach", "a2", "a0", yaw=1.0, t=FAR, max_iters=5, neighbors=27),
]
# scans behind one source in one call: a near and farther guesses that stop at different passes, another world, an empty
# target, no voxel in reach
_M = dict(max_iters=8, max_corr_dist=1.5, trans_eps=5e-3, rot_eps=5e-4, neighbors=7)
CASES += [_case("mix_near", "a2", "a0", **_M), _case("mix_off", "a2", "a0", yaw=0.5, t=(0.25, 0.20, 0.05), **_M),
          _case("mix_mid", "a2", "a0", yaw=-0.3, t=(0.05, -0.03, 0.0), **_M), _case("mix_other", "a2", "b0", at=np.eye(4), **_M),
          _case("mix_empty", "a2", "empty", **_M), _case("mix_far", "a2", "a0", t=FAR, **_M), _case("mix_a1", "a2", "a1", yaw=0.2, **_M)]
MIXED = ["mix_near", "mix_off", "mix_mid", "mix_other", "mix_empty", "mix_far", "mix_a1"]

guess = GC.guess


def params(case):
    """The parameter block of a case, every float rounded to the float32 the device holds."""
    p = dict(max_iters=30, max_corr_dist=0.0, trans_eps=0.0, rot_eps=0.0, plane_eps=1e-3, resolution=1.0, neighbors=7, min_points=1)
    p.update(case["params"])
    return {k: (int(v) if k in ("max_iters", "neighbors", "min_points") else float(np.float32(v))) for k, v in p.items()}


def run(case, normals, second=False):
    """The restatement's run of a case; normals(name) -> [n, 3]; second: the other summation order and inverse."""
    prm = params(case)
    return V.align(GC.cloud(case["src"]), normals(case["src"]), GC.cloud(case["tgt"]), normals(case["tgt"]), init_T=guess(case),
                   how="adj" if second else "inv", order="reversed" if second else "forward", **prm)


def reference(case, normals):
    """dict(ref, floor (m, rad), stable)."""
    r, r2 = run(case, normals), run(case, normals, second=True)
    ft, fa = V.pose_err(r["T"], r2["T"])
    stable = bool(r["iters"] == r2["iters"] and r["status"] == r2["status"] and np.isfinite(r["T"]).all() and np.isfinite(r2["T"]).all()
                  and 10 * ft <= GC.POSE_CAP and 10 * fa <= GC.POSE_CAP)
    return dict(ref=r, floor=(float(ft), float(fa)), stable=stable)


def by_name(name):
    return next(c for c in CASES if c["name"] == name)
