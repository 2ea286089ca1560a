"""Inputs shared by tests/test_gn_sweep_cpu.py and tests/test_gn_sweep_gpu.py, the sweep of the two Gauss-Newton
refinements (point-to-plane ICP and generalized ICP: gn6.hpp, gn6_kernels.hpp): synthetic worlds and the scans taken in
them (CPU synth.lidar_scan, whose device twin tests/test_raycast_gpu.py pins), hand-built clouds for the edge inputs, and
the list of whole-alignment cases with the float64 restatements' verdict on each (tests/p2l_ref.py, tests/gicp_ref.py,
run two ways: the pairs summed forward and reversed, and for generalized ICP M by numpy.linalg.inv and by the adjugate).

Nothing here looks at a device: whether a case is "stable" is decided by the restatements alone.  The 1-NN search and
the normals are the CPU oracle's (oracle/: nn3, ground_knn + ground_normals), which the device's are pinned to bit for
bit (tests/test_reg_gpu.py, tests/test_p2l_gpu.py); the module that holds them is handed in."""
import functools

import numpy as np

import gicp_ref as G
import p2l_ref as P

N_AZ = 200            # azimuth steps of a scan: ~12 k points, an align of the restatement takes well under a second
NORMAL_K = 10         # gloc_p2l_default_params / gloc_gicp_default_params
SYSTEM_CAP = 1e-9     # tests/test_gicp_gpu.py: 10 x the restatement's floor on a system may not exceed this ...
POSE_CAP = 1e-8       # ... and 10 x its floor on a pose not this
NO_PAIR = 0xFFFFFFFF
SIZES = (1, 5, 6, 63, 64, 65, 127, 128, 129, 255, 256, 257)      # sources: one wave, one work-group, the ld padding

# name -> (seed, n_boxes, extent) of synth.make_world
WORLDS = {"a": (1001, 400, 50.0), "b": (2002, 300, 40.0), "c": (3003, 500, 60.0)}


def _se3(*a, **k):
    from gloc3d_amd import synth
    return synth.se3(*a, **k)


def scan_poses():
    """world <- sensor poses of the scans taken in every world: 0 and 1 serve as targets, 2 and 3 as sources."""
    return [np.eye(4), _se3(-3.0, (0.4, -0.3, 0.0)), _se3(2.0, (0.2, 0.0, 0.0)), _se3(-1.5, (0.1, 0.15, 0.02), roll_deg=-0.5)]


def corner_scene(seed):
    """A hand-built scene of a few hundred points: three mutually orthogonal lattices (a floor and two walls, 0.25 m
    apart, 2 cm of noise) as the target; as the source 10 of its points with 5 cm of noise.  With a gate of a few
    centimetres a handful of pairs decide every pass: the scene of the jobs that lose their pairs once they have moved."""
    rng = np.random.default_rng(seed)
    g = np.arange(0.0, 3.0, 0.25)
    u, v = [m.ravel() for m in np.meshgrid(g, g)]
    z = np.zeros_like(u)
    tgt = np.concatenate([np.stack([u, v, z], 1), np.stack([u, z, v], 1), np.stack([z, u, v], 1)]) + rng.normal(size=(3 * len(u), 3)) * 0.02
    tgt += np.array([2.0, 1.0, -1.0])                     # (off the origin: the normals' orientation is decided by it)
    pick = rng.choice(len(tgt), 10, replace=False)
    src = tgt[pick] + rng.normal(size=(10, 3)) * 0.05
    return np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32)


def _odd(xyz):
    """NaN rows, inf rows and duplicated points, as tests/test_p2l_gpu.py::test_normals_equal_the_oracle_bit_for_bit."""
    odd = xyz.copy()
    odd[100:140] = odd[0:40]
    odd[::97, 1] = np.nan
    odd[5::301, 0] = np.inf
    odd[7::403, 2] = -np.inf
    odd[11::211] = np.nan
    return odd


@functools.lru_cache(maxsize=None)
def cloud(name):
    """float32 [n, 3], in its sensor's frame.
      "a0" .. "c3"      scan k of world a / b / c
      "a2_odd", "a0_odd" the first 5000 / 6000 points of a scan with NaN rows, inf rows and duplicated points
      "a0_dup"          2000 points of a0, every one of them three times over
      "a0_zn"           two points of a0 between three NaN rows: a target all of whose normals are zero
      "empty"           no points
      "a2_n<k>"         k points of a2, evenly spread over the scan
      "k<seed>_t / _s"  corner_scene(seed)'s target / source
      "full_t / _s"     a default synth.lidar_scan (~122 k points) and one taken 0.3 m and 1.5 degrees beside it"""
    from gloc3d_amd import synth
    if name == "empty":
        return np.zeros((0, 3), np.float32)
    if name[0] == "k":
        return corner_scene(int(name[1:-2]))[0 if name.endswith("_t") else 1]
    if name.startswith("full_"):
        w = synth.make_world(WORLDS["a"][0], n_boxes=WORLDS["a"][1], extent=WORLDS["a"][2])
        pose = np.eye(4) if name == "full_t" else _se3(1.5, (0.3, -0.1, 0.0))
        return np.ascontiguousarray(synth.lidar_scan(w, pose, seed=77 + (name == "full_s"))[:, :3])
    if "_" in name:
        base, kind = name.split("_")
        xyz = cloud(base)
        if kind == "odd":
            return np.ascontiguousarray(_odd(xyz[:5000 if base == "a2" else 6000]))
        if kind == "zn":                                  # two finite points between NaN rows: fewer than 3 neighbours, no normal
            z = np.full((5, 3), np.nan, np.float32)
            z[1], z[3] = xyz[len(xyz) // 3], xyz[2 * len(xyz) // 3]
            return z
        if kind == "dup":
            return np.ascontiguousarray(np.repeat(xyz[::len(xyz) // 2000][:2000], 3, axis=0))
        n = int(kind[1:])
        return np.ascontiguousarray(xyz[np.linspace(0, len(xyz) - 1, n).astype(np.int64)])
    seed, n_boxes, extent = WORLDS[name[0]]
    k = int(name[1])
    w = synth.make_world(seed, n_boxes=n_boxes, extent=extent)
    return np.ascontiguousarray(synth.lidar_scan(w, scan_poses()[k], seed=seed + 10 + k, n_az=N_AZ)[:, :3])


EDGE_SOURCES = ("a2_odd", "a0_dup") + tuple("a2_n%d" % n for n in SIZES)
EDGE_TARGETS = ("a0_odd", "a0_dup", "a0_zn", "empty")

_NORMALS = {}


def normals(name, oracle):
    """The cloud's normals from its NORMAL_K nearest neighbours, as the scan store builds them (the oracle's: pinned)."""
    if name not in _NORMALS:
        xyz = cloud(name)
        _NORMALS[name] = oracle.ground_normals(xyz, oracle.ground_knn(xyz, NORMAL_K)[0])[0] if len(xyz) else np.zeros((0, 3), np.float32)
    return _NORMALS[name]


def finite_nn(oracle):
    """The search the restatements are handed: the oracle's exact 1-NN of every finite point among the FINITE targets
    (smallest index among equals, positions in the whole target); NO_PAIR and FLT_MAX for a non-finite point or where
    there is no finite target -- what the device's search returns (tests/test_reg_gpu.py::
    test_nn_with_nan_points_in_source_and_target, test_empty_scans)."""
    def nn(p, t):
        p, t = np.asarray(p, np.float32).reshape(-1, 3), np.asarray(t, np.float32).reshape(-1, 3)
        idx = np.full(len(p), NO_PAIR, np.uint32)
        d2 = np.full(len(p), np.finfo(np.float32).max, np.float32)
        fp, ft = np.isfinite(p).all(1), np.isfinite(t).all(1)
        if fp.any() and ft.any():
            back = np.flatnonzero(ft).astype(np.uint32)
            i, d = oracle.nn3(p[fp], t[ft], grid=True)
            hit = i < len(back)
            idx[fp] = np.where(hit, back[np.where(hit, i, 0)], NO_PAIR)
            d2[fp] = d
        return idx, d2
    return nn


def truth(src, tgt):
    """source frame -> target frame of two scans of one world; the identity for everything hand-built."""
    if len(src) == 2 and len(tgt) == 2 and src[0] == tgt[0] and src[0] in WORLDS:
        Ps = scan_poses()
        return np.linalg.inv(Ps[int(tgt[1])]) @ Ps[int(src[1])]
    if (src + "_").startswith("a2_") and (tgt + "_").startswith("a0_") and (src, tgt) != ("a2", "a0"):
        return truth("a2", "a0")                          # (clouds cut from those two scans)
    return np.eye(4)


def _case(name, method, src, tgt, yaw=0.0, t=(0.0, 0.0, 0.0), pitch=0.0, roll=0.0, at=None, **params):
    """Guess = truth x offset, or `at` x offset.  params: max_iters, max_corr_dist, trans_eps, rot_eps (and plane_eps)."""
    return dict(name=name, method=method, src=src, tgt=tgt, off=(yaw, t, pitch, roll), at=at, params=params)


def _both(name, *a, **k):
    return [_case(name + "_p2l", "p2l", *a, **k), _case(name + "_gicp", "gicp", *a, **k)]


FAR = (1000.0, 0.0, 0.0)

# ---- the cases -----------------------------------------------------------------------------------------------------------
# (1) scans of three worlds against two targets each, guesses from 0.05 m / 0.5 deg to 1.5 m / 40 deg off, with and
#     without a gate, max_iters on both sides of the host's look every 4 passes, the stop test off, on, and half set
CASES = []
CASES += _both("a20_near", "a2", "a0", yaw=1.0, t=(0.10, -0.05, 0.02), max_iters=10, max_corr_dist=1.0)
CASES += _both("a31_eps", "a3", "a1", yaw=-2.0, t=(-0.15, 0.10, -0.03), roll=0.4, max_iters=30, max_corr_dist=1.0, trans_eps=1e-4, rot_eps=1e-5)
CASES += _both("b20_it1", "b2", "b0", yaw=0.5, t=(0.25, 0.20, 0.05), max_iters=1)
CASES += _both("b31_it3", "b3", "b1", yaw=-4.0, t=(0.3, -0.4, 0.0), max_iters=3, max_corr_dist=2.0)
CASES += _both("c20_it4", "c2", "c0", yaw=3.0, t=(-0.2, 0.3, 0.05), pitch=0.5, max_iters=4)
CASES += _both("c31_it5", "c3", "c1", yaw=-1.0, t=(0.05, 0.02, 0.0), max_iters=5, max_corr_dist=0.3)
CASES += _both("a21_it8", "a2", "a1", yaw=6.0, t=(0.6, -0.5, 0.1), max_iters=8, max_corr_dist=3.0)
CASES += _both("b30_it9", "b3", "b0", yaw=-8.0, t=(-0.9, 0.4, -0.05), roll=1.0, max_iters=9)
CASES += _both("c21_trans_only", "c2", "c1", yaw=1.5, t=(0.2, 0.1, 0.0), max_iters=6, max_corr_dist=1.0, trans_eps=1.0)
CASES += _both("a30_rot_only", "a3", "a0", yaw=-1.5, t=(0.1, -0.2, 0.02), max_iters=5, max_corr_dist=1.0, rot_eps=1.0)
CASES += _both("b21_yaw25", "b2", "b1", yaw=25.0, t=(0.5, 0.5, 0.0), max_iters=3)
CASES += _both("c30_yaw40", "c3", "c0", yaw=40.0, t=(1.0, -1.0, 0.1), max_iters=4)
CASES += _both("a20_yaw60", "a2", "a0", yaw=-60.0, t=(-1.5, 0.3, 0.0), pitch=3.0, max_iters=3)
CASES += _both("b20_big_eps", "b2", "b0", yaw=12.0, t=(1.2, 0.8, 0.1), max_iters=9, trans_eps=10.0, rot_eps=10.0)
# (2) the stop test against the look: eps set so that the restatement stops at pass 4 (a look) and at pass 5 (one after)
_STOP = dict(max_iters=9, max_corr_dist=1.0)
CASES += [_case("a20_stop4_p2l", "p2l", "a2", "a0", yaw=1.0, t=(0.10, -0.05, 0.02), trans_eps=8e-3, rot_eps=8e-4, **_STOP),
          _case("a20_stop5_p2l", "p2l", "a2", "a0", yaw=1.0, t=(0.10, -0.05, 0.02), trans_eps=5e-3, rot_eps=5e-4, **_STOP),
          _case("a20_stop4_gicp", "gicp", "a2", "a0", yaw=1.0, t=(0.10, -0.05, 0.02), trans_eps=1.3e-2, rot_eps=1e-3, **_STOP),
          _case("a20_stop5_gicp", "gicp", "a2", "a0", yaw=1.0, t=(0.10, -0.05, 0.02), trans_eps=5e-3, rot_eps=4e-4, **_STOP)]
# (3) identical scans at the identity: every residual is exactly zero, g = 0 and the update's angle is 0
CASES += _both("a0_self_capped", "a0", "a0", max_iters=4)
CASES += _both("a0_self_eps", "a0", "a0", max_iters=9, trans_eps=1e-6, rot_eps=1e-6)
CASES += _both("b1_self_eps", "b1", "b1", max_iters=9, trans_eps=1e-6, rot_eps=1e-6)
# (4) edge inputs: non-finite rows and duplicates on either side, an empty target, tiny sources, no pair in reach
CASES += _both("odd_src", "a2_odd", "a0", yaw=1.0, t=(0.1, 0.1, 0.0), max_iters=5, max_corr_dist=1.0)
CASES += _both("odd_tgt", "a2", "a0_odd", yaw=-1.0, t=(0.1, -0.1, 0.0), max_iters=5, max_corr_dist=1.0)
CASES += _both("odd_both", "a2_odd", "a0_odd", yaw=0.5, t=(0.05, 0.1, 0.02), max_iters=8, max_corr_dist=1.0, trans_eps=1e-3, rot_eps=1e-4)
CASES += _both("dup_src", "a0_dup", "a0", yaw=1.0, t=(0.1, 0.0, 0.0), max_iters=4)
CASES += _both("dup_tgt", "a2", "a0_dup", yaw=1.0, t=(0.1, 0.0, 0.0), max_iters=4, max_corr_dist=2.0)
CASES += _both("zero_nrm_tgt", "a2", "a0_zn", yaw=1.0, t=(0.1, 0.0, 0.0), max_iters=4)      # point-to-plane: no pair; generalized: all
CASES += _both("empty_tgt", "a2", "empty", yaw=1.0, t=(0.1, 0.0, 0.0), max_iters=5)
CASES += _both("n1", "a2_n1", "a0", max_iters=3)
CASES += _both("n5", "a2_n5", "a0", yaw=1.0, max_iters=3)
CASES += _both("n64", "a2_n64", "a0", yaw=1.0, t=(0.1, 0.05, 0.0), max_iters=5)
CASES += _both("n257", "a2_n257", "a0", yaw=-1.0, t=(0.1, -0.05, 0.02), max_iters=9, trans_eps=1e-3, rot_eps=1e-4)
CASES += _both("out_of_reach", "a2", "a0", yaw=1.0, t=FAR, max_iters=5, max_corr_dist=1.0)
# (5) the corner scene behind a gate of centimetres (found by a search over seeds and guesses with the restatements
#     alone): jobs that lose their pairs after one or more updates, beside ones that converge, hit the cap, or have
#     no six pairs to begin with -- MIXED holds the batches of them
CORNER = dict(max_iters=8, max_corr_dist=0.12, trans_eps=1e-5, rot_eps=1e-5)
_K1 = [(0.8, (-0.03, -0.06, -0.06)), (0.3, (0.05, 0.04, -0.06)), (-0.3, (0.04, -0.03, -0.05)), (1.9, (0.05, 0.01, 0.03)),
       (-0.6, (-0.04, -0.05, 0.01)), (-0.7, (0.05, -0.03, 0.01))]      # generalized ICP: cap, stop at 5, at 6, at once, lost at 2, at 4
_K6 = [(1.0, (0.02, 0.0, 0.0)), (0.1, (0.05, -0.04, 0.05)), (0.0, (0.0, 0.0, 0.0)), (-1.1, (-0.01, 0.04, -0.01)),
       (-1.0, (-0.04, 0.02, 0.03)), (0.6, (0.05, 0.02, 0.0))]          # point-to-plane: cap, at once, lost at 1, 2, 4 and 6
CASES += [_case("k1_%d_gicp" % i, "gicp", "k1_s", "k1_t", yaw=y, t=t, **CORNER) for i, (y, t) in enumerate(_K1)]
CASES += [_case("k6_%d_p2l" % i, "p2l", "k6_s", "k6_t", yaw=y, t=t, **CORNER) for i, (y, t) in enumerate(_K6)]
# ... and, the same source against another seed's corner, two guesses that converge (at passes 3 and 5)
CASES += [_case("k6_6_p2l", "p2l", "k6_s", "k14_t", yaw=0.9, t=(0.04, -0.04, -0.03), **CORNER),
          _case("k6_7_p2l", "p2l", "k6_s", "k14_t", yaw=0.4, t=(0.02, -0.03, -0.04), **CORNER)]
CASES += [_case("k5_stop5_p2l", "p2l", "k5_s", "k5_t", **CORNER)]
# (6) the corner scene tens of degrees off without a gate: first updates of more than 0.3 rad
CASES += _both("k1_yaw30", "k1_s", "k1_t", yaw=30.0, t=(0.5, 0.0, 0.0), max_iters=3)
CASES += _both("k1_yaw90", "k1_s", "k1_t", yaw=90.0, t=(0.5, 0.0, 0.0), max_iters=3)
# (7) scans behind one source in one call: a near and a farther guess that stop at different passes, another world,
#     an empty target, no pair in reach
_M = dict(max_iters=6, max_corr_dist=1.0, trans_eps=2e-3, rot_eps=2e-4)
for _m in ("p2l", "gicp"):
    CASES += [_case("mix_near_" + _m, _m, "a2", "a0", **_M), _case("mix_off_" + _m, _m, "a2", "a0", yaw=0.5, t=(0.25, 0.20, 0.05), **_M),
              _case("mix_mid_" + _m, _m, "a2", "a0", yaw=-0.3, t=(0.05, -0.03, 0.0), **_M),
              _case("mix_other_" + _m, _m, "a2", "b0", at=np.eye(4), **_M), _case("mix_empty_" + _m, _m, "a2", "empty", **_M),
              _case("mix_far_" + _m, _m, "a2", "a0", t=FAR, **_M)]

# The mixed batches: names of cases with one source and one parameter block, run as ONE call.  A method's first batch (the
# corner scene) ends every way a job can: at the cap, converged at different passes, degenerate at once, degenerate mid-run.
MIXED = {"gicp": [["k1_%d_gicp" % i for i in range(6)], ["mix_%s_gicp" % k for k in ("near", "off", "mid", "other", "empty", "far")]],
         "p2l": [["k6_%d_p2l" % i for i in range(8)], ["mix_%s_p2l" % k for k in ("near", "off", "mid", "other", "empty", "far")]]}


def guess(case):
    yaw, t, pitch, roll = case["off"]
    base = truth(case["src"], case["tgt"]) if case["at"] is None else np.asarray(case["at"], np.float64)
    return (base @ _se3(yaw, t, pitch_deg=pitch, roll_deg=roll)).astype(np.float32)


def params(case):
    """max_iters, max_corr_dist, trans_eps, rot_eps, plane_eps with every float rounded to the float32 the device's
    parameter block holds."""
    p = dict(max_iters=30, max_corr_dist=0.0, trans_eps=0.0, rot_eps=0.0, plane_eps=1e-3)
    p.update(case["params"])
    return {k: (int(v) if k == "max_iters" else float(np.float32(v))) for k, v in p.items()}


def run(case, oracle, second=False, events=None):
    """The restatement's run of a case; second: the other summation order (and for generalized ICP the other inverse)."""
    prm = params(case)
    nn = finite_nn(oracle)
    src, tgt = cloud(case["src"]), cloud(case["tgt"])
    kw = dict(init_T=guess(case), max_iters=prm["max_iters"], max_corr_dist=prm["max_corr_dist"], trans_eps=prm["trans_eps"],
              rot_eps=prm["rot_eps"], order="reversed" if second else "forward", events=events)
    if case["method"] == "p2l":
        return P.align(src, tgt, normals(case["tgt"], oracle), nn, **kw)
    return G.align(src, normals(case["src"], oracle), tgt, normals(case["tgt"], oracle), nn, plane_eps=prm["plane_eps"],
                   how="adj" if second else "inv", **kw)


def reference(case, oracle):
    """dict(ref, events, floor (m, rad), stable): stable when both runs take the same branches, agree on iters and status
    and end with finite poses 10 x whose distance stays under POSE_CAP."""
    ev, ev2 = [], []
    r, r2 = run(case, oracle, events=ev), run(case, oracle, second=True, events=ev2)
    ft, fa = P.pose_err(r["T"], r2["T"])
    stable = bool(ev == ev2 and r["iters"] == r2["iters"] and r["status"] == r2["status"] and np.isfinite(r["T"]).all()
                  and np.isfinite(r2["T"]).all() and 10 * ft <= POSE_CAP and 10 * fa <= POSE_CAP)
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
