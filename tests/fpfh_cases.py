"""The case table of the FPFH feature-based global registration tests: clouds, the known-answer pairs, and their
restatement results (computed once per session and shared; tests/fpfh_ref.py is the contract).

Scans are synth.lidar_scan at n_beams = 16, n_az = 400 (at most 6 400 points) of three worlds; the known-answer pairs are
voxel-filtered at LEAF with the approximate voxel filter (tests/ndt_ref.py restates gloc_scan_store_add_approx_voxel), the
filter the stage is meant to run behind.  PARAMS is the committed setting of the known-answer table: the defaults, found
sufficient on the CPU before any device run (test_fpfh_cases_cpu.py holds the rule that decides)."""
import functools

import numpy as np

import fpfh_ref as F
import gn_cases
import ndt_ref

N_BEAMS, N_AZ = 16, 400
LEAF = 0.5
PARAMS = dict(F.DEFAULTS)
WORLDS = gn_cases.WORLDS
SIZES = (1, 4, 63, 64, 65, 257)
EDGE_CAP = 0.01             # at most 1 % of a cloud's points may be edge-flagged
OK_T, OK_R = 1.0, 5.0       # the reference's success rule: within 1 m / 5 degrees of ground truth

# name -> (world, yaw of the target pose, yaw of the source pose, source position): the relative yaw and distance are the
# case.  Eight pairs of one world each (relative yaw 0, 45, 90, 135, 170, 180 degrees, 0 - 4 m apart), two of different worlds.
KNOWN = {
    "yaw0_1m": ("a", 0.0, 0.0, (1.0, 0.0, 0.0)),
    "yaw45_2m": ("a", 0.0, 45.0, (1.5, 1.3, 0.0)),
    "yaw90_0m": ("b", 10.0, 100.0, (0.0, 0.0, 0.0)),
    "yaw90_3m": ("a", 0.0, 90.0, (-2.0, 2.2, 0.0)),
    "yaw135_2m": ("c", -20.0, 115.0, (2.0, 0.0, 0.0)),
    "yaw170_1m": ("a", 0.0, 170.0, (0.6, -0.8, 0.0)),
    "yaw180_4m": ("b", 0.0, 180.0, (4.0, 0.0, 0.0)),
    "yaw180_0m": ("c", 0.0, 180.0, (0.0, 0.0, 0.0)),
    "other_ab": ("a", 0.0, 30.0, (1.0, 0.0, 0.0), "b"),
    "other_bc": ("b", 0.0, 90.0, (0.0, 1.0, 0.0), "c"),
}


def _world(name):
    from gloc3d_amd import synth
    seed, n_boxes, extent = WORLDS[name]
    return synth.make_world(seed, n_boxes=n_boxes, extent=extent)


def _scan(world, pose, seed):
    from gloc3d_amd import synth
    return np.ascontiguousarray(synth.lidar_scan(_world(world), pose, seed=seed, n_beams=N_BEAMS, n_az=N_AZ)[:, :3], np.float32)


def relative_yaw(name):
    k = KNOWN[name]
    return abs(((k[2] - k[1]) + 180.0) % 360.0 - 180.0)


@functools.lru_cache(maxsize=None)
def known_pair(name):
    """(src, tgt, truth): the two raw scans (float32 [n, 3], each in its sensor's frame) and source -> target, or None for
    scans of different worlds."""
    from gloc3d_amd import synth
    k = KNOWN[name]
    seed = WORLDS[k[0]][0]
    Pt, Ps = synth.se3(k[1], (0.0, 0.0, 0.0)), synth.se3(k[2], k[3])
    tgt = _scan(k[0], Pt, seed + 31)
    src = _scan(k[4] if len(k) > 4 else k[0], Ps, seed + 32)
    return src, tgt, (None if len(k) > 4 else np.linalg.inv(Pt) @ Ps)


@functools.lru_cache(maxsize=None)
def known_filtered(name):
    src, tgt, truth = known_pair(name)
    return np.ascontiguousarray(ndt_ref.approx_voxel(src, LEAF), np.float32), np.ascontiguousarray(ndt_ref.approx_voxel(tgt, LEAF), np.float32), truth


@functools.lru_cache(maxsize=None)
def cloud(name):
    """float32 [n, 3]:
      "a" / "b" / "c"   a raw scan of that world (16 x 400 beams)
      "a_vox"           ... voxel-filtered at LEAF
      "corner"          gn_cases' corner scene (three orthogonal lattices)
      "a_odd"           world a's scan with NaN rows, inf rows and duplicated points
      "zn"              two finite points between NaN rows: every normal is zero
      "empty"           no points
      "n<k>"            k points of "a", evenly spread"""
    if name in WORLDS:
        return _scan(name, None, WORLDS[name][0] + 30)
    if name == "a_vox":
        return np.ascontiguousarray(ndt_ref.approx_voxel(cloud("a"), LEAF), np.float32)
    if name == "corner":
        return gn_cases.corner_scene(5)[0]
    if name == "a_odd":
        return np.ascontiguousarray(gn_cases._odd(cloud("a")[:5000]))
    if name == "zn":
        z = np.full((5, 3), np.nan, np.float32)
        z[1], z[3] = cloud("a")[100], cloud("a")[2000]
        return z
    if name == "empty":
        return np.zeros((0, 3), np.float32)
    if name[0] == "n":
        a = cloud("a")
        return np.ascontiguousarray(a[np.linspace(0, len(a) - 1, int(name[1:])).astype(np.int64)])
    raise KeyError(name)


CLOUDS = ("a", "b", "c", "a_vox", "corner", "a_odd", "zn", "empty") + tuple("n%d" % k for k in SIZES)

_FEATURES, _KNOWN = {}, {}


def features(name, oracle):
    """fpfh_ref.features of a cloud at PARAMS, once per session (never modified by a test)."""
    if name not in _FEATURES:
        _FEATURES[name] = F.features(cloud(name), PARAMS["normal_k"], PARAMS["feature_k"], oracle)
    return _FEATURES[name]


def pose_error(T, truth):
    """(metres, degrees) between two source -> target poses."""
    D = np.linalg.inv(np.asarray(truth, np.float64)) @ np.asarray(T, np.float64)
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(D[:3, 3])), float(np.degrees(np.arccos(c)))


def known_result(name, oracle):
    """The restatement alone on a known-answer pair at PARAMS: fpfh_ref.register's dict + err (m, deg; None for the pairs of
    different worlds) + located."""
    if name not in _KNOWN:
        src, tgt, truth = known_filtered(name)
        r = F.register(src, tgt, oracle, stream_id=0, **PARAMS)
        r["err"] = None if truth is None else pose_error(r["T"], truth)
        r["located"] = bool(truth is not None and r["ok"] and r["err"][0] <= OK_T and r["err"][1] <= OK_R)
        _KNOWN[name] = r
    return _KNOWN[name]


def known_answer_cases(oracle):
    """The names of the cases the restatement locates: what the device is then held to."""
    return [n for n in KNOWN if known_result(n, oracle)["located"]]
