"""The case table of the ISS keypoint tests (tests/iss_ref.py is the contract): clouds with the parameters they are searched
at and what the case is meant to have, the restatement's saliencies and keypoints of every case and of the known-answer pairs
of tests/fpfh_cases.py, computed once per session and shared, never modified by a test.

The cases are the smallest at which the kernels can go wrong:
  "empty" "n1" "n2" "n4"   0, 1, 2 and min_nn - 1 points close together: no list reaches min_nn, K = 0
  "u63" "u64" "u65"        uniform points in a 6 m cube: the edge of a 64-point chunk
  "uniform"                fpfh_radius_cases' 4 161 uniform points (66 chunks) at the defaults
  "k127" .. "k257"         ... with non_max_radius chosen so that K is 127, 128, 129, 255, 256, 257: the matcher's tile and
                           work-group sizes (the radii were found by bisection on the restatement)
  "lattice"                the shuffled 8 x 8 x 8 integer lattice at salient_radius = non_max_radius = 2: three distinct
                           saliencies shared by up to 96 points each (the tie rule decides), neighbours exactly at r
  "plane"                  400 points with one exact z: l3 is exactly zero, nothing is salient, K = 0
  "dups"                   uniform points of which 40 occur twice: a point and its copy have the same saliency to the bit
  "nan"                    uniform points and one NaN row
  "corner"                 fpfh_cases' corner scene: every 128-wide list is truncated
  "a_odd"                  a scan with NaN rows, inf rows and duplicated points"""
import functools

import numpy as np

import fpfh_cases as K
import fpfh_radius_cases as RK
import iss_ref as I

D = I.params()
K_RADII = {127: 1.9560546875, 128: 1.95263671875, 129: 1.94921875, 255: 1.646728515625, 256: 1.64501953125, 257: 1.6416015625}

# name -> (parameters, what the case must have under the restatement: "keypoints" (K >= 3), "none" (K = 0), or an exact K)
CASES = {
    "empty": (D, "none"), "n1": (D, "none"), "n2": (D, "none"), "n4": (D, "none"),
    "u63": (D, "keypoints"), "u64": (D, "keypoints"), "u65": (D, "keypoints"),
    "uniform": (D, "keypoints"),
    "lattice": (I.params(salient_radius=2.0), "keypoints"),
    "plane": (D, "none"),
    "dups": (D, "keypoints"), "nan": (D, "keypoints"), "corner": (D, "keypoints"), "a_odd": (D, "keypoints"),
}
CASES.update({"k%d" % k: (I.params(non_max_radius=r), k) for k, r in K_RADII.items()})

# the keypoint parameters the batch entries are held to on the known-answer pairs: the defaults (36 .. 39 keypoints per
# filtered scan) and a denser set
ISS_SETS = dict(default=D, dense=I.params(non_max_radius=1.0))


def _small(seed, n, half):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-half, half, (n, 3)), np.float32)


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "empty":
        return np.zeros((0, 3), np.float32)
    if name in ("n1", "n2", "n4"):
        return _small(40 + int(name[1:]), int(name[1:]), 1.0)
    if name in ("u63", "u64", "u65"):
        return _small(int(name[1:]), int(name[1:]), 3.0)
    if name == "uniform" or name[0] == "k":
        return RK.cloud("uniform")
    if name == "lattice":
        return RK.cloud("lattice")
    if name == "plane":
        xy = np.random.default_rng(5).uniform(-5.0, 5.0, (400, 2))
        return np.ascontiguousarray(np.concatenate([xy, np.full((400, 1), 0.25)], 1), np.float32)
    if name == "dups":
        x = _small(300, 300, 4.0)
        rng = np.random.default_rng(301)
        x = np.concatenate([x, x[rng.choice(300, 40, replace=False)]])
        return np.ascontiguousarray(x[rng.permutation(len(x))])
    if name == "nan":
        x = _small(302, 200, 3.5).copy()
        x[77] = np.nan
        return x
    return K.cloud(name)                                                   # "corner", "a_odd"


_SAL, _KNOWN_KP = {}, {}


def saliency(name, oracle):
    """iss_ref.saliency of a case + the keypoint flags: dict(sal, eig, idx, count, keep, kp), read-only."""
    if name not in _SAL:
        prm = CASES[name][0]
        sal, eig, idx, count = I.saliency(cloud(name), prm, oracle)
        keep = I.nms(cloud(name), sal, prm["non_max_radius"])
        out = dict(sal=sal, eig=eig, idx=idx, count=count, keep=keep, kp=np.flatnonzero(keep).astype(np.uint32))
        for a in out.values():
            a.setflags(write=False)
        _SAL[name] = out
    return _SAL[name]


def known_keypoints(pair, iss, oracle):
    """(source keypoints, target keypoints) of a known-answer pair (voxel-filtered) at ISS_SETS[iss]."""
    if (pair, iss) not in _KNOWN_KP:
        src, tgt, _ = K.known_filtered(pair)
        _KNOWN_KP[pair, iss] = (I.keypoints(src, ISS_SETS[iss], oracle), I.keypoints(tgt, ISS_SETS[iss], oracle))
    return _KNOWN_KP[pair, iss]


def known_features(pair, sup, oracle):
    """(source features, target features) of a known-answer pair: k-mode at fpfh_cases.PARAMS for sup = None, else the
    radius support fpfh_radius_cases.SUPPORTS[sup]."""
    if sup is not None:
        return RK.known_features(pair, sup, oracle)
    import fpfh_ref as F
    if (pair, None) not in _KNOWN_KP:
        src, tgt, _ = K.known_filtered(pair)
        _KNOWN_KP[pair, None] = tuple(F.features(x, K.PARAMS["normal_k"], K.PARAMS["feature_k"], oracle)["feat"] for x in (src, tgt))
    return _KNOWN_KP[pair, None]


_RESULT = {}


def known_result(pair, sup, iss, graph, oracle):
    """The restatement alone on a known-answer pair: iss_ref.register's dict (RANSAC at fpfh_cases.PARAMS and stream 0, or
    the graph at its defaults)."""
    key = (pair, sup, iss, graph)
    if key not in _RESULT:
        src, tgt, _ = K.known_filtered(pair)
        fs, ft = known_features(pair, sup, oracle)
        ks, kt = known_keypoints(pair, iss, oracle)
        _RESULT[key] = I.register(src, tgt, fs, ft, ks, kt, oracle, graph=graph, **({} if graph else K.PARAMS))
    return _RESULT[key]
