"""The case table of the radius-support FPFH tests (tests/fpfh_radius_ref.py is the contract): supports, clouds, the lists
and features of every pairing and the known-answer results, computed once per session and shared, never modified by a test.

A support is (normal_radius, feature_radius, normal_max_nn, feature_max_nn, normal_min_nn).  The clouds are fpfh_cases'
plus two made for the search:
  "lattice"   a shuffled 8 x 8 x 8 integer lattice, searched at r = 2, max_nn = 16: 33 points within r of an interior point,
              six of them exactly at d2 == r2, and the cap cuts through the twelve ties at d2 = 2 -- the boundary's <= and the
              index tie-break both decide the list
  "uniform"   4 161 uniform points in a 20 m cube, searched at r = 1.5, max_nn = 128: 66 chunks of 64, lists mostly short"""
import functools

import numpy as np

import fpfh_cases as K
import fpfh_radius_ref as R
import fpfh_ref as F
import pairgraph_ref as G

S_A = (1.0, 2.5, 32, 128, 5)
S_B = (0.75, 1.5, 32, 64, 5)
S_RAW = (0.5, 1.0, 30, 100, 5)
S_MIN = (0.4, 0.8, 16, 48, 4)
SUPPORTS = dict(S_A=S_A, S_B=S_B, S_RAW=S_RAW, S_MIN=S_MIN)

# the pairings whose normals and features the device is held to: (cloud, support name)
FEATURES = (("a_vox", "S_A"), ("a_vox", "S_B"), ("a", "S_RAW"), ("b", "S_RAW"), ("a_odd", "S_RAW"), ("c", "S_MIN"), ("corner", "S_A"),
            ("zn", "S_A"), ("empty", "S_A")) + tuple(("n%d" % k, "S_A") for k in K.SIZES)
# the searches on their own: (cloud, radius, max_nn) -- both lists of every pairing above, and the two made for the search
LISTS = tuple(dict.fromkeys([(c, SUPPORTS[s][0], SUPPORTS[s][2]) for c, s in FEATURES] + [(c, SUPPORTS[s][1], SUPPORTS[s][3]) for c, s in FEATURES]
                            + [("lattice", 2.0, 16), ("uniform", 1.5, 128)]))
KNOWN_SUPPORTS = ("S_B", "S_A")


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "lattice":
        g = np.arange(8, dtype=np.float32)
        p = np.stack([m.ravel() for m in np.meshgrid(g, g, g, indexing="ij")], 1)
        return np.ascontiguousarray(p[np.random.default_rng(8).permutation(len(p))], np.float32)
    if name == "uniform":
        return np.ascontiguousarray(np.random.default_rng(4161).uniform(-10.0, 10.0, (4161, 3)), np.float32)
    return K.cloud(name)


@functools.lru_cache(maxsize=None)
def lists(name, r, max_nn):
    """fpfh_radius_ref.radius_lists of a cloud (read-only)."""
    out = R.radius_lists(cloud(name), r, max_nn)
    for a in out:
        a.setflags(write=False)
    return out


_FEATURES, _KNOWN_FEAT, _KNOWN, _GRAPH = {}, {}, {}, {}


def features(name, sup, oracle):
    """fpfh_radius_ref.features of a cloud at SUPPORTS[sup], once per session."""
    if (name, sup) not in _FEATURES:
        _FEATURES[name, sup] = R.features(cloud(name), SUPPORTS[sup], oracle)
    return _FEATURES[name, sup]


def known_features(name, sup, oracle):
    """(source features, target features) of a known-answer pair (voxel-filtered) at SUPPORTS[sup]."""
    if (name, sup) not in _KNOWN_FEAT:
        src, tgt, _ = K.known_filtered(name)
        _KNOWN_FEAT[name, sup] = (R.features(src, SUPPORTS[sup], oracle)["feat"], R.features(tgt, SUPPORTS[sup], oracle)["feat"])
    return _KNOWN_FEAT[name, sup]


def known_result(name, sup, oracle):
    """The restatement alone on a known-answer pair: fpfh_ref.register's dict on the radius features + err + located."""
    if (name, sup) not in _KNOWN:
        src, tgt, truth = K.known_filtered(name)
        fs, ft = known_features(name, sup, oracle)
        r = R.register(src, tgt, SUPPORTS[sup], oracle, stream_id=0, src_feat=fs, tgt_feat=ft, **K.PARAMS)
        r["err"] = None if truth is None else K.pose_error(r["T"], truth)
        r["located"] = bool(truth is not None and r["ok"] and r["err"][0] <= K.OK_T and r["err"][1] <= K.OK_R)
        _KNOWN[name, sup] = r
    return _KNOWN[name, sup]


def known_graph_result(name, sup, oracle):
    """... and through the correspondence graph (pairgraph_ref.register on the same features, its defaults)."""
    if (name, sup) not in _GRAPH:
        src, tgt, _ = K.known_filtered(name)
        fs, ft = known_features(name, sup, oracle)
        _GRAPH[name, sup] = G.register(src, tgt, oracle, src_feat=fs, tgt_feat=ft)
    return _GRAPH[name, sup]


def known_answer_cases(sup, oracle):
    """The names of the pairs the restatement locates at this support: what the device is then held to."""
    return [n for n in K.KNOWN if known_result(n, sup, oracle)["located"]]
