"""The case table of the Fast Global Registration tests: pair lists (P, Q) and their restatement results (tests/fgr_ref.py
is the contract), computed once per session and shared, never modified by a test.  The lists are pairgraph_cases' own
generators:

  the ten known-answer pairs of tests/fpfh_cases.py (voxel-filtered, fpfh_ref's features and mutual matches): "known:<name>"
  "planted<M>"   M = 0, 1, 2, 3, 4, 63, 64, 65, 257, 1025, and 4096 | 4097: either side of the 4096 active pairs the GNC
                 kernel keeps in LDS (reached with tuple_tries = 0, where every finite pair is active; with the test on, at
                 most 3 max_tuples pairs are)
  "dup", "odd", "all", "none"
  "line"         P_i = (i, 0, 0), Q_i = (i + 1, 0, 0), i < 40: every tuple passes, H[0][0] is exactly 0, so the first update
                 is degenerate with no rounding involved: status 2, the identity, ok = 0

("cliques" is left out on purpose: its GNC runs into a singular system near update 55, and where exactly depends on
rounding.)  ROWS are the parameter rows the device is compared at; test_fgr_cases_cpu.py holds that at every row no
synthetic list has an EDGE-flagged tuple edge, and that no Cholesky pivot of any case comes near the degeneracy rule."""
import numpy as np

import fgr_ref as R
import fpfh_cases
import pairgraph_cases as PG

PARAMS = dict(R.DEFAULTS)
LDS_CAP = 4096
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 257, 1025, LDS_CAP, LDS_CAP + 1)
KNOWN = tuple(fpfh_cases.KNOWN)
SAME_WORLD = tuple(n for n in KNOWN if len(fpfh_cases.KNOWN[n]) == 4)
SYNTH = tuple("planted%d" % m for m in SIZES) + ("dup", "odd", "all", "none", "line")
CASES = tuple("known:" + n for n in KNOWN) + SYNTH
OK_T, OK_R = fpfh_cases.OK_T, fpfh_cases.OK_R
EDGE_CAP = fpfh_cases.EDGE_CAP

# the parameter rows of the device tests (name -> overrides of PARAMS); max_iters 4 | 5 crosses the first anneal step
ROWS = dict(default={}, iters1=dict(max_iters=1), iters4=dict(max_iters=4), iters5=dict(max_iters=5), no_test=dict(tuple_tries=0),
            one_tuple=dict(max_tuples=1), anneal1=dict(anneal_every=1))
SCALE1 = dict(tuple_scale=1.0)   # on "all" only

# The same-world known pairs the restatement locates at PARAMS (stream 0), as computed: ok and within OK_T / OK_R of truth.
# Seven of the eight; "yaw135_2m" is the miss (4 inliers, 3.7 m / 91 degrees off).
LOCATED = ("yaw0_1m", "yaw45_2m", "yaw90_0m", "yaw90_3m", "yaw170_1m", "yaw180_4m", "yaw180_0m")

# The GNC has no stop test, so a run on few pairs can anneal itself into a singular system: with max_tuples = 1 (three active
# pairs) these two lists do, at updates 18 and 8, after pivots that pass the 1e-12 rule by a factor of 1.1 and 1.7 -- where
# such a run ends hangs on rounding, as it does for "cliques".  Every other (case, row) keeps its pivots a factor 1e3 or
# more above the rule, or fails it with a pivot of exactly 0 (test_fgr_cases_cpu.py).
NEAR_RULE = (("planted257", "one_tuple"), ("planted1025", "one_tuple"))

# The synthetic (case, row) runs with pairs within 1e-4 + 1e-4 |x| of the inlier threshold, and how many: poses that are not
# converged (one update) or fitted to one tuple, on the two longest lists.  Every other synthetic run has none.
NEAR_THRESH = {("planted4096", "iters1"): 1, ("planted4096", "one_tuple"): 5, ("planted4097", "iters1"): 4}

_RESULTS = {}


def ok_hangs_on_flagged_pairs(r):
    """Could the pairs flagged near the inlier threshold carry the inlier count across what ok asks for?  Only then may two
    correct evaluations differ in ok.  No run of this table does (test_fgr_cases_cpu.py)."""
    return r["near"] > 0 and r["status"] == 0 and abs(r["inliers"] - r["need"]) <= r["near"]


def pair_list(name, oracle):
    """(P, Q, planted mask or None, truth or None) of any case of the table."""
    if name == "line":
        i = np.arange(40, dtype=np.float32)
        z = np.zeros(40, np.float32)
        return np.stack([i, z, z], 1), np.stack([i + 1, z, z], 1), None, None
    return PG.pair_list(name, oracle)


def result(name, oracle, **over):
    """fgr_ref.fgr of a case at PARAMS (+ over), stream 0, once per session; + err (m, deg) and located for a known pair."""
    key = (name, tuple(sorted(over.items())))
    if key not in _RESULTS:
        P, Q, _, truth = pair_list(name, oracle)
        r = R.fgr(P, Q, oracle, **dict(PARAMS, **over))
        r["err"] = None if truth is None or not name.startswith("known:") else fpfh_cases.pose_error(r["T"], truth)
        r["located"] = bool(r["err"] is not None and r["ok"] and r["err"][0] <= OK_T and r["err"][1] <= OK_R)
        _RESULTS[key] = r
    return _RESULTS[key]
