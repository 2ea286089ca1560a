"""The case table of the correspondence-graph registration tests: pair lists (P, Q) and their restatement results
(tests/pairgraph_ref.py is the contract), computed once per session and shared, never modified by a test.

  the ten known-answer pairs of tests/fpfh_cases.py (voxel-filtered, fpfh_ref's features and mutual matches): "known:<name>"
  "planted<M>"   M pairs, about a third of them a rigid motion of random points with 2 cm of noise, the rest uniform
                 outliers; M = 0, 1, 2, 3, 4 and the sizes around the 64-bit word of the bit rows: 63, 64, 65, 129, 257, 1025
  "dup"          a planted list in which every pair of the first 30 occurs twice more
  "odd"          a planted list with NaN and infinite rows on either side
  "all"          130 pairs of a pure translation: every pair compatible with every other
  "none"         66 pairs on two lines of different pitch: no two compatible

and the lists that walk the score kernel's row widths (WIDE; lanes_per_row is the power of two >= min(words, 64)):
  "planted<M>"   M = 513, 600, 1000, 1024 (9, 10, 16, 16 words: 16 lanes per row), 2049, 4096 (33, 64 words: 64 lanes), 4097,
                 4161 (65, 66 words: rows streamed 64 words at a time); up to 5 scoring chunks and 3 accumulation blocks
  "all<M>"       M = 64 (one word of 64 set bits but the diagonal's, walked by 64 teams), 2049, 4100: "all" at those sizes
  "cliques"      270 pairs in seven groups of CLIQUES pairs, every pair of a group compatible and no pair across groups,
                 the groups interleaved by a fixed permutation: every number of G1 - G4 has a closed form (cliques_expected)

Every list is checked on the CPU to have no EDGE-flagged entry (test_pairgraph_cases_cpu.py): the cap is zero."""
import functools

import numpy as np

import fpfh_cases
import fpfh_ref as F
import pairgraph_ref as G

PARAMS = dict(G.DEFAULTS)
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 129, 257, 1025)
KNOWN = tuple(fpfh_cases.KNOWN)
SAME_WORLD = tuple(n for n in KNOWN if len(fpfh_cases.KNOWN[n]) == 4)
SYNTH = tuple("planted%d" % m for m in SIZES) + ("dup", "odd", "all", "none")
WIDE_SIZES = (513, 600, 1000, 1024, 2049, 4096, 4097, 4161)
ALL_SIZES = (64, 2049, 4100)
WIDE = tuple("planted%d" % m for m in WIDE_SIZES) + tuple("all%d" % m for m in ALL_SIZES)
CLIQUES = (130, 65, 64, 5, 3, 2, 1)         # pairs of group g; the largest at g = 0, where its pose has no lever arm
CLIQUES_T = (0.75, -0.5, 0.25)              # the common translation (exact in float32)
OK_T, OK_R = fpfh_cases.OK_T, fpfh_cases.OK_R


def _motion(rng):
    from gloc3d_amd import synth
    T = synth.se3(rng.uniform(-180.0, 180.0), (rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-0.5, 0.5)))
    return np.asarray(T, np.float64)


def planted(m, seed, share=0.35):
    """(P, Q float32 [m, 3], planted [m] bool, T): planted pairs obey q = T p + noise; the others pair random points."""
    rng = np.random.default_rng(seed)
    T = _motion(rng)
    P = rng.uniform((-30, -30, -2), (30, 30, 4), (m, 3))
    n_in = min(m, max(3, int(round(share * m)))) if m >= 3 else 0
    mask = np.zeros(m, bool)
    mask[rng.permutation(m)[:n_in]] = True
    Q = rng.uniform((-30, -30, -2), (30, 30, 4), (m, 3))
    Q[mask] = P[mask] @ T[:3, :3].T + T[:3, 3] + rng.normal(0.0, 0.02, (n_in, 3))
    return np.ascontiguousarray(P, np.float32), np.ascontiguousarray(Q, np.float32), mask, T


def _all(m, seed):
    """m pairs of a pure translation of uniform points: every pair compatible with every other."""
    rng = np.random.default_rng(seed)
    P = rng.uniform((-30, -30, -2), (30, 30, 4), (m, 3)).astype(np.float32)
    T = np.eye(4)
    T[:3, 3] = (2.5, -1.25, 0.5)
    return P, np.ascontiguousarray(P + np.float32([2.5, -1.25, 0.5]), np.float32), np.ones(m, bool), T


def all_expected(m, n_seeds=64):
    """The closed form of "all<m>": a complete graph.  Every degree m - 1, every S_ij = m - 2, every score (m - 1)(m - 2); the
    seeds are positions 0, 1, ...; every seed's set is the whole list and so are its inliers; the first seed wins."""
    k = min(m, n_seeds)
    seeds = np.full(n_seeds, G.NONE, np.uint32)
    seeds[:k] = np.arange(k)
    per_seed = np.zeros(n_seeds, np.uint32)
    per_seed[:k] = m
    return dict(degree=np.full(m, m - 1, np.uint32), score=np.full(m, (m - 1) * (m - 2), np.uint64), seeds=seeds, set_sizes=per_seed,
                seed_inliers=per_seed.copy(), winner_rank=0, inliers=m, ok=True)


@functools.lru_cache(maxsize=None)
def _cliques():
    """(P, Q, None, T, group [M]): group g's pairs are local points within +-2.5 m about (50 g, 0, 0) in P and the same local
    points about (120 g, 0, 0) in Q, moved by CLIQUES_T.  Inside a group the two lengths are equal (up to float32 rounding of
    coordinates below 1000 m, 1e-4 m); across groups a, b the local parts differ by at most 5 sqrt(3) < 8.7 m in either
    cloud, so the lengths are within 8.7 m of 50 |a - b| and 120 |a - b| and differ by at least 70 - 17.4 = 52.6 m: far from
    any threshold on both sides.  A fixed permutation deals the positions out, so every group lies across the 64-bit words."""
    rng = np.random.default_rng(4243)
    M = sum(CLIQUES)
    group = np.repeat(np.arange(len(CLIQUES)), CLIQUES)[rng.permutation(M)]
    local = rng.uniform(-2.5, 2.5, (M, 3)).astype(np.float32)
    P, Q = local.copy(), local + np.float32(CLIQUES_T)
    P[:, 0] += np.float32(50.0) * group.astype(np.float32)
    Q[:, 0] += np.float32(120.0) * group.astype(np.float32)
    T = np.eye(4)
    T[:3, 3] = CLIQUES_T
    return np.ascontiguousarray(P, np.float32), np.ascontiguousarray(Q, np.float32), None, T, group


def cliques_expected(n_seeds=64):
    """The closed form of "cliques", no restatement involved.  A member of a group of n has degree n - 1; S_ij = n - 2 inside
    the group, so its score is (n - 1)(n - 2).  Seeds: score descending, then position.  A seed's row maximum is n - 2: zero
    for n = 1, 2 (no set, size 0, no hypothesis), otherwise every S of the row equals the maximum and the set is the group,
    n members; its fit is the group's translation, which no pair of another group follows within 50 m: n inliers.  The
    winner is rank 0, the first member of the largest group, with its n inliers; + group [M] and block (C as it must be)."""
    group = _cliques()[4]
    M = len(group)
    n = np.asarray(CLIQUES)[group]
    score = ((n - 1) * (n - 2)).astype(np.uint64)
    order = np.lexsort((np.arange(M), -score.astype(np.int64)))[:n_seeds]
    seeds = np.full(n_seeds, G.NONE, np.uint32)
    seeds[:len(order)] = order
    per_seed = np.zeros(n_seeds, np.uint32)
    per_seed[:len(order)] = np.where(n[order] >= 3, n[order], 0)
    return dict(degree=(n - 1).astype(np.uint32), score=score, seeds=seeds, set_sizes=per_seed, seed_inliers=per_seed.copy(),
                winner_rank=0, inliers=max(CLIQUES), ok=True, group=group,
                block=(group[:, None] == group[None, :]) & ~np.eye(M, dtype=bool))


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """(P, Q, planted mask or None, truth or None) of a synthetic list."""
    if name.startswith("all") and name != "all":
        return _all(int(name[3:]), 43 + int(name[3:]))
    if name == "cliques":
        return _cliques()[:4]
    if name.startswith("planted"):
        m = int(name[7:])
        return planted(m, 500 + m)
    if name == "dup":
        P, Q, mask, T = planted(90, 41)
        rep = np.concatenate([np.arange(90), np.arange(30), np.arange(30)])
        return np.ascontiguousarray(P[rep]), np.ascontiguousarray(Q[rep]), mask[rep], T
    if name == "odd":
        P, Q, mask, T = planted(100, 42)
        P, Q = P.copy(), Q.copy()
        P[3] = np.nan
        Q[10, 1] = np.inf
        P[50, 2], Q[50, 0] = -np.inf, np.nan
        Q[64] = np.nan
        P[99, 0] = np.inf
        mask[[3, 10, 50, 64, 99]] = False
        return P, Q, mask, T
    if name == "all":
        return _all(130, 43)
    if name == "none":
        i = np.arange(66, dtype=np.float32)
        z = np.zeros(66, np.float32)
        return np.stack([i, z, z], 1), np.stack([3 * i, z + 1, z], 1), None, None
    raise KeyError(name)


_LISTS, _RESULTS = {}, {}


def pair_list(name, oracle):
    """(P, Q, planted mask or None, truth or None) of any case of the table."""
    if name not in _LISTS:
        if name.startswith("known:"):
            src, tgt, truth = fpfh_cases.known_filtered(name[6:])
            fs = F.features(src, PARAMS["normal_k"], PARAMS["feature_k"], oracle)["feat"]
            ft = F.features(tgt, PARAMS["normal_k"], PARAMS["feature_k"], oracle)["feat"]
            idx, _ = F.match(fs, ft, True)
            keep = np.flatnonzero(idx != F.NONE)
            _LISTS[name] = (np.ascontiguousarray(src[keep]), np.ascontiguousarray(tgt[idx[keep]]), None, truth)
        else:
            _LISTS[name] = synthetic(name)
    return _LISTS[name]


CASES = tuple("known:" + n for n in KNOWN) + SYNTH
EXTRA = WIDE + ("cliques",)


def result(name, oracle, **over):
    """pairgraph_ref.graph of a case at PARAMS (+ over), once per session; + err (m, deg) and located for a known pair.
    C and S are None for a list longer than pairgraph_ref.KEEP_MATRICES (150 MB a case at 4 100 pairs, kept all session)."""
    key = (name, tuple(sorted(over.items())))
    if key not in _RESULTS:
        P, Q, _, truth = pair_list(name, oracle)
        r = G.graph(P, Q, oracle, **dict(PARAMS, **over))
        r["err"] = None if truth is None or not name.startswith("known:") else fpfh_cases.pose_error(r["T"], truth)
        r["located"] = bool(r["err"] is not None and r["ok"] and r["err"][0] <= OK_T and r["err"][1] <= OK_R)
        _RESULTS[key] = r
    return _RESULTS[key]
