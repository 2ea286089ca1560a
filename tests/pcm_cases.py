"""Seeded cases for the tests of gloc_pgo_consistency (tests/pcm_ref.py is the contract): the noisy family on
pgo_cases.graph, whose results are restated by the reference, and a closed-form family whose results follow from its
construction."""
import functools

import numpy as np

import pcm_ref as M
import pgo_cases as G

LD = np.longdouble
DRIFT = (0.002, 0.02)            # pgo_cases.graph's own drift: rad and m per step, the steps being the default path
# name -> (n, closures, seed, outliers, undrifted start, (drift_rot, drift_trans) of the params)
NOISY = {
    "n60_undrifted": (60, 64, 5, 0.3, True, (0.0, 0.0)),
    "n60_drift0": (60, 64, 5, 0.3, False, (0.0, 0.0)),
    "n60_own": (60, 64, 5, 0.3, False, DRIFT),
    "n120_drift0": (120, 129, 7, 0.5, False, (0.0, 0.0)),
    "n120_own": (120, 129, 7, 0.5, False, DRIFT),
    "n200_drift0": (200, 257, 9, 0.6, False, (0.0, 0.0)),
    "n200_own": (200, 257, 9, 0.6, False, DRIFT),
}


def closures_of(g, poses=None):
    """The closure edges of a pgo_cases graph as gloc_pgo_consistency takes them; `path` is the node index."""
    c = ~g["odo"]
    P = g["init"] if poses is None else poses
    return dict(poses=P, src=g["src"][c], tgt=g["tgt"][c], Z=g["Z"][c], info=g["info"][c], path=np.arange(len(P), dtype=np.float64),
                outlier=g["outlier"][c])


@functools.lru_cache(maxsize=None)
def noisy(name):
    """(case, params): the case is closures_of() of the graph, params the overrides of the defaults."""
    n, closures, seed, outliers, undrifted, drift = NOISY[name]
    g = G.graph(n, closures, seed=seed, noise=1.0, outliers=outliers, drift=(0, 0) if undrifted else DRIFT)
    return closures_of(g), dict(drift_rot=drift[0], drift_trans=drift[1])


@functools.lru_cache(maxsize=None)
def restated(name, long=False):
    """The reference's results on a noisy case, computed once per process and precision; callers do not write into them."""
    c, prm = noisy(name)
    return M.consistency(c["poses"], c["src"], c["tgt"], c["Z"], c["info"], c["path"], LD if long else np.float64, **prm)


# ---- the closed-form family ---------------------------------------------------------------------------------------------------
GROUPS = (130, 65, 64, 5, 3, 2, 1)               # L = 270


def scaled_groups(L):
    """GROUPS scaled to L closures: the first group takes what rounding leaves, the order of sizes stays strict at the top."""
    if L == sum(GROUPS):
        return GROUPS
    f = L / sum(GROUPS)
    g = [max(1, int(s * f)) for s in GROUPS[1:]]
    return (L - sum(g),) + tuple(g)


@functools.lru_cache(maxsize=None)
def cliques(L=270, seed=11, n=40):
    """Poses at the truth; closure a of group g measures Z = T_j^-1 G_g T_i with one rigid motion G_g per group, the groups'
    motions 20 m apart (G_0 is the identity: the largest group is the true one).  Within a group the cycle through two
    closures closes to float32 rounding of Z; across groups it misses by the difference of two motions, 20 m or more
    against centimetres of Sigma.  group [L]: the group of each position, dealt by a fixed permutation."""
    rng = np.random.default_rng(seed)
    sizes = scaled_groups(L)
    group = np.repeat(np.arange(len(sizes)), sizes)[rng.permutation(L)]
    truth = G.trajectory(n, rng)
    motions = [np.eye(4)] + [G.se3(rng.normal(size=3) * 0.2, [20.0 * g, 0.0, 0.0]) for g in range(1, len(sizes))]
    src, tgt = np.empty(L, np.uint32), np.empty(L, np.uint32)
    for a in range(L):
        i, j = rng.integers(0, n, 2)
        while abs(int(i) - int(j)) < 2:
            i, j = rng.integers(0, n, 2)
        src[a], tgt[a] = i, j
    Z = np.array([np.linalg.inv(truth[j]) @ motions[g] @ truth[i] for i, j, g in zip(src, tgt, group)]).astype(np.float32)
    info = G.random_info(rng, 8)[rng.integers(0, 8, L)]
    return dict(poses=truth, src=src, tgt=tgt, Z=Z, info=info, path=None, group=group, sizes=np.array(sizes))


def cliques_expected(c):
    """degree, score, and the winner's mask by construction."""
    n = c["sizes"][c["group"]].astype(np.int64)
    return dict(degree=(n - 1).astype(np.uint32), score=((n - 1) * (n - 2)).astype(np.uint64), mask=(c["group"] == 0).astype(np.uint8),
                winner_seed=int(np.flatnonzero(c["group"] == 0)[0]), clique_size=int(c["sizes"][0]))
