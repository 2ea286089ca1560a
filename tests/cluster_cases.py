"""The shared cases of the Euclidean clusters and outlier filters (tests/cluster_ref.py): small clouds, seeded, each built
to reach one clause of E1 - E7 or one path of the kernels.  CASES: name -> (cloud function, dict(tolerance, min_size,
max_size)); fuzz(seed): 30 random clouds whose component counts range from 1 to n; FILTER_PARAMS / filter_cloud(): the stages
of E7."""
import functools

import numpy as np

import cluster_ref as E

R = 0.5                                                    # the tolerance of the hand-made cases
R32 = np.float32(R)


def _one():
    return np.array([[1.0, -2.0, 0.5]], np.float32)


def _pair_at_r():                                          # d2 = 0.25 = r2 exactly: linked
    return np.array([[0, 0, 0], [R32, 0, 0]], np.float32)


def _pair_beyond_r():                                      # one ulp more: (0.5 + 2^-24)^2 rounds above 0.25
    return np.array([[0, 0, 0], [np.nextafter(R32, np.float32(1)), 0, 0]], np.float32)


def _chain(n=130, y=0.0):                                  # 0.9 r apart: one component through three chunks of 64
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = np.arange(n, dtype=np.float32) * np.float32(0.9 * R)
    p[:, 1] = y
    return p


def _chain_shuffled():                                     # the root is index 0 of the shuffle, not a spatial end
    return _chain()[np.random.default_rng(5).permutation(130)]


def _two_chains():                                         # interleaved in upload order, 1.5 r apart: two components
    out = np.empty((200, 3), np.float32)
    out[0::2], out[1::2] = _chain(100), _chain(100, 1.5 * R)
    return out


def _duplicates():
    return np.tile(np.array([[3.25, -1.5, 0.75]], np.float32), (300, 1))


def _isolated():                                           # a grid 2 r apart, shuffled: 257 components
    g = np.stack(np.meshgrid(np.arange(17), np.arange(16), indexing="ij"), -1).reshape(-1, 2)[:257]
    p = np.zeros((257, 3), np.float32)
    p[:, :2] = g * np.float32(2 * R)
    return p[np.random.default_rng(6).permutation(257)]


def _one_component():                                      # a random walk of steps below r, shuffled: one component of 257
    rng = np.random.default_rng(7)
    step = rng.standard_normal((257, 3))
    step *= (0.8 * R) / np.linalg.norm(step, axis=1, keepdims=True)
    return np.cumsum(step, axis=0).astype(np.float32)[rng.permutation(257)]


def _non_finite():                                         # NaN and +-inf rows among clumps
    rng = np.random.default_rng(8)
    p = (rng.standard_normal((400, 3)) * 0.4 + rng.integers(0, 4, (400, 1)) * 3.0).astype(np.float32)
    p[3::17, 0] = np.nan
    p[5::23, 1] = np.inf
    p[7::29, 2] = -np.inf
    p[11::31] = np.nan
    return p


def _slab():                                               # 66 chunks, every box within r of the 65 others: the ballot loop's second round
    rng = np.random.default_rng(9)
    p = rng.uniform((-10, -10, -0.5), (10, 10, 0.5), (4200, 3)).astype(np.float32)
    p[::600] += np.float32(200.0) * (1 + np.arange(7, dtype=np.float32))[:, None]     # seven points on their own, far out
    return p


def _sizes():                                              # components of 5, 5, 4, 3, 6, 1, 4 points, 10 m apart, upload order mixed
    rng = np.random.default_rng(10)
    blobs = [np.array([10.0 * b, 0, 0]) + rng.uniform(-0.1, 0.1, (k, 3)) for b, k in enumerate((5, 5, 4, 3, 6, 1, 4))]
    p = np.concatenate(blobs).astype(np.float32)
    return p[rng.permutation(len(p))]


CASES = {
    "one": (_one, dict(tolerance=R)),
    "pair_at_r": (_pair_at_r, dict(tolerance=R)),
    "pair_beyond_r": (_pair_beyond_r, dict(tolerance=R)),
    "chain": (_chain, dict(tolerance=R)),
    "chain_shuffled": (_chain_shuffled, dict(tolerance=R)),
    "two_chains": (_two_chains, dict(tolerance=R)),
    "duplicates": (_duplicates, dict(tolerance=R)),
    "isolated": (_isolated, dict(tolerance=R)),
    "one_component": (_one_component, dict(tolerance=R)),
    "non_finite": (_non_finite, dict(tolerance=0.6)),
    "non_finite_min3": (_non_finite, dict(tolerance=0.3, min_size=3)),
    "slab": (_slab, dict(tolerance=40.0)),
    "slab_fine": (_slab, dict(tolerance=0.35, min_size=2)),
    "sizes_all": (_sizes, dict(tolerance=R)),                       # equal sizes: the tie goes to the smaller root
    "sizes_4_5": (_sizes, dict(tolerance=R, min_size=4, max_size=5)),   # 4 = min and 5 = max stay, 3 and 6 go
    "sizes_min6": (_sizes, dict(tolerance=R, min_size=6)),
    "sizes_max1": (_sizes, dict(tolerance=R, min_size=0, max_size=1)),
    "sizes_none": (_sizes, dict(tolerance=R, min_size=7)),          # nothing is kept
}


@functools.lru_cache(maxsize=None)
def cloud(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def ref(name):
    """The restatement's answer on a case, computed once and shared (read only)."""
    return E.cluster(cloud(name), **CASES[name][1])


# ---- fuzz ------------------------------------------------------------------------------------------------------------------
N_FUZZ = 30


@functools.lru_cache(maxsize=None)
def fuzz(seed):
    """(xyz [n, 3] float32, tolerance): n in [1, 3000], the square of a uniform draw with the ends and the chunk size put in
    by hand; uniform box, clumps, or a planar ring of ground returns; the tolerance from far below the typical spacing (n
    components) to the cloud's extent (one)."""
    rng = np.random.default_rng(1000 + seed)
    n = {4: 1, 9: 3000, 14: 2, 19: 64, 24: 65}.get(seed, 1 + int(2999 * rng.uniform() ** 2))
    layout = seed % 3
    if layout == 0:
        p = rng.uniform(-5, 5, (n, 3))
    elif layout == 1:
        p = rng.standard_normal((n, 3)) * 0.3 + rng.integers(0, 1 + n // 40, (n, 1)) * np.array([[2.5, 1.0, 0.0]])
    else:
        az, rad = rng.uniform(0, 2 * np.pi, n), rng.choice(np.array([4.0, 6.5, 10.0]), n) + rng.normal(0, 0.02, n)
        p = np.stack([rad * np.cos(az), rad * np.sin(az), rng.normal(0, 0.01, n)], 1)
    p = p.astype(np.float32)
    spacing = 10.0 / max(n, 2) ** (1 / 3)
    kind = seed % 5
    if kind == 0:
        tol = 100.0                                        # spans the cloud: one component
    elif kind == 1:
        tol = 1e-7                                         # below any spacing: every point on its own
    else:
        tol = spacing * float(np.exp(rng.uniform(np.log(0.2), np.log(3.0))))
    if seed % 7 == 3 and n > 4:
        p[rng.integers(0, n, 3)] = np.nan
    return p, float(np.float32(tol))


@functools.lru_cache(maxsize=None)
def fuzz_ref(seed):
    p, tol = fuzz(seed)
    return E.cluster(p, tol)


# ---- E5 - E7 ---------------------------------------------------------------------------------------------------------------
FILTER_PARAMS = dict(min_range=1.5, max_range=30.0, ror_radius=0.6, ror_min_neighbors=3, sor_mean_k=8, sor_std_mul=1.0,
                     cluster_tolerance=0.7, cluster_min_size=10, cluster_max_size=0)
SINGLE_STAGES = {
    "range": dict(min_range=1.5, max_range=30.0),
    "range_max_only": dict(max_range=12.0),
    "range_min_only": dict(min_range=6.0),
    "ror": dict(ror_radius=0.6, ror_min_neighbors=3),
    "ror_none_needed": dict(ror_radius=0.25, ror_min_neighbors=0),   # every finite point stays
    "sor": dict(sor_mean_k=8, sor_std_mul=1.0),
    "sor_k1": dict(sor_mean_k=1, sor_std_mul=0.0),
    "sor_k15": dict(sor_mean_k=15, sor_std_mul=-0.25),
    "cluster": dict(cluster_tolerance=0.7, cluster_min_size=10),
    "cluster_max": dict(cluster_tolerance=0.7, cluster_min_size=2, cluster_max_size=400),
}


@functools.lru_cache(maxsize=None)
def filter_cloud():
    """1 500 points: a dense ground patch and two walls, a few dozen stray points, points beyond and below the ranges,
    duplicates, and non-finite rows."""
    rng = np.random.default_rng(77)
    ground = np.concatenate([rng.uniform(-8, 8, (800, 2)), rng.normal(-1.7, 0.02, (800, 1))], 1)
    wall1 = np.stack([rng.uniform(3, 9, 250), np.full(250, 6.0) + rng.normal(0, 0.02, 250), rng.uniform(-1.7, 1.0, 250)], 1)
    wall2 = np.stack([np.full(200, -7.0) + rng.normal(0, 0.02, 200), rng.uniform(-4, 4, 200), rng.uniform(-1.7, 0.5, 200)], 1)
    stray = rng.uniform(-25, 25, (120, 3))
    far = rng.uniform(-60, 60, (60, 3))
    near = rng.uniform(-0.8, 0.8, (40, 3))
    p = np.concatenate([ground, wall1, wall2, stray, far, near]).astype(np.float32)
    p = p[rng.permutation(len(p))]
    p[100:110] = p[90:100]                                 # exact duplicates
    p[7::211, 0] = np.nan
    p[13::307, 2] = np.inf
    return p
