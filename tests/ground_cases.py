"""Case table of the ground pre-alignment sweep (pure numpy): cloud shapes for the k-NN and the normals, estimate scenes that
reach one branch each, and the parameter rows.  tests/test_ground_cases_cpu.py proves on the oracle that every case reaches
what it is named for; tests/test_ground_sweep_gpu.py runs the same cases through the C ABI.

Also here: the k-NN stated in plain fp32 numpy (the oracle's operation order) and the normals' covariance solved by
numpy.linalg.eigh, the two independent references the oracle itself is held to on these shapes."""
import numpy as np

from util import ground_scene

NONE = 0xFFFFFFFF
FLT_MAX = np.float32(np.finfo(np.float32).max)

# ---- parameters ------------------------------------------------------------------------------------------------------------

DEFAULTS = dict(near_range2=400.0, knn=10, plane_thresh=0.1, ransac_iters=1000, ransac_conf=0.99, seed=0)
REQUIRED_VALUES = dict(knn=(3, 6, 16), ransac_iters=(1, 255, 257, 65536), ransac_conf=(-1.0, 0.0, 0.5, 0.99, 1.0, 2.0),
                       seed=(0, 1, 2), plane_thresh=(0.01, 0.3), near_range2=(25.0, 400.0, 1e6))
K_ENTRY = (1, 2, 3, 10, 16)          # the bare k-NN entry point; the normals' entry point takes those >= 3


def _rows():
    """The defaults, every listed value with the others at their defaults, and a few rows that move several at once."""
    rows = [dict(DEFAULTS)]
    for f, values in REQUIRED_VALUES.items():
        rows += [dict(DEFAULTS, **{f: v}) for v in values if v != DEFAULTS[f]]
    rows += [dict(DEFAULTS, ransac_iters=65536, ransac_conf=0.0),                 # every one of 65536 hypotheses counts
             dict(DEFAULTS, ransac_iters=257, ransac_conf=2.0, plane_thresh=0.01, knn=16, seed=2),
             dict(DEFAULTS, ransac_iters=255, ransac_conf=0.5, plane_thresh=0.3, knn=3, seed=1, near_range2=25.0),
             dict(DEFAULTS, ransac_iters=1, ransac_conf=1.0, knn=6)]
    return rows


PARAM_ROWS = _rows()
FIELDS = tuple(DEFAULTS)


def row_id(row):
    d = ["%s=%g" % (f, row[f]) for f in FIELDS if row[f] != DEFAULTS[f]]
    return ",".join(d) or "defaults"


# ---- cloud shapes for the k-NN and the normals -----------------------------------------------------------------------------

# (447 is 7 chunks: with it the chunk count takes every value modulo the 4 waves of a work-group)
SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 321, 447, 4033, 4095, 4097, 4161)


def _uniform(m, seed):
    return np.random.default_rng(seed).uniform(-5, 5, (m, 3)).astype(np.float32)


def _identical():
    return np.tile(np.array([1.5, -2.25, 0.75], np.float32), (1000, 1))


def _lattice():
    g = np.arange(12, dtype=np.float32) - 5
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return p[np.random.default_rng(11).permutation(p.shape[0])]           # index order is not spatial order


def _sheet(z, seed):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(-6, 6, (2500, 2)), np.full(2500, z)].astype(np.float32)


def _line():
    t = np.random.default_rng(13).uniform(-8, 8, 1500)
    return np.c_[t, np.full(1500, 0.5), np.full(1500, -1.5)].astype(np.float32)


def _clusters_outliers():
    rng = np.random.default_rng(14)
    centres = rng.uniform(-5, 5, (5, 3))
    pts = [c + 0.01 * rng.standard_normal((500, 3)) for c in centres]
    d = rng.standard_normal((40, 3))
    pts.append(1e3 * d / np.linalg.norm(d, axis=1, keepdims=True) + rng.uniform(-1, 1, (40, 3)))
    p = np.concatenate(pts).astype(np.float32)
    return p[rng.permutation(p.shape[0])]


def _far_offset():
    return (np.random.default_rng(15).uniform(0, 1, (3000, 3)) + np.array([8000.0, -8000.0, 8000.0])).astype(np.float32)


def nonfinite_rows(m=3000):
    """row -> (columns, value) of the `nonfinite` shape: whole rows and single coordinates, the first and the last row."""
    rng = np.random.default_rng(16)
    bad = {0: ((0, 1, 2), np.nan), m - 1: ((1,), np.inf)}
    values = (np.nan, np.inf, -np.inf)
    for n, r in enumerate(rng.choice(np.arange(1, m - 1), 28, replace=False).tolist()):
        cols = (0, 1, 2) if n % 4 == 0 else (int(rng.integers(3)),)
        bad[r] = (cols, values[n % 3])
    bad[63], bad[64] = ((2,), -np.inf), ((0, 1, 2), np.inf)                # two neighbours in the index order
    return bad


def _nonfinite():
    p = _uniform(3000, 16)
    for r, (cols, v) in nonfinite_rows().items():
        p[r, list(cols)] = v
    return p


SHAPES = dict(identical=_identical, lattice=_lattice, sheet=lambda: _sheet(-1.5, 12), sheet_above=lambda: _sheet(2.0, 17),
              line=_line, clusters_outliers=_clusters_outliers, far_offset=_far_offset, nonfinite=_nonfinite)
SHAPES.update({"size%d" % m: (lambda m=m: _uniform(m, 100 + m)) for m in SIZES})
DEGENERATE = ("identical", "line")          # no separated smallest eigenvalue anywhere: exempt from the eigh comparison
# neighbourhood size of the normals on each shape (the eigh comparison and the device's normals); 10 where not listed
NORMALS_K = dict(lattice=16)

_cache = {}


def shape(name):
    if name not in _cache:
        _cache[name] = SHAPES[name]()
        _cache[name].setflags(write=False)
    return _cache[name]


# ---- the k-NN in plain fp32 numpy ------------------------------------------------------------------------------------------

def knn_numpy(p, k, block=512):
    """Ascending (d2, index) lists of the k nearest among the same points, d2 = (dx*dx + dy*dy) + dz*dz in fp32; a distance
    that is not below FLT_MAX (NaN, inf) is no neighbour; short lists are padded with 0xFFFFFFFF / FLT_MAX."""
    p = np.ascontiguousarray(p, np.float32)
    m, kk = p.shape[0], min(k, p.shape[0])
    idx, d2 = np.full((m, k), NONE, np.uint32), np.full((m, k), FLT_MAX, np.float32)
    for b in range(0, m, block):
        q = p[b:b + block]
        with np.errstate(all="ignore"):
            dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            d = np.where(d < FLT_MAX, d, np.float32(np.inf))
        # one integer key per pair, (bits(d2) << 32) | index: non-negative floats order as their bit patterns do, and equal
        # distances then order by the smaller index
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(m, dtype=np.uint64)[None, :]
        key = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1)
        dd = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
        good = np.isfinite(dd)
        idx[b:b + block, :kk] = np.where(good, (key & np.uint64(NONE)).astype(np.uint32), NONE)
        d2[b:b + block, :kk] = np.where(good, dd, FLT_MAX)
    return idx, d2


def tie_share(p, k):
    """Share of the sources whose k-th and (k+1)-th distances are equal (the list then depends on the index rule)."""
    _, d2 = knn_numpy(p, k + 1)
    return float(np.mean(d2[:, k - 1] == d2[:, k]))


# ---- the normals by numpy.linalg.eigh --------------------------------------------------------------------------------------

def normals_eigh(p, idx):
    """(eigenvalues ascending [m, 3], unit eigenvector of the smallest [m, 3], neighbours used [m]) of the fp64 covariance
    of every point's listed neighbours."""
    p64 = np.where(np.isfinite(p), p, 0).astype(np.float64)
    valid = idx != NONE
    cnt = valid.sum(1)
    nb = p64[np.where(valid, idx, 0)] * valid[..., None]
    mean = nb.sum(1) / np.maximum(cnt, 1)[:, None]
    d = (nb - mean[:, None, :]) * valid[..., None]
    w, v = np.linalg.eigh(np.einsum("mka,mkb->mab", d, d))
    return w, v[:, :, 0], cnt


def separation(w):
    """(l1 - l0) / l2, 0 where the largest eigenvalue is 0."""
    with np.errstate(all="ignore"):
        return np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)


def angle_between(a, b):
    """Angle between two lines given by direction vectors (sign-free), accurate near 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(np.einsum("ij,ij->i", a, b)))


# ---- estimate scenes -------------------------------------------------------------------------------------------------------

def with_stride(cloud4, stride, seed=0):
    """The first three columns of a cloud plus stride - 3 channels the transform has to carry along unchanged."""
    n = cloud4.shape[0]
    extra = np.random.default_rng(1000 + seed).uniform(-100, 100, (n, 13)).astype(np.float32)
    extra[:, 0] = cloud4[:, 3] if cloud4.shape[1] > 3 else extra[:, 0]
    return np.ascontiguousarray(np.c_[cloud4[:, :3], extra][:, :stride], np.float32)


def _wall(rng, n, x=8.0):
    return np.c_[np.full(n, x), rng.uniform(-4, 4, n), rng.uniform(-1, 2, n)]


STEP = 2.0 ** -10


def _gadget(site, site_offsets, arms):
    """Points at `site` whose 10 nearest are themselves plus the heads of the arms around them -- a flat neighbourhood, so their
    normal is the vertical -- while every arm is a vertical stack of 11 points 2^-10 apart whose own neighbourhoods are collinear
    (normal along x, bin 9).  So the site points are alone in their bin whatever their own arrangement is."""
    site = np.asarray(site, np.float64)
    rows = [site + o for o in site_offsets]
    for a in arms:
        rows += [site + a + np.array([0.0, 0.0, j * STEP]) for j in range(-5, 6)]
    return np.array(rows)


ARMS_Y = [np.array([0.0, 0.125, 0.0]), np.array([0.0, -0.125, 0.0])]
ARMS_XY = ARMS_Y + [np.array([0.125, 0.0, 0.0]), np.array([-0.125, 0.0, 0.0])]


def _collinear_ground():
    rng = np.random.default_rng(21)
    offs = [np.array([j / 256.0, 0.0, 0.0]) for j in range(-3, 3)]        # six distinct points on the line y = 0, z = -1.75
    parts = [_gadget((2.0 + i, 0.0, -1.75), offs, ARMS_Y) for i in range(8)]
    return np.concatenate(parts + [_wall(rng, 300, 12.0)]).astype(np.float32)


def _duplicate_ground():
    rng = np.random.default_rng(22)
    g = _gadget((4.0, 0.0, -1.75), [np.zeros(3)] * 6, ARMS_XY)
    return np.concatenate([g, _wall(rng, 300)]).astype(np.float32)


def _tiny_bin():
    rng = np.random.default_rng(23)
    g = _gadget((4.0, 0.0, -1.75), [np.zeros(3)] * 2, ARMS_XY)
    return np.concatenate([_wall(rng, 300), g]).astype(np.float32)


def _ceiling_wins():
    rng = np.random.default_rng(24)
    xy = rng.uniform(-5, 5, (1500, 2))
    ceil = np.c_[xy, 2.5 + 0.05 * xy[:, 1] + 0.003 * rng.standard_normal(1500)]
    fxy = rng.uniform(-4, 4, (600, 2))
    floor = np.c_[fxy, -1.7 + 0.003 * rng.standard_normal(600)]
    p = np.concatenate([ceil, floor, _wall(rng, 400)])
    return p[rng.permutation(p.shape[0])].astype(np.float32)


def _bin_tie():
    rng = np.random.default_rng(25)
    ceil = np.c_[rng.uniform(-4, 4, (800, 2)), np.full(800, 2.5)]         # exactly flat: normals exactly -z, bin 0
    floor = np.c_[rng.uniform(-4, 4, (800, 2)), np.full(800, -1.75)]      # normals exactly +z, bin 17
    p = np.concatenate([floor, ceil, _wall(rng, 300)])
    return p[rng.permutation(p.shape[0])].astype(np.float32)


def _mini_scene(n, seed, noise=0.004, bowl=0.0):
    """n points within range: four fifths a slightly tilted noisy floor (curved upward by bowl * r^2, so that the hypotheses'
    inlier counts differ), the rest a wall 2 m beyond its edge."""
    rng = np.random.default_rng(seed)
    nf = (4 * n) // 5
    half = 0.07 * np.sqrt(nf)                                              # ~0.14 m between floor points at any n
    xy = rng.uniform(-half, half, (nf, 2))
    floor = np.c_[xy, -1.7 + 0.03 * xy[:, 0] + bowl * (xy * xy).sum(1) + noise * rng.standard_normal(nf)]
    wall = np.c_[np.full(n - nf, half + 2.0), rng.uniform(-half, half, n - nf), rng.uniform(-1.5, 2, n - nf)]
    p = np.concatenate([floor, wall])
    return p[rng.permutation(n)].astype(np.float32)


FAR_ROW = np.array([30.0, 40.0, 0.0], np.float32)                          # 50 m from the sensor
SEL_TILE = 2048                                                            # flags per tile of the compaction


def many_tiles_rows(n=530000, want=3000):
    """The rows of `many_tiles` that are within range: the first and the last, both sides of the first tile seams, inside tiles
    255..258 (where the sum over the tiles before a tile takes its second round), and a scatter over the rest."""
    rng = np.random.default_rng(27)
    rows = {0, n - 1}
    for j in range(1, 7):
        rows |= {j * SEL_TILE - 1, j * SEL_TILE}
    for t in range(255, 259):
        rows |= {t * SEL_TILE - 1, t * SEL_TILE, (t + 1) * SEL_TILE - 1}
        rows |= set((t * SEL_TILE + rng.choice(SEL_TILE, 150, replace=False)).tolist())
    rows = {r for r in rows if r < n}
    rest = rng.choice(n, want, replace=False).tolist()
    for r in rest:
        if len(rows) >= want:
            break
        rows.add(int(r))
    return np.array(sorted(rows))


def _many_tiles():
    rows = many_tiles_rows()
    cloud = np.tile(FAR_ROW, (530000, 1))
    cloud[rows] = _mini_scene(rows.shape[0], 27)
    return cloud


def _tile_flagged(flagged):
    cloud = np.tile(FAR_ROW, (2 * SEL_TILE, 1))
    cloud[list(flagged)] = _mini_scene(len(flagged), 29)
    return cloud


TILE_LAST_ROWS = (100, SEL_TILE - 1, 3000, 2 * SEL_TILE - 1)


def _lidar(stride, n_az=100):
    cloud, _ = ground_scene(3.0, -2.0, n_az=n_az)
    return with_stride(cloud, stride)


SCENES = dict(lidar3=lambda: _lidar(3), lidar5=lambda: _lidar(5), lidar16=lambda: _lidar(16),
              ceiling_wins=lambda: with_stride(_ceiling_wins(), 5, 1), bin_tie=_bin_tie,
              collinear_ground=_collinear_ground, duplicate_ground=lambda: with_stride(_duplicate_ground(), 16, 2),
              tiny_bin=_tiny_bin,
              multi_slab=lambda: _mini_scene(13507, 26, bowl=0.004),
              many_tiles=_many_tiles,
              tile_edges2047=lambda: _mini_scene(2047, 28), tile_edges2048=lambda: _mini_scene(2048, 28),
              tile_edges2049=lambda: with_stride(_mini_scene(2049, 28), 5, 3),
              tile_edges_last=lambda: _tile_flagged(TILE_LAST_ROWS))
# the two large scenes run at the defaults and one other seed only; every other scene runs every row
FEW_ROWS = {"many_tiles": (dict(DEFAULTS), dict(DEFAULTS, seed=1)), "multi_slab": (dict(DEFAULTS), dict(DEFAULTS, seed=2))}
# parameters at which a scene reaches its branch, where they are not the defaults (ceiling_wins: a seed whose winning sample
# comes out with a downward normal, so that the transform takes its sign flip)
SCENE_PARAMS = dict(ceiling_wins=dict(DEFAULTS, seed=0))


def scene(name):
    key = "scene:" + name
    if key not in _cache:
        _cache[key] = np.ascontiguousarray(SCENES[name](), np.float32)
        _cache[key].setflags(write=False)
    return _cache[key]


def rows_of(name):
    rows = list(FEW_ROWS.get(name, PARAM_ROWS))
    own = SCENE_PARAMS.get(name)
    if own is not None and own not in rows:
        rows.append(own)
    return rows


def big_scene():
    """The lidar scene at the size the other ground tests use (about 16 000 points within range)."""
    if "big" not in _cache:
        _cache["big"] = ground_scene(3.0, -2.0)[0]
        _cache["big"].setflags(write=False)
    return _cache["big"]


def moved_fp64(cloud, T):
    return (cloud[:, :3].astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)).astype(np.float32)
