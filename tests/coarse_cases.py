"""The case table of the coarse (x, y, yaw) matcher's tests: small synthetic occupancy images, an independent numpy
statement of the grid and of the overlap count, and the parameter rows of the sweep.  No GPU and no oracle in here:
tests/test_coarse_cases_cpu.py proves the table against the CPU restatement, tests/test_coarse_sweep_gpu.py holds the
device to the restatement bit for bit.

An occupancy image is uint8, 0 = occupied, 255 = free (below 100 counts as occupied), and comes with (ox, oy, resolution):
pixel (x, y) is voxel (lround(ox / resolution) + x, lround(oy / resolution) + y), voxel ix lies in cell
floor(ix / cell_px) + 256 of a 512 x 512 grid, and what falls outside the grid is dropped.  A pattern is an int array
[n, 2] of cell offsets (du, dv) from the sensor's cell 256; `image_of` turns it into an image with one occupied pixel, picked
by the case's seed, in every cell.

  GRID_CASES       name -> builder of one grid case (`grid_case(name)` caches it): the pattern families at every cell_px of
                   the sweep, and the edges of the grid, the image origin, the threshold and the cell list's size classes
  PARAM_ROWS       the parameter rows of the sweep, in the order the sweep runs them
  SWEEP_PAIRS      (query, database) case stems matched under every row
  known_cases()    known-answer pairs: the database is the query turned by whole quarter turns and shifted by whole cells
  rule_pair(n)     the 1.2 x rule: the identity overlaps 10 cells, the quarter turn n
  EDGE_PAIRS       the acceptance edges (n_query 15 / 16, overlap at and below min_overlap * n_query, the stretched query)
"""
import functools

import numpy as np

G, HALF = 512, 256
FIELDS = ("cell_px", "n_yaw", "max_shift", "top_yaw", "refine", "min_overlap")
DEFAULTS = dict(cell_px=2, n_yaw=360, max_shift=64, top_yaw=12, refine=4, min_overlap=0.25)
# grids remember their resolution and cell_px: one resolution per cell_px (0.2 is the default)
RESOLUTION = {1: 0.5, 2: 0.2, 3: 0.25, 16: 0.1}
CELL_PX = (1, 2, 3, 16)
# what check_params admits (coarse.hip)
BOUNDS = dict(cell_px=(1, 16), n_yaw=(1, 3600), max_shift=(0, 255), top_yaw=(0, 64), refine=(0, 8))


def _row(cell_px, n_yaw, max_shift, top_yaw, refine, min_overlap):
    return dict(cell_px=cell_px, n_yaw=n_yaw, max_shift=max_shift, top_yaw=top_yaw, refine=refine, min_overlap=min_overlap)


# Not the full product.  Within a cell_px the order changes n_yaw on the live handle and changes it back (360, 7, 360, 3600,
# 64, ...): the cached cos / sin table.  Three rows hold n_yaw = 3600, one of them at max_shift = 255 (the restatement needs
# more than a second for that one).
PARAM_ROWS = (
    _row(2, 360, 64, 12, 4, 0.0),
    _row(2, 7, 64, 7, 4, 0.25),          # top_yaw = n_yaw below one stride of 64 lanes
    _row(2, 360, 255, 64, 8, 0.25),      # 1022 lag jobs, 65 candidates, 289 shifts
    _row(2, 3600, 255, 64, 8, 0.25),
    _row(2, 64, 64, 64, 4, 0.25),        # top_yaw = n_yaw = one stride
    _row(2, 65, 5, 64, 0, 1.0),          # one rotation into the second stride
    _row(2, 1, 0, 0, 0, 0.25),           # one rotation, one lag, the identity alone, one shift
    _row(2, 1, 64, 1, 4, 0.25),
    _row(2, 360, 0, 1, 0, 0.25),
    _row(2, 360, 5, 0, 4, 0.25),
    _row(2, 3600, 5, 12, 0, 1.0),
    _row(2, 8, 64, 8, 8, 0.0),
    _row(2, 360, 64, 1, 4, 1.0),
    _row(1, 360, 64, 12, 4, 0.25),
    _row(1, 7, 255, 1, 8, 0.0),
    _row(1, 64, 0, 12, 0, 0.25),
    _row(1, 3600, 64, 64, 4, 0.25),
    _row(3, 360, 64, 12, 4, 0.25),
    _row(3, 65, 255, 64, 8, 1.0),
    _row(3, 7, 5, 0, 0, 0.0),
    _row(3, 64, 5, 1, 4, 0.25),
    _row(16, 360, 64, 12, 4, 0.25),
    _row(16, 65, 0, 64, 8, 0.25),
    _row(16, 1, 255, 0, 4, 1.0),
)
# every one of these values is in some row (test_coarse_cases_cpu.py checks it)
REQUIRED_VALUES = dict(cell_px=(1, 2, 3, 16), n_yaw=(1, 7, 64, 65, 360, 3600), top_yaw=(0, 1, 12, 64), max_shift=(0, 5, 64, 255),
                       refine=(0, 4, 8), min_overlap=(0.0, 0.25, 1.0))


def row_id(row):
    return "px%d-yaw%d-shift%d-top%d-ref%d-min%g" % tuple(row[f] for f in FIELDS)


# ---- the independent statement -------------------------------------------------------------------------------------

def _round_half_away(v):
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def grid_numpy(img, ox, oy, res, cell_px):
    """(cells, dilated): the occupied cells as sorted (v << 16) | u, uint32, and their 3 x 3 dilation as a [512, 512] boolean
    array indexed [v, u].  ox, oy and res are taken as the float32 values the C interfaces receive."""
    img = np.asarray(img, np.uint8)
    ix0 = int(_round_half_away(np.float64(np.float32(ox)) / np.float64(np.float32(res))))
    iy0 = int(_round_half_away(np.float64(np.float32(oy)) / np.float64(np.float32(res))))
    y, x = np.nonzero(img < 100)
    u = np.floor_divide(ix0 + x.astype(np.int64), cell_px) + HALF
    v = np.floor_divide(iy0 + y.astype(np.int64), cell_px) + HALF
    m = (u >= 0) & (u < G) & (v >= 0) & (v < G)
    occ = np.zeros((G, G), bool)
    occ[v[m], u[m]] = True
    vv, uu = np.nonzero(occ)                                  # row-major: sorted by (v, u)
    cells = ((vv.astype(np.uint32) << 16) | uu.astype(np.uint32)).astype(np.uint32)
    return cells, dilate(occ)


def dilate(occ):
    """The 3 x 3 dilation of a [512, 512] boolean map: nothing wraps, nothing leaves the grid."""
    pad = np.zeros((G + 2, G + 2), bool)
    pad[1:-1, 1:-1] = occ
    out = np.zeros((G, G), bool)
    for a in range(3):
        for b in range(3):
            out |= pad[a:a + G, b:b + G]
    return out


def rotated_cells(q_cells, k, n_yaw, cell_px):
    """The cells (u, v int64, inside [n] bool) of the query's cell centres turned by 2 pi k / n_yaw about the sensor: the
    centre of cell u is pixel (u - 256) * cell_px + (cell_px - 1) / 2; the rotation is fp32 and un-fused with cos / sin rounded
    once from fp64; the pixel is rounded with halves away from zero and re-binned by floor division."""
    q = np.asarray(q_cells, np.uint32)
    x = (((q & 0xFFFF).astype(np.int64) - HALF) * cell_px).astype(np.float32) + np.float32(0.5) * np.float32(cell_px - 1)
    y = (((q >> 16).astype(np.int64) - HALF) * cell_px).astype(np.float32) + np.float32(0.5) * np.float32(cell_px - 1)
    a = 2.0 * np.pi * k / n_yaw
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    rx, ry = c * x - s * y, s * x + c * y                     # float32 arrays: every product and sum rounds on its own
    u = np.floor_divide(_round_half_away(rx), cell_px) + HALF
    v = np.floor_divide(_round_half_away(ry), cell_px) + HALF
    return u, v, (u >= 0) & (u < G) & (v >= 0) & (v < G)


def overlap_numpy(q_cells, d_dilated, k, n_yaw, tx, ty, cell_px):
    """The number of query cells that, turned by rotation k of n_yaw and shifted by (tx, ty) cells, fall on a set bit of the
    dilated database map.  A cell that leaves the grid by the rotation or by the shift counts nothing."""
    u, v, m = rotated_cells(q_cells, k, n_yaw, cell_px)
    u, v = u[m] + tx, v[m] + ty
    m = (u >= 0) & (u < G) & (v >= 0) & (v < G)
    return int(np.count_nonzero(d_dilated[v[m], u[m]]))


def best_window(q_cells, d_dilated, k, n_yaw, tx0, ty0, refine, cell_px):
    """(overlap, tx, ty): the largest overlap over the shifts within `refine` of (tx0, ty0), the first in (dy, dx) row-major order
    among equals."""
    best = (-1, 0, 0)
    for dy in range(-refine, refine + 1):
        for dx in range(-refine, refine + 1):
            o = overlap_numpy(q_cells, d_dilated, k, n_yaw, tx0 + dx, ty0 + dy, cell_px)
            if o > best[0]:
                best = (o, tx0 + dx, ty0 + dy)
    return best


# ---- images ---------------------------------------------------------------------------------------------------------

def pack(duv):
    """Cell offsets [n, 2] (du, dv) -> sorted unique (v << 16) | u of those inside the grid."""
    d = np.asarray(duv, np.int64).reshape(-1, 2)
    u, v = d[:, 0] + HALF, d[:, 1] + HALF
    m = (u >= 0) & (u < G) & (v >= 0) & (v < G)
    return np.unique(((v[m] << 16) | u[m]).astype(np.uint32))


def unpack(cells):
    c = np.asarray(cells, np.uint32)
    return np.stack([(c & 0xFFFF).astype(np.int64) - HALF, (c >> 16).astype(np.int64) - HALF], 1)


def image_of(duv, cell_px, seed, margin=2):
    """(img, ox, oy, res) of a pattern: the image spans the pattern's pixels and `margin` free pixels around them; every cell
    gets one occupied pixel, picked by the seed among its cell_px x cell_px."""
    res = RESOLUTION[cell_px]
    d = np.asarray(duv, np.int64).reshape(-1, 2)
    if d.shape[0] == 0:
        return np.full((3, 4), 255, np.uint8), _origin(-2, res), _origin(-1, res), res
    rng = np.random.default_rng(seed)
    px = d * cell_px + rng.integers(0, cell_px, d.shape)
    lo = d.min(0) * cell_px - margin
    hi = d.max(0) * cell_px + cell_px - 1 + margin
    img = np.full((hi[1] - lo[1] + 1, hi[0] - lo[0] + 1), 255, np.uint8)
    img[px[:, 1] - lo[1], px[:, 0] - lo[0]] = 0
    return img, _origin(lo[0], res), _origin(lo[1], res), res


def _origin(ix0, res):
    """The metric origin of an image whose first pixel is voxel ix0 (float32, as the interfaces take it)."""
    o = float(np.float32(int(ix0) * np.float64(np.float32(res))))
    assert int(_round_half_away(np.float64(np.float32(o)) / np.float64(np.float32(res)))) == int(ix0)
    return o


# ---- patterns (cell offsets from the sensor) ------------------------------------------------------------------------------

def p_random(seed, n=300, reach=60):
    rng = np.random.default_rng(seed)
    return unpack(pack(rng.integers(-reach, reach + 1, (n, 2))))


def p_lshape():
    """An L with a bar: no rotation by a multiple of a quarter turn maps it onto itself."""
    leg = [(-40, v) for v in range(-30, 41)] + [(-39, v) for v in range(-30, 41)]
    foot = [(u, -30) for u in range(-38, 31)] + [(u, -29) for u in range(-38, 31)]
    bar = [(u, 12 + (u // 9)) for u in range(-10, 46)]
    dots = [(25, 40), (31, 33), (50, -12), (7, -55), (-55, 7), (18, 27)]
    return unpack(pack(leg + foot + bar + dots))


def p_square(h=8):
    a = np.arange(-h, h + 1)
    return np.stack(np.meshgrid(a, a), -1).reshape(-1, 2)


def p_plus(arm=30, w=1):
    a, b = np.arange(-arm, arm + 1), np.arange(-w, w + 1)
    return unpack(pack(np.concatenate([np.stack(np.meshgrid(a, b), -1).reshape(-1, 2), np.stack(np.meshgrid(b, a), -1).reshape(-1, 2)])))


def p_stripes(period=8, n=3, half_len=20):
    """2 n + 1 stripes along y, `period` cells apart."""
    return np.stack(np.meshgrid(np.arange(-n, n + 1) * period, np.arange(-half_len, half_len + 1)), -1).reshape(-1, 2)


def p_block(w, h, extra=0, at=(-32, -32)):
    """A dense block of w x h cells and `extra` more cells in the next row."""
    b = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2)
    e = np.stack([np.arange(extra), np.full(extra, h)], 1)
    return np.concatenate([b, e]) + np.asarray(at)


def p_spaced(n, seed, reach=40, gap=3):
    """n cells, any two at least `gap` cells apart on some axis: no cell inside another's dilation."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = rng.integers(-reach, reach + 1, 2)
        if all(max(abs(c[0] - o[0]), abs(c[1] - o[1])) >= gap for o in out):
            out.append((int(c[0]), int(c[1])))
    return np.asarray(out, np.int64)


BORDER = (0, 31, 32, 255, 256, 511)
FAR = np.asarray((37, -21))


def p_border(seed):
    """Cells on columns and rows 0, 31, 32, 255, 256 and 511: every crossing, and a few cells along each line."""
    rng = np.random.default_rng(seed)
    b = np.asarray(BORDER)
    cross = np.stack(np.meshgrid(b, b), -1).reshape(-1, 2)
    along = np.stack([np.repeat(b, 6), rng.integers(0, G, 36)], 1)
    return np.concatenate([cross, along, along[:, ::-1]]) - HALF


def rot90(duv, cell_px, turns=1):
    """A pattern turned by quarter turns about the sensor (the centre of voxel 0): the cell that holds the turned cell centre,
    with pixel ix covering [ix - 1/2, ix + 1/2).  In half pixels the centre of cell d is 2 d cell_px + cell_px - 1."""
    d = np.asarray(duv, np.int64).reshape(-1, 2)
    for _ in range(turns % 4):
        c2 = 2 * d * cell_px + cell_px - 1                    # centres, in half pixels
        r2 = np.stack([-c2[:, 1], c2[:, 0]], 1)               # (x, y) -> (-y, x)
        d = np.floor_divide(r2 + 1, 2 * cell_px)              # the cell of real coordinate r: floor((r + 1/2) / cell_px)
    return d


# ---- grid cases -----------------------------------------------------------------------------------------------------------

def _case(cell_px, img, ox, oy, res, want=None):
    """want: the cells the builder meant to occupy (None where the image is not made from a pattern)."""
    return dict(cell_px=cell_px, img=img, ox=ox, oy=oy, res=res, want=want)


def _pattern_case(duv, cell_px, seed):
    return _case(cell_px, *image_of(duv, cell_px, seed), want=pack(duv))


def _oversize(cell_px, seed):
    """An image larger than the grid on every side: occupied pixels all over it, those outside the 512 cells are dropped."""
    rng = np.random.default_rng(seed)
    side = G * cell_px
    w, h = side + 90, side + 50
    img = np.full((h, w), 255, np.uint8)
    img[rng.integers(0, h, 900), rng.integers(0, w, 900)] = 0
    img[0, 0] = img[h - 1, w - 1] = img[25, 45] = img[25 + side - 1, 45 + side - 1] = 0     # corners: outside, outside, cell (0, 0), cell (511, 511)
    res = RESOLUTION[cell_px]
    return _case(cell_px, img, _origin(-side // 2 - 45, res), _origin(-side // 2 - 25, res), res)


def _half_origin(cell_px, sign, seed):
    """ox / res = sign * 0.5 and oy / res = -sign * 0.5 exactly: lround takes them to +-1, not to 0."""
    rng = np.random.default_rng(seed)
    res = RESOLUTION[cell_px]
    img = np.where(rng.random((4 * cell_px + 3, 5 * cell_px + 2)) < 0.3, 0, 255).astype(np.uint8)
    half = float(np.float32(res) * np.float32(0.5))            # exact: a power of two
    return _case(cell_px, img, sign * half, -sign * half, res)


def _threshold(cell_px, seed):
    """Pixel values either side of the threshold: below 100 is occupied."""
    rng = np.random.default_rng(seed)
    img = rng.choice(np.asarray([0, 1, 98, 99, 100, 101, 254, 255], np.uint8), (9 * cell_px, 11 * cell_px))
    res = RESOLUTION[cell_px]
    return _case(cell_px, img, _origin(-5 * cell_px - 1, res), _origin(-4 * cell_px - 1, res), res)


def _negative(cell_px, seed):
    """Every pixel index from -3 cell_px - 1 to 2 cell_px, half of the pixels occupied: floor division below zero."""
    rng = np.random.default_rng(seed)
    n = 5 * cell_px + 2
    img = np.where(rng.random((n, n)) < 0.5, 0, 255).astype(np.uint8)
    img[:, ::cell_px] = 255                                      # leave some cells empty, so that a wrong bin shows
    res = RESOLUTION[cell_px]
    return _case(cell_px, img, _origin(-3 * cell_px - 1, res), _origin(-3 * cell_px - 1, res), res)


def _builders():
    out = {}
    for i, cp in enumerate(CELL_PX):
        s = 100 * (i + 1)
        out["random:%d" % cp] = functools.partial(_pattern_case, p_random(s + 1), cp, s + 1)
        out["random2:%d" % cp] = functools.partial(_pattern_case, p_random(s + 2, n=250, reach=45), cp, s + 2)
        out["lshape:%d" % cp] = functools.partial(_pattern_case, p_lshape(), cp, s + 3)
        out["square:%d" % cp] = functools.partial(_pattern_case, p_square(), cp, s + 4)
        out["plus:%d" % cp] = functools.partial(_pattern_case, p_plus(), cp, s + 5)
        out["stripes:%d" % cp] = functools.partial(_pattern_case, p_stripes(), cp, s + 6)
        # the same shapes out of the identity's reach (it is verified within `refine` cells of no shift): the answer then comes from
        # the rotation candidates, where a quarter-turn symmetry ties four rotations and a period ties the lags
        out["square_far:%d" % cp] = functools.partial(_pattern_case, p_square() + FAR, cp, s + 11)
        out["plus_far:%d" % cp] = functools.partial(_pattern_case, p_plus() + FAR, cp, s + 12)
        out["stripes_far:%d" % cp] = functools.partial(_pattern_case, p_stripes(n=5) + FAR, cp, s + 13)
        out["one:%d" % cp] = functools.partial(_pattern_case, [(3, -2)], cp, s + 7)
        out["empty:%d" % cp] = functools.partial(_pattern_case, np.zeros((0, 2), np.int64), cp, s + 8)
        out["n15:%d" % cp] = functools.partial(_pattern_case, p_spaced(16, s + 9)[:15], cp, s + 9)
        out["n16:%d" % cp] = functools.partial(_pattern_case, p_spaced(16, s + 9), cp, s + 9)
        out["dense:%d" % cp] = functools.partial(_pattern_case, p_block(70, 60, at=(-30, -28)), cp, s + 10)    # 4200 cells
    for cp in (1, 3):
        out["border:%d" % cp] = functools.partial(_pattern_case, p_border(50 + cp), cp, 50 + cp)
        out["half_plus:%d" % cp] = functools.partial(_half_origin, cp, +1, 60 + cp)
        out["half_minus:%d" % cp] = functools.partial(_half_origin, cp, -1, 70 + cp)
    for cp in (1, 2):
        out["oversize:%d" % cp] = functools.partial(_oversize, cp, 80 + cp)
    for cp in (2, 3):
        out["threshold:%d" % cp] = functools.partial(_threshold, cp, 90 + cp)
    for cp in (2, 3, 16):
        out["negative:%d" % cp] = functools.partial(_negative, cp, 95 + cp)
    # the cell list's size classes step by 4096 cells: dense blocks at cell_px = 1
    out["cells4096:1"] = functools.partial(_pattern_case, p_block(64, 64), 1, 11)
    out["cells4097:1"] = functools.partial(_pattern_case, p_block(64, 64, extra=1), 1, 12)
    out["cells10000:1"] = functools.partial(_pattern_case, p_block(100, 100, at=(-50, -47)), 1, 13)
    return out


GRID_CASES = _builders()
SYMMETRIC = ("square", "plus", "stripes")
SYMMETRIC_FAR = ("square_far", "plus_far", "stripes_far")


def names_of(cell_px):
    return [n for n in GRID_CASES if n.endswith(":%d" % cell_px)]


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """dict(cell_px, img, ox, oy, res, want).  Cached: nobody writes to it."""
    c = GRID_CASES[name]()
    c["img"].setflags(write=False)
    return c


def case_of_pattern(duv, cell_px, seed):
    """A grid case made on the spot (the probes, the pairs below)."""
    return _pattern_case(duv, cell_px, seed)


def probe_patterns(cells):
    """(probe, halo) cell offsets of a grid's cells: every cell within one cell of an occupied one, clipped to the grid -- each
    lies on the dilated map -- and every cell exactly two cells away -- none does."""
    occ = np.zeros((G, G), bool)
    c = np.asarray(cells, np.uint32)
    occ[(c >> 16).astype(np.int64), (c & 0xFFFF).astype(np.int64)] = True
    one = dilate(occ)
    two = dilate(one) & ~one
    f = lambda m: np.stack(np.nonzero(m)[::-1], 1).astype(np.int64) - HALF
    return f(one), f(two)


PROBE_PARAMS = dict(n_yaw=1, max_shift=0, top_yaw=0, refine=0, min_overlap=0.25)

# ---- pairs ----------------------------------------------------------------------------------------------------------------

# matched under every row of PARAM_ROWS, as "<stem>:<cell_px>": random against random, a known-answer pair (the L turned by a
# quarter turn and shifted by (3, -2) cells), a symmetric pair, sparse against dense
SWEEP_PAIRS = (("random", "random2"), ("lshape", "lshape_turned"), ("plus", "plus_far"), ("random2", "dense"))
SWEEP_SHIFT = (3, -2)
for _cp in CELL_PX:
    GRID_CASES["lshape_turned:%d" % _cp] = functools.partial(_pattern_case, rot90(p_lshape(), _cp) + np.asarray(SWEEP_SHIFT), _cp, 40 + _cp)

# Known answers.  (max_shift, top_yaw, refine) of each and the truth it allows: with top_yaw = 0 only the identity is verified, so
# the truth is no rotation and a shift inside the refine window; with max_shift = 0 the lags are zero and the shift is zero.
KNOWN_SEARCH = ((64, 12, 4, (17, -9)), (0, 1, 0, (0, 0)), (255, 64, 8, (100, -70)), (5, 0, 2, (2, -1)))
KNOWN_N_YAW = (1, 4, 7, 8, 360, 3600)


def known_pattern():
    """About 300 cells with no symmetry: the L with its bar and a sparse random field."""
    return unpack(pack(np.concatenate([p_lshape()[::2], p_random(7, n=120, reach=50)])))


def known_cases():
    """[(id, cell_px, params, turns, shift)]: every cell_px, n_yaw and search of the table, except that n_yaw = 3600 is matched with the
    cheap searches only (at max_shift = 255 it costs the restatement more than a second a pair)."""
    out = []
    for cp in CELL_PX:
        for n_yaw in KNOWN_N_YAW:
            for max_shift, top_yaw, refine, shift in KNOWN_SEARCH:
                if n_yaw == 3600 and max_shift > 5:
                    continue
                top = min(top_yaw, n_yaw)
                turns = 1 if (n_yaw % 4 == 0 and top >= 1) else 0
                prm = dict(n_yaw=n_yaw, max_shift=max_shift, top_yaw=top, refine=refine, min_overlap=0.25)
                out.append(("px%d-yaw%d-shift%d-top%d-ref%d" % (cp, n_yaw, max_shift, top, refine), cp, prm, turns, shift))
    return out


def known_pair(cell_px, turns, shift):
    """(query case, database case): the database is the query turned and shifted."""
    q = known_pattern()
    return case_of_pattern(q, cell_px, 21), case_of_pattern(rot90(q, cell_px, turns) + np.asarray(shift), cell_px, 22)


# The 1.2 x rule.  P1 lies along +x just above the axis, P2 in the (-x, +y) quadrant away from both axes; the database holds P1 and
# the quarter turn of P2.  Matched with four rotations and no shift: the identity overlaps P1 only, rotation 1 overlaps P2 only,
# rotations 2 and 3 nothing (every turned set lands in a quadrant strip of its own).
RULE_PARAMS = dict(n_yaw=4, max_shift=0, top_yaw=4, refine=0, min_overlap=0.25)
RULE_P1 = np.asarray([(12 + 7 * i, 4 + (i * i) % 11) for i in range(10)], np.int64)


def rule_p2(n):
    return np.asarray([(-20 - 5 * j, 22 + 3 * ((j * j) % 7) + (j % 2)) for j in range(n)], np.int64)


def rule_pair(n, cell_px=2):
    """(query case, database case) with |P1| = 10 and |P2| = n: 5 n > 6 * 10 decides."""
    p2 = rule_p2(n)
    return (case_of_pattern(np.concatenate([RULE_P1, p2]), cell_px, 31),
            case_of_pattern(np.concatenate([RULE_P1, rot90(p2, cell_px)]), cell_px, 32))


# The acceptance edges.  Matched with one rotation, no lag and one shift, so the overlap is the number of query cells on the
# dilated database map.  The shared cells are within 5 cells of the sensor: no scale factor of 0.88 .. 1.12 moves one of them by a
# cell, every factor overlaps alike and the scale comes back as exactly 1.
EDGE_PARAMS = dict(n_yaw=1, max_shift=0, top_yaw=0, refine=0, min_overlap=0.25)
EDGE_SHARED = np.asarray([(2, 1), (-3, 2), (1, -4), (-2, -3)], np.int64)
EDGE_REST = np.asarray([(20 + 4 * i, -30 + 5 * i) for i in range(12)], np.int64)      # in the query only
EDGE_ELSE = np.asarray([(-40, 40), (-44, 35), (-30, 44)], np.int64)                   # in the database only
# name -> (query cells, shared cells in the database, overlap, ok)
EDGE_PAIRS = {
    "q16_overlap4": (16, 4, 4, True),        # 4 >= 0.25 * 16
    "q16_overlap3": (16, 3, 3, False),
    "q15_overlap4": (15, 4, 4, False),       # 4 >= 0.25 * 15, but fewer than 16 query cells are never accepted
    "q15_overlap3": (15, 3, 3, False),
}


def edge_pair(name, cell_px=2):
    nq, shared, _, _ = EDGE_PAIRS[name]
    q = np.concatenate([EDGE_SHARED, EDGE_REST[:nq - 4]])
    d = np.concatenate([EDGE_SHARED[:shared], EDGE_ELSE])
    return case_of_pattern(q, cell_px, 33), case_of_pattern(d, cell_px, 34)


# The stretched query: the database is a filled disc of 25 cells about the sensor, the query 300 of its cells with every offset
# multiplied by 1.3.  The database is the query scaled by 1 / 1.3, below the smallest factor 0.88; the smaller the factor, the more of
# the query falls on the disc (its dilation reaches 26 cells, the query 32.5 f: 83 % at 0.88, 76 % at 0.92), so the estimate lands on
# that end of the range and ok is withdrawn although min_overlap = 0 asks for nothing.
STRETCH_PARAMS = dict(n_yaw=360, max_shift=64, top_yaw=12, refine=4, min_overlap=0.0)


def stretch_pattern(radius=25):
    a = np.arange(-radius, radius + 1)
    d = np.stack(np.meshgrid(a, a), -1).reshape(-1, 2)
    return d[(d ** 2).sum(1) <= radius * radius]


def stretch_pair(factor=1.3, cell_px=2):
    """(query case, database case); factor = 1 gives the unstretched query, which is accepted."""
    disc = stretch_pattern()
    part = disc[np.random.default_rng(37).permutation(len(disc))[:300]]
    q = np.rint(part * factor).astype(np.int64)
    return case_of_pattern(unpack(pack(q)), cell_px, 35), case_of_pattern(disc, cell_px, 36)
