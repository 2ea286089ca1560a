"""The scan index of scan_store.hip in plain numpy: header and key grid, the Hilbert keys (and their inverse), the
curve order, the launch orders, and the judgements of the boxes of all three levels.  float32 where the kernel's value
is stored (header, keys, group extents), float64 where a property of stored numbers is judged (containment, tightness).
Everything is vectorised: a 270 k-point scan takes a fraction of a second.  Not a test module and not GPU code; the
statement has its own proof in test_scan_index_ref_cpu.py."""
import numpy as np

CH, SB, SUP = 128, 16, 64          # points per chunk, per sub-block; chunks per super-chunk
RANGE = 64.0                       # boxes are kept as (centre, -half extent / RANGE)
NN_FAR = np.float32(1.0e18)        # coordinate of the padding points
EMPTY_NH = np.float32(1.0e30)      # stored "half extent" of an empty sub-block (its centre is 0)


def f2ord(x):
    """Order-preserving map float32 -> uint32 (scan_index.hpp)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def ord2f(v):
    v = np.ascontiguousarray(v, np.uint32)
    u = np.where(v & 0x80000000, v & 0x7FFFFFFF, ~v).astype(np.uint32)
    return u.view(np.float32)


def sizes(n):
    """Counts of the layout of an n-point scan: chunks, padded points, sub-block pairs, super-chunks."""
    nch = (n + CH - 1) // CH
    n_pad = max(nch, 1) * CH
    return dict(nch=nch, n_pad=n_pad, npairs=n_pad // (2 * SB), nsup=(nch + SUP - 1) // SUP)


# ---- header ------------------------------------------------------------------------------------------------------------
def header(xyz, finite_only=False):
    """lo / hi: min and max of f2ord per axis; ox, oy, oz: the minima; inv_cell = 1 / max(0.25, ext / 1023), all float32.
    An empty scan: lo = 0xFFFFFFFF, hi = 0, grid (0, 0, 0, 4).  finite_only: a non-finite coordinate takes no part (an
    axis without any finite coordinate keeps the empty lo / hi and counts as origin 0, extent 0)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    lo = np.full(3, 0xFFFFFFFF, np.uint32)
    hi = np.zeros(3, np.uint32)
    if len(xyz) == 0:
        return dict(lo=lo, hi=hi, ox=np.float32(0), oy=np.float32(0), oz=np.float32(0), inv_cell=np.float32(4))
    o = f2ord(xyz)
    for a in range(3):
        oa = o[np.isfinite(xyz[:, a]), a] if finite_only else o[:, a]
        if len(oa):
            lo[a], hi[a] = oa.min(), oa.max()
    some = lo <= hi
    mn = np.where(some, ord2f(np.where(some, lo, 0x80000000)), np.float32(0)).astype(np.float32)
    mx = np.where(some, ord2f(np.where(some, hi, 0x80000000)), np.float32(0)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (mx - mn).astype(np.float32)
        ext = np.fmax(np.fmax(e[0], e[1]), e[2])                          # fmaxf: a NaN operand is dropped
        cell = np.fmax(np.float32(0.25), np.float32(ext / np.float32(1023.0)))
        inv = np.float32(np.float32(1.0) / cell)
    return dict(lo=lo, hi=hi, ox=mn[0], oy=mn[1], oz=mn[2], inv_cell=inv)


# ---- Hilbert keys: Skilling's transpose form, 10 bits per axis (math3.hpp::morton_key) ----------------------------------
BITS = 10


def _spread10(v):
    v = v & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def _compact10(v):
    v = v & np.uint32(0x09249249)
    v = (v | (v >> np.uint32(2))) & np.uint32(0x030C30C3)
    v = (v | (v >> np.uint32(4))) & np.uint32(0x0300F00F)
    v = (v | (v >> np.uint32(8))) & np.uint32(0x030000FF)
    v = (v | (v >> np.uint32(16))) & np.uint32(0x3FF)
    return v


def hilbert_encode(cells):
    """cells [n, 3] integers in [0, 1024) -> keys [n] uint32 < 2^30; axis 0 holds the most significant bit of each triple."""
    X = [np.array(cells[:, a], np.uint32) for a in range(3)]
    M = 1 << (BITS - 1)
    Q = M
    while Q > 1:
        P = np.uint32(Q - 1)
        for i in range(3):
            hit = (X[i] & np.uint32(Q)) != 0
            t = np.where(hit, np.uint32(0), (X[0] ^ X[i]) & P)
            X[0] = np.where(hit, X[0] ^ P, X[0] ^ t)
            if i:
                X[i] = X[i] ^ t
        Q >>= 1
    X[1] = X[1] ^ X[0]
    X[2] = X[2] ^ X[1]
    t = np.zeros_like(X[0])
    Q = M
    while Q > 1:
        t = np.where((X[2] & np.uint32(Q)) != 0, t ^ np.uint32(Q - 1), t)
        Q >>= 1
    X = [x ^ t for x in X]
    return (_spread10(X[0]) << np.uint32(2)) | (_spread10(X[1]) << np.uint32(1)) | _spread10(X[2])


def hilbert_decode(keys):
    """The inverse of hilbert_encode: keys [n] -> cells [n, 3] (Skilling's TransposetoAxes)."""
    k = np.asarray(keys, np.uint32)
    X = [_compact10(k >> np.uint32(2)), _compact10(k >> np.uint32(1)), _compact10(k)]
    t = X[2] >> np.uint32(1)
    X[2] = X[2] ^ X[1]
    X[1] = X[1] ^ X[0]
    X[0] = X[0] ^ t
    Q = 2
    while Q != (1 << BITS):
        P = np.uint32(Q - 1)
        for i in (2, 1, 0):
            hit = (X[i] & np.uint32(Q)) != 0
            t = np.where(hit, np.uint32(0), (X[0] ^ X[i]) & P)
            X[0] = np.where(hit, X[0] ^ P, X[0] ^ t)
            if i:
                X[i] = X[i] ^ t
        Q <<= 1
    return np.stack(X, 1).astype(np.int64)


def grid_cells(xyz, ox, oy, oz, inv_cell):
    """(uint32) fminf(fmaxf((x - o) * inv_cell, 0), 1023) per axis in float32, un-fused; fmaxf turns a NaN into 0."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    o = np.array([ox, oy, oz], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = ((xyz - o).astype(np.float32) * np.float32(inv_cell)).astype(np.float32)
        f = np.fmin(np.fmax(f, np.float32(0)), np.float32(1023))
    return f.astype(np.uint32)


def hilbert_key(xyz, ox, oy, oz, inv_cell):
    return hilbert_encode(grid_cells(xyz, ox, oy, oz, inv_cell))


def curve_order(xyz):
    """The whole statement of a scan's curve order: (perm, sorted keys), perm[s] = original index at sorted position s."""
    h = header(xyz)
    k = hilbert_key(xyz, h["ox"], h["oy"], h["oz"], h["inv_cell"])
    perm = np.argsort(k, kind="stable")
    return perm, k[perm]


# ---- boxes ---------------------------------------------------------------------------------------------------------------
def block_minmax(pts_sorted, size, nblocks=None):
    """Per block of `size` consecutive points and per axis the min and max of the FINITE coordinates, float64 [nb, 3]
    each; an axis of a block without any finite coordinate (or a block past the end) has mn = +inf > mx = -inf."""
    p = np.asarray(pts_sorted, np.float64).reshape(-1, 3)
    n = len(p)
    nb = (n + size - 1) // size if nblocks is None else nblocks
    full = np.full((nb * size, 3), np.nan)
    full[:n] = p
    full = full.reshape(nb, size, 3)
    fin = np.isfinite(full)
    return np.where(fin, full, np.inf).min(1), np.where(fin, full, -np.inf).max(1)


def box_interval(c, nh):
    """Stored (centre, -half extent / 64) -> (c, h, lo, hi) in float64."""
    c = np.asarray(c, np.float64)
    h = -np.asarray(nh, np.float64) * RANGE
    return c, h, c - h, c + h


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def boxes_contain(c, nh, mn, mx):
    """Every finite coordinate the box stands for lies inside [c - h, c + h]: exact, no tolerance.  [nb, 3] bool."""
    some = mn <= mx
    with np.errstate(invalid="ignore"):                  # (an infinite centre and half extent: NaN corners contain nothing)
        _, _, lo, hi = box_interval(c, nh)
        return ~some | ((lo <= mn) & (mx <= hi))


def boxes_tight(c, nh, mn, mx):
    """h <= H (1 + 1e-6) + ulp32(max(|mn|, |mx|)) + 1e-30, H the exact half extent.  The kernel computes
    max(c - mn, mx - c) * 1.0000005 + 1e-30 in fp32 with c = fl(0.5 mn + 0.5 mx): the centre is off by at most one
    rounding (an ulp of the larger corner, which the larger of the two differences inherits), each difference and the
    product round by 2^-24 relative (together with 5e-7 below 1e-6), and the constant is the kernel's own."""
    _, h, _, _ = box_interval(c, nh)
    some = mn <= mx
    with np.errstate(invalid="ignore"):
        H = 0.5 * (mx - mn)
        bound = H * (1 + 1e-6) + ulp32(np.maximum(np.abs(mn), np.abs(mx))) + 1e-30
        return ~some | (h <= bound)


def unpack_sb2(sb2):
    """The interleaved pairs [npairs, 3, 4] -> centres and negated scaled half extents per sub-block, [2 * npairs, 3]."""
    f = np.asarray(sb2, np.float32).reshape(-1, 12)
    c = np.empty((len(f), 2, 3), np.float32)
    nh = np.empty((len(f), 2, 3), np.float32)
    for h in range(2):
        c[:, h, 0], c[:, h, 1], c[:, h, 2] = f[:, 0 + h], f[:, 2 + h], f[:, 4 + h]
        nh[:, h, 0], nh[:, h, 1], nh[:, h, 2] = f[:, 6 + h], f[:, 8 + h], f[:, 10 + h]
    return c.reshape(-1, 3), nh.reshape(-1, 3)


def super_contain_chunks(sup_lo, sup_hi, c, nh):
    """Super box s contains the stored interval of every chunk box 64 s .. 64 s + 63 that exists.  [nch, 3] bool."""
    _, _, lo, hi = box_interval(c, nh)
    s = np.arange(len(lo)) // SUP
    return (np.asarray(sup_lo, np.float64)[s, :3] <= lo) & (hi <= np.asarray(sup_hi, np.float64)[s, :3])


def super_tight(sup_lo, sup_hi, c, nh):
    """A super box exceeds the union of its chunk intervals by at most 4e-7 (|c| + h) per side plus an fp32 ulp of the
    corner (the kernel: slack 2e-7 (|c| + h), the corner and the subtraction of the slack rounded once each): the
    extreme over the chunks of (corner -/+ that allowance) bounds the stored corner.  [nsup, 3] bool."""
    c, h, lo, hi = box_interval(c, nh)
    allow_lo = 4e-7 * (np.abs(c) + h) + ulp32(lo)
    allow_hi = 4e-7 * (np.abs(c) + h) + ulp32(hi)
    nsup = (len(c) + SUP - 1) // SUP
    starts = np.arange(nsup) * SUP
    floor = np.minimum.reduceat(lo - allow_lo, starts, axis=0)
    ceil = np.maximum.reduceat(hi + allow_hi, starts, axis=0)
    return (np.asarray(sup_lo, np.float64)[:, :3] >= floor) & (np.asarray(sup_hi, np.float64)[:, :3] <= ceil)


def padding_ok(pad):
    """pts[n : n_pad]: each (1e18, 1e18, 1e18) with index bits 0xFFFFFFFF."""
    pad = np.ascontiguousarray(pad, np.float32).reshape(-1, 4)
    return bool((pad[:, :3] == NN_FAR).all() and (pad[:, 3].view(np.uint32) == 0xFFFFFFFF).all())


# ---- launch order ----------------------------------------------------------------------------------------------------------
def group_extent_keys(points_sorted, group):
    """~f2ord((dx dx + dy dy) + dz dz) in float32 per group of `group` consecutive sorted points (d: the extent of the
    group's bounding box): ascending keys = widest first."""
    p = np.ascontiguousarray(points_sorted, np.float32).reshape(-1, 3)
    n = len(p)
    ng = (n + group - 1) // group
    full = np.full((ng * group, 3), np.nan, np.float32)
    full[:n] = p
    full = full.reshape(ng, group, 3)
    d = (np.nanmax(full, 1) - np.nanmin(full, 1)).astype(np.float32)
    e = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32) + d[:, 2] * d[:, 2]).astype(np.float32)
    return ~f2ord(e)


def launch_order(points_sorted, group):
    """The launch order of the source groups: stable argsort of the extent keys (equal extents in ascending group id)."""
    return np.argsort(group_extent_keys(points_sorted, group), kind="stable").astype(np.uint32)


# ---- kd order ----------------------------------------------------------------------------------------------------------------
def kd_order_numpy(pts_curve):
    """scan_index.hpp's rule on points given in curve order: P = 16 * 2^L >= n positions, at every level every
    aligned node is sorted (stable) along the widest axis of its bounding box.  Returns the kd position -> curve
    position table."""
    n = len(pts_curve)
    L = 0
    while (16 << L) < n:
        L += 1
    cur = np.arange(n)
    for l in range(L):
        shift = 4 + L - l
        p = pts_curve[cur]
        node = np.arange(n) >> shift
        o = np.stack([f2ord(p[:, a]) for a in range(3)], 1)
        lo = np.full((1 << l, 3), 0xFFFFFFFF, np.uint32)
        hi = np.zeros((1 << l, 3), np.uint32)
        np.minimum.at(lo, node, o)
        np.maximum.at(hi, node, o)
        ext = ord2f(hi) - ord2f(lo)                      # fp32, as the kernel
        axis = np.zeros(1 << l, np.int64)
        e = ext[:, 0].copy()
        m = ext[:, 1] > e
        axis[m] = 1
        e[m] = ext[m, 1]
        axis[ext[:, 2] > e] = 2
        key = (node.astype(np.uint64) << np.uint64(32)) | o[np.arange(n), axis[node]].astype(np.uint64)
        cur = cur[np.argsort(key, kind="stable")]
    return cur


# ---- the inputs of the GPU tests (checked by test_scan_index_ref_cpu.py) ---------------------------------------------------
EDGE_SIZES = dict(
    subblocks_and_pairs=[1, 2, 15, 16, 17, 31, 32, 33],
    groups_and_chunks=[63, 64, 65, 127, 128, 129, 255, 256, 257],
    sort_tiles=[2047, 2048, 2049, 4097],
    super_boxes=[8191, 8192, 8193],
    tile_blocks=[131071, 131072, 131073],
)
SORT_TILE = 2048                   # keys per tile of the segmented radix sort (seg_sort.hpp)
SMALL_MAX = 4096                   # groups the in-LDS sort of the launch orders takes
GROUP_SIZES = [(63, 15), (64, 16), (65, 17), (127, 33), (128, 128), (129, 129), (255, 8191), (256, 8192), (257, 8193)]


def uniform_cloud(n, seed, side=40.0):
    return np.random.default_rng(seed).uniform(-side / 2, side / 2, (n, 3)).astype(np.float32)


def edge_clouds():
    """The batch of 4a: uniform clouds in a 40 m cube at every size of EDGE_SIZES, an empty scan between two of them."""
    out = []
    for k, ns in enumerate(EDGE_SIZES.values()):
        for n in ns:
            out.append(uniform_cloud(n, 1000 * k + n % 997))
    out.insert(5, np.zeros((0, 3), np.float32))
    return out


def tie_cloud():
    """128 distinct points, each 2048 times (the same 128-point block over and over), among 4000 single points: in curve
    order the copies of a point stand together, so every run holds whole groups of 64, 128 and 256 identical points --
    extent exactly 0 -- between groups of every other extent.  266 144 points: 4159 groups at one source per lane."""
    rng = np.random.default_rng(77)
    base = rng.uniform(-20, 20, (128, 3)).astype(np.float32)
    return np.concatenate([np.tile(base, (2048, 1)), rng.uniform(-20, 20, (4000, 3)).astype(np.float32)])


# Centre of the far cluster of (iv) and (v): 1000 m BELOW the rest along y, the axis on which one of its points is +inf --
# a box whose upper corner is infinite keeps the cluster only if its lower corner survives the infinity.
FAR = np.array([3.0, -1000.0, -2.0], np.float32)
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]


def nonfinite_clouds():
    """The scans of 4d, as (name, cloud): (i) - (iii) 100 points in a 10 m cube with one non-finite coordinate in point 37;
    (iv) 300 and (v) 20 000 points with six points 1000 m away at positions 10 .. 15, one of them with an infinite y."""
    rng = np.random.default_rng(4242)
    base = rng.uniform(-5, 5, (100, 3)).astype(np.float32)
    out = []
    for name, axis, v in (("i", 0, np.float32(np.inf)), ("ii", 2, np.float32(-np.inf)), ("iii", 1, NEG_NAN)):
        c = base.copy()
        c.view(np.uint32)[37, axis] = np.array([v], np.float32).view(np.uint32)[0]     # (the bits: a NaN keeps its sign)
        out.append((name, c))
    for name, n, side in (("iv", 300, 10.0), ("v", 20000, 40.0)):
        c = rng.uniform(-side / 2, side / 2, (n, 3)).astype(np.float32)
        c[10:16] = FAR + rng.uniform(-1, 1, (6, 3)).astype(np.float32)
        c[12, 1] = np.float32(np.inf)
        out.append((name, c))
    return out
