"""CPU: the numpy statement of the scan index (scan_index_ref.py) proves itself -- the Hilbert keys are a bijection of the
1024^3 grid whose consecutive keys are neighbouring cells -- and the inputs of the GPU tests are what they are said to
be: the size lists contain the boundaries they name, the tie cloud has its ties, the far clusters are far."""
import numpy as np

import scan_index_ref as ref


def test_hilbert_decode_inverts_encode():
    rng = np.random.default_rng(1)
    cells = rng.integers(0, 1024, (100_000, 3))
    keys = ref.hilbert_encode(cells)
    assert keys.dtype == np.uint32 and keys.max() < (1 << 30)
    assert (ref.hilbert_decode(keys) == cells).all()
    k = rng.integers(0, 1 << 30, 100_000).astype(np.uint32)
    assert (ref.hilbert_encode(ref.hilbert_decode(k)) == k).all()


def test_consecutive_keys_are_neighbouring_cells():
    rng = np.random.default_rng(2)
    k = rng.integers(0, (1 << 30) - 1, 100_000).astype(np.uint32)
    k[:4] = [0, 1, (1 << 30) - 2, (1 << 29) - 1]                 # the ends and the middle of the curve
    d = np.abs(ref.hilbert_decode(k + np.uint32(1)) - ref.hilbert_decode(k))
    assert (d.sum(1) == 1).all() and (d.max(1) == 1).all()       # exactly 1 in exactly one axis


def test_keys_worked_by_hand():
    """With M = 512: (0, 0, 0) passes every step unchanged -> 0.  (1023, 0, 0): the first step (Q = 512) inverts the low
    bits of X0 -> (512, 0, 0), nothing else applies; Gray -> (512, 512, 512), t = 511 -> (1023, 1023, 1023): every bit
    set, the last key.  (0, 0, 1023): at every Q the set bit of X2 inverts X0's low bits (and at Q < 512 X0's own set
    bit inverts them back first): X = (511, 0, 1023); Gray -> (511, 511, 512), t = 511 -> (0, 0, 1023): every third bit
    from bit 0.  (0, 0, 1): every Q exchanges the low bits of X0 and X1, then of X0 and X2 where they differ: (0, 0, 1) ->
    (1, 0, 0) -> (0, 1, 0) -> (0, 0, 1), a cycle of three, run through three times by the nine steps; Gray -> (0, 0, 1),
    t = 0: key 1, the first step of the curve."""
    hand = {(0, 0, 0): 0, (1023, 0, 0): (1 << 30) - 1, (0, 0, 1023): 0x09249249, (0, 0, 1): 1}
    cells = np.array(list(hand), np.int64)
    assert (ref.hilbert_encode(cells) == np.array(list(hand.values()), np.uint32)).all()
    # the curve starts and ends in corners of the grid that share an edge of the cube
    assert (ref.hilbert_decode(np.array([0, (1 << 30) - 1], np.uint32)) == [[0, 0, 0], [1023, 0, 0]]).all()


def test_f2ord_orders_and_inverts():
    x = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    o = ref.f2ord(x)
    assert (np.diff(o.astype(np.int64)) > 0).all() and (ref.ord2f(o).view(np.uint32) == x.view(np.uint32)).all()
    assert ref.f2ord(ref.NEG_NAN) < o[0] and ref.f2ord(np.float32(np.nan)) > o[-1]   # a sign-bit-set NaN orders lowest


def test_header_statement():
    h = ref.header(np.zeros((0, 3), np.float32))
    assert (h["ox"], h["oy"], h["oz"], h["inv_cell"]) == (0, 0, 0, 4) and (h["lo"] > h["hi"]).all()
    c = np.array([[0, 0, 0], [1023, 1, 2]], np.float32)
    h = ref.header(c)
    assert h["inv_cell"] == 1 and (ref.grid_cells(c, h["ox"], h["oy"], h["oz"], h["inv_cell"]) == c).all()
    assert ref.header(np.ones((5, 3), np.float32))["inv_cell"] == 4                   # the smallest cell is 0.25 m
    assert ref.header(ref.uniform_cloud(4099, 5))["inv_cell"] == 4                    # ... which a 40 m cube has,
    assert ref.header(ref.uniform_cloud(4099, 5, side=400.0))["inv_cell"] < 3         # a 400 m cube does not
    for name, cl in ref.nonfinite_clouds():
        h = ref.header(cl, finite_only=True)
        clean = np.where(np.isfinite(cl), cl, np.float32(0.5))                       # (inside the cube on every axis)
        g = ref.header(clean)
        assert all(h[k] == g[k] for k in ("ox", "oy", "oz", "inv_cell")) and np.isfinite(h["inv_cell"]), name


def test_box_judgements_on_boxes_made_here():
    """The judgements accept the kernel's arithmetic done in numpy float32 and refuse a box a hair too small or 1 % fat."""
    rng = np.random.default_rng(3)
    p = (rng.uniform(-40, 40, (1000, 3)) + [0, 500, -3000]).astype(np.float32)
    mn, mx = ref.block_minmax(p, 16)
    m32, x32 = mn.astype(np.float32), mx.astype(np.float32)
    c = (np.float32(0.5) * m32 + np.float32(0.5) * x32).astype(np.float32)
    he = (np.maximum(c - m32, x32 - c).astype(np.float32) * np.float32(1.0000005) + np.float32(1e-30)).astype(np.float32)
    nh = (-he * np.float32(1 / 64)).astype(np.float32)
    assert ref.boxes_contain(c, nh, mn, mx).all() and ref.boxes_tight(c, nh, mn, mx).all()
    assert not ref.boxes_tight(c, nh * np.float32(1.01), mn, mx).all()
    assert not ref.boxes_contain(c, nh * np.float32(0.9999), mn, mx).all()
    cc, hh = c.astype(np.float64), he.astype(np.float64)
    sl = (np.float32(2e-7) * (np.abs(c) + he)).astype(np.float32)
    lo = ((c - he).astype(np.float32) - sl).astype(np.float32)
    hi = ((c + he).astype(np.float32) + sl).astype(np.float32)
    st = np.arange(0, len(c), 64)
    ulo, uhi = np.minimum.reduceat(lo, st, axis=0), np.maximum.reduceat(hi, st, axis=0)
    assert ref.super_contain_chunks(ulo, uhi, c, nh).all() and ref.super_tight(ulo, uhi, c, nh).all()
    assert not ref.super_tight(ulo - np.float32(0.01), uhi, c, nh).all()
    lo0 = np.minimum.reduceat((cc - hh), st, axis=0)
    assert not ref.super_contain_chunks(np.nextafter(lo0.astype(np.float32), np.float32(np.inf)) + np.float32(1e-3), uhi, c, nh).all()


def test_size_lists_contain_the_boundaries_they_name():
    E = ref.EDGE_SIZES
    for b in (ref.SB, 2 * ref.SB):                                                   # a sub-block, a pair
        assert {b - 1, b, b + 1} <= set(E["subblocks_and_pairs"])
    for b in (64, 128, 256):                                                         # groups at cs = 1, 2, 4; 128: a chunk
        assert {b - 1, b, b + 1} <= set(E["groups_and_chunks"])
    assert ref.CH == 128
    assert {ref.SORT_TILE - 1, ref.SORT_TILE, ref.SORT_TILE + 1, 2 * ref.SORT_TILE + 1} <= set(E["sort_tiles"])
    b = ref.CH * ref.SUP
    assert {b - 1, b, b + 1} <= set(E["super_boxes"])
    assert [ref.sizes(n)["nsup"] for n in E["super_boxes"]] == [1, 1, 2]
    b = 64 * ref.SORT_TILE
    assert {b - 1, b, b + 1} <= set(E["tile_blocks"])
    assert [-(-n // ref.SORT_TILE) for n in E["tile_blocks"]] == [64, 64, 65]
    every = [n for ns in E.values() for n in ns]
    for L in (0, 1, 4, 9, 13):                                                       # kd trees of 16 * 2^L positions
        assert {(16 << L) - 1, (16 << L) + 1} <= set(every), L
    clouds = ref.edge_clouds()
    assert sorted(len(c) for c in clouds) == sorted(every + [0]) and 0 < [len(c) for c in clouds].index(0) < len(clouds) - 1
    assert any(len(c) % 4 for c in clouds) and max(len(c) for c in clouds) <= 270_000
    assert [ns for ns, _ in ref.GROUP_SIZES] == E["groups_and_chunks"]              # every source-group boundary once
    assert [nt for _, nt in ref.GROUP_SIZES] == [15, 16, 17, 33, 128, 129, 8191, 8192, 8193]
    for ns, nt in ref.GROUP_SIZES:
        assert ns in E["groups_and_chunks"] and nt in every


def test_group_counts_straddle_the_in_lds_sort():
    assert -(-262144 // 64) == ref.SMALL_MAX and -(-262145 // 64) == ref.SMALL_MAX + 1


def test_tie_cloud_has_its_ties():
    c = ref.tie_cloud()
    assert len(c) <= 270_000 and -(-len(c) // 64) > ref.SMALL_MAX >= -(-len(c) // 128)   # both sort paths
    perm, _ = ref.curve_order(c)
    p = c[perm]
    for cs in (1, 2, 4):
        k = ref.group_extent_keys(p, 64 * cs)
        vals, counts = np.unique(k, return_counts=True)
        assert counts.max() >= 50 and (counts == 1).sum() >= 50, cs                   # ties, and groups that are none
        o = ref.launch_order(p, 64 * cs)
        same = np.diff(k[o].astype(np.int64)) == 0
        assert (np.diff(k[o].astype(np.int64)) >= 0).all() and (np.diff(o.astype(np.int64))[same] > 0).all()


def test_far_clusters_are_far():
    for name, c in ref.nonfinite_clouds():
        bad = ~np.isfinite(c)
        assert bad.sum() == 1, name
        if name in ("iv", "v"):
            far = np.zeros(len(c), bool)
            far[10:16] = True
            assert bad[12, 1] and (far & ~bad.any(1)).sum() == 5
            rest = c[~far]
            lo, hi = rest.min(0).astype(np.float64), rest.max(0).astype(np.float64)
            q = c[far & ~bad.any(1)].astype(np.float64)
            gap = np.maximum(np.maximum(lo - q, q - hi), 0)                           # distance to the others' hull box
            assert (np.sqrt((gap ** 2).sum(1)) > 100).all(), name
            assert c[12, 1] == np.inf and (q[:, 1] < lo[1] - 100).all()              # below the others, on the infinite axis
        else:
            assert bad[37].sum() == 1 and len(c) == 100
    assert ref.nonfinite_clouds()[2][1].view(np.uint32)[37, 1] == 0xFFC00000
