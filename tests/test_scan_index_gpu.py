"""GPU: the scan index itself (scan_store.hip + seg_sort.hpp).  The registration tests cannot see a wrong ORDER --
the 1-NN search is exact whatever order the points are in, a bad sort only makes it slow -- so the orders are
checked here directly: the curve order (hand-written segmented radix sort: sorted, a permutation, stable), the
launch order of the source groups (widest first), the kd order of a target index against a numpy statement of
the same rule, and a batch of scans against the same scans added one at a time.  Everything else the culled search
trusts -- the header's key grid, the keys themselves, the boxes of all three levels, the padding, the launch orders for
1, 2 and 4 sources per lane -- is checked against scan_index_ref.py, the index in plain numpy: a box that is too large
or a wrong key only makes the search slow, a box that is too small loses neighbours on the clouds where it matters."""
import numpy as np
import pytest

import scan_index_ref as ref
from scan_index_ref import kd_order_numpy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clouds():
    from gloc3d_amd import synth
    rng = np.random.default_rng(9)
    w = synth.make_world(1001)
    full = np.ascontiguousarray(synth.lidar_scan(w, synth.se3(3.0, (0.4, -0.2, 0.0)), seed=4)[:, :3])
    dup = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    dup[1000:2000] = dup[:1000]                           # exact duplicates: equal keys, equal coordinates
    dup[2500:] = np.float32(1.25)                         # 500 identical points
    big = np.concatenate([full, full[:20000] + np.float32(0.013)])   # 143 929 points: 71 sort tiles (> 64: the scan
                                                                      # kernel's carry over tile blocks), 14 kd levels
    return [full, np.ascontiguousarray(full[::7]), dup, rng.normal(0, 8, (2049, 3)).astype(np.float32),
            rng.uniform(-5, 5, (17, 3)).astype(np.float32), rng.uniform(-5, 5, (1, 3)).astype(np.float32), big]


def test_curve_order_is_sorted_stable_and_a_permutation(capi, clouds):
    st = capi.ScanStore()
    for c in clouds:
        d = st.debug_index(st.add(c))
        n = len(c)
        assert not d["kd"] and (np.sort(d["perm"]) == np.arange(n)).all()
        assert (np.diff(d["keys"].astype(np.int64)) >= 0).all() and d["keys"].max() < (1 << 30)
        same = np.diff(d["keys"].astype(np.int64)) == 0   # equal keys keep ascending original index (stable sort)
        assert (np.diff(d["perm"].astype(np.int64))[same] > 0).all()
        # launch order: groups of 128 sorted points, widest bounding box first, equal extents in ascending id
        p = c[d["perm"]]
        ng = (n + 127) // 128
        ext = np.empty(ng, np.float32)
        for g in range(ng):
            q = p[g * 128:(g + 1) * 128]
            dd = (q.max(0) - q.min(0)).astype(np.float32)
            ext[g] = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
        assert (np.sort(d["order2"]) == np.arange(ng)).all()
        eo = ext[d["order2"]]
        assert (np.diff(eo) <= 0).all()
        assert (np.diff(d["order2"].astype(np.int64))[np.diff(eo) == 0] > 0).all()
    st.close()


def test_a_batch_of_scans_is_indexed_like_the_scans_one_by_one(capi, clouds):
    st = capi.ScanStore()
    one = [st.debug_index(st.add(c)) for c in clouds]
    ids = st.add_batch(clouds + [np.zeros((0, 3), np.float32)])
    assert st.points(ids[-1]) == 0
    for c, i, a in zip(clouds, ids, one):
        b = st.debug_index(i)
        assert (st.download(i) == c).all()
        for k in ("perm", "keys", "kpos", "order2"):
            assert (a[k] == b[k]).all(), k
    kitti = [np.concatenate([c, np.ones((len(c), 1), np.float32)], 1) for c in clouds[:3]]   # x y z i: stride 4
    for i, a in zip(st.add_batch(kitti), one):
        assert (st.debug_index(i)["perm"] == a["perm"]).all()
    st.close()


def test_kd_order_is_the_stated_rule(capi, clouds):
    st = capi.ScanStore()
    ids = st.add_batch(clouds)
    before = [st.debug_index(i) for i in ids]
    st.build_target_index_batch(ids)                      # one batch: scans of 13, 11, 8, 8, 1 and 0 levels together
    for c, i, b in zip(clouds, ids, before):
        d = st.debug_index(i)
        assert d["kd"] and (d["keys"] == b["keys"]).all()  # the curve keys stay the cold-start lookup
        want = kd_order_numpy(c[b["perm"]])               # kd position -> curve position
        assert (d["perm"] == b["perm"][want]).all()
        inv = np.empty(len(c), np.int64)
        inv[want] = np.arange(len(c))
        assert (d["kpos"] == inv).all()                   # curve position -> kd position
        assert (np.sort(d["order2"]) == np.arange((len(c) + 127) // 128)).all()
    one = capi.ScanStore()                                # the same scans re-sorted one at a time
    for c, i in zip(clouds, ids):
        j = one.build_target_index(one.add(c))
        assert (one.debug_index(j)["perm"] == st.debug_index(i)["perm"]).all()
    one.close()
    st.close()


def test_kd_cells_are_disjoint_along_the_split_axis(capi, clouds):
    """The property the search gains from: the two halves of every kd node are separated along the node's widest
    axis (lower half <= upper half), so sibling boxes overlap in at most a plane."""
    st = capi.ScanStore()
    c = clouds[0]
    i = st.build_target_index(st.add(c))
    p = c[st.debug_index(i)["perm"]]
    n = len(p)
    L = 0
    while (16 << L) < n:
        L += 1
    for l in (0, 3, 7, L - 1):
        size = 16 << (L - l)
        for node in range(0, min(1 << l, 40)):
            a, b = node * size, min((node + 1) * size, n)
            if b - a <= size // 2:
                continue
            q = p[a:b]
            ax = int(np.argmax(q.max(0) - q.min(0)))
            assert q[:size // 2, ax].max() <= q[size // 2:, ax].min()
    st.close()


# ---- the whole index against scan_index_ref.py ---------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def fetch(st, i):
    """Everything the two developer exports give for scan i: debug_index + debug_boxes, the launch orders of all settings."""
    d = st.debug_index(i)
    d.update(st.debug_boxes(i, 2))
    d["orders"] = {cs: (d["order"] if cs == 2 else st.debug_boxes(i, cs)["order"]) for cs in (1, 2, 4)}
    return d


def check_header(c, d, finite_only=False):
    h = ref.header(c, finite_only=finite_only)
    assert (d["lo"] == h["lo"]).all() and (d["hi"] == h["hi"]).all(), (d["lo"], h["lo"], d["hi"], h["hi"])
    for k in ("ox", "oy", "oz", "inv_cell"):
        got, want = np.float32(d[k]), np.float32(h[k])
        assert got.view(np.uint32) == want.view(np.uint32), (k, got, want)      # bit for bit: IEEE division, no contraction
    return h


def check_keys(c, d, rows=None):
    """keys[s] is the Hilbert key, on the header's own grid, of the point with the s-th smallest key (through kpos in a
    kd-ordered index); rows: the original indices judged (all by default)."""
    if not len(c):
        return
    orig = d["perm"][d["kpos"]]                                               # curve position -> original index
    want = ref.hilbert_key(c[orig], d["ox"], d["oy"], d["oz"], d["inv_cell"])
    sel = np.ones(len(c), bool) if rows is None else rows[orig]
    assert (d["keys"][sel] == want[sel]).all()


def check_boxes(c, d, tight=True):
    """Containment of every finite coordinate at all three levels (exact), tightness of every level against the
    derived bounds, the empty sub-blocks, the padding points."""
    n = len(c)
    if not n:
        assert all(len(d[k]) == 0 for k in ("box_lo", "box_hi", "sb2", "sup_lo", "sup_hi", "pad"))
        return
    z = ref.sizes(n)
    p = c[d["perm"]]
    assert len(d["box_lo"]) == z["nch"] and len(d["sb2"]) == z["npairs"] and len(d["sup_lo"]) == z["nsup"]
    cc, nh = d["box_lo"][:, :3], d["box_hi"][:, :3]
    mn, mx = ref.block_minmax(p, ref.CH)
    assert ref.boxes_contain(cc, nh, mn, mx).all(), "a chunk box misses a point"
    sc, snh = ref.unpack_sb2(d["sb2"])
    smn, smx = ref.block_minmax(p, ref.SB, 2 * z["npairs"])
    assert ref.boxes_contain(sc, snh, smn, smx).all(), "a sub-block box misses a point"
    past = np.arange(2 * z["npairs"]) * ref.SB >= n
    assert (sc[past] == 0).all() and (snh[past] == ref.EMPTY_NH).all(), "an empty sub-block is not the empty box"
    umn, umx = ref.block_minmax(p, ref.CH * ref.SUP)
    ulo, uhi = d["sup_lo"][:, :3].astype(np.float64), d["sup_hi"][:, :3].astype(np.float64)
    assert ((umn > umx) | ((ulo <= umn) & (umx <= uhi))).all(), "a super box misses a point"
    assert len(d["pad"]) == z["n_pad"] - n and ref.padding_ok(d["pad"])
    if tight:
        assert ref.boxes_tight(cc, nh, mn, mx).all(), "a chunk box is wider than its arithmetic allows"
        assert ref.boxes_tight(sc, snh, smn, smx).all(), "a sub-block box is wider than its arithmetic allows"
        assert ref.super_contain_chunks(d["sup_lo"], d["sup_hi"], cc, nh).all(), "a super box misses a chunk box"
        assert ref.super_tight(d["sup_lo"], d["sup_hi"], cc, nh).all(), "a super box is wider than its slack allows"


def check_orders(c, d):
    p = c[d["perm"]]
    for cs in (1, 2, 4):
        assert (d["orders"][cs] == ref.launch_order(p, 64 * cs)).all(), cs


@pytest.fixture(scope="module")
def edge(capi):
    """4a's batch -- one add_batch call at every size where the structure changes, an empty scan among them; add_batch
    takes one stride per call, so the x y z i cloud comes in a call of its own (400 m wide: the one scan here whose key
    grid has cells above the 0.25 m floor) -- fetched in curve order, then re-sorted into kd order in one
    build_target_index_batch and fetched again."""
    st = capi.ScanStore()
    clouds = ref.edge_clouds()
    ids = st.add_batch(clouds)
    c4 = np.concatenate([ref.uniform_cloud(4099, 5, side=400.0), np.ones((4099, 1), np.float32)], 1)
    ids += st.add_batch([c4])
    clouds.append(np.ascontiguousarray(c4[:, :3]))
    curve = [fetch(st, i) for i in ids]
    st.build_target_index_batch(ids)
    kd = [fetch(st, i) for i in ids]
    st.close()
    return dict(clouds=clouds, curve=curve, kd=kd)


def test_edge_batch_headers_and_keys_are_the_statement(edge):
    for c, d, k in zip(edge["clouds"], edge["curve"], edge["kd"]):
        assert not d["kd"] and (k["kd"] or len(c) == 0)
        for x in (d, k):
            check_header(c, x)
            check_keys(c, x)
        if len(c):
            perm, keys = ref.curve_order(c)                                    # the whole statement: order and keys
            assert (d["perm"] == perm).all() and (d["keys"] == keys).all() and (k["keys"] == keys).all()


def test_edge_batch_boxes_and_padding(edge):
    for c, d, k in zip(edge["clouds"], edge["curve"], edge["kd"]):
        check_boxes(c, d)
        check_boxes(c, k)


def test_edge_batch_launch_orders_for_1_2_4_sources_per_lane(edge):
    for c, d, k in zip(edge["clouds"], edge["curve"], edge["kd"]):
        check_orders(c, d)
        check_orders(c, k)


def test_edge_batch_kd_order_is_the_stated_rule(edge):
    for c, d, k in zip(edge["clouds"], edge["curve"], edge["kd"]):
        if len(c):
            assert (k["perm"] == d["perm"][kd_order_numpy(c[d["perm"]])]).all(), len(c)


def test_debug_boxes_refuses_what_debug_index_refuses(capi):
    st = capi.ScanStore()
    i = st.add(ref.uniform_cloud(10, 1))
    assert len(st.debug_boxes(i, 4)["order"]) == 1             # (the call declares the entry's argument types)
    f, none = capi.lib().gloc_scan_store_debug_boxes, [None] * 9
    invalid = [k for k, v in capi.ERR_NAMES.items() if v == "GLOC_ERR_INVALID"][0]
    assert f(None, i, 2, *none) == invalid and "null store" in capi.lib().gloc_last_error().decode()
    assert f(st._h, i + 100, 2, *none) == invalid and "unknown scan id" in capi.lib().gloc_last_error().decode()
    order = np.empty(1, np.uint32)
    assert f(st._h, i, 3, *none[:8], order.ctypes.data) == invalid     # 3 sources per lane: no such launch order
    assert f(st._h, i, 2, *none) == capi.GLOC_OK                       # every output may be null
    st.release(i)
    assert f(st._h, i, 2, *none) == invalid
    st.close()


@pytest.mark.parametrize("n", [262144, 262145])
def test_launch_order_at_the_limit_of_the_in_lds_sort(capi, n):
    """One source per lane: 4096 groups are sorted in LDS, 4097 by the 32-bit radix sort."""
    st = capi.ScanStore()
    c = ref.uniform_cloud(n, 3)
    i = st.add(c)
    p = c[st.debug_index(i)["perm"]]
    assert (st.debug_boxes(i, 1)["order"] == ref.launch_order(p, 64)).all()
    st.close()


def test_equal_extents_keep_ascending_group_id_on_both_sort_paths(capi):
    st = capi.ScanStore()
    c = ref.tie_cloud()
    i = st.add(c)
    p = c[st.debug_index(i)["perm"]]
    for cs in (1, 2, 4):                                                       # 4159 groups (radix), 2080 and 1040 (LDS)
        o = st.debug_boxes(i, cs)["order"]
        k = ref.group_extent_keys(p, 64 * cs)[o].astype(np.int64)
        assert (np.diff(k) >= 0).all() and (np.diff(o.astype(np.int64))[np.diff(k) == 0] > 0).all(), cs
        assert (o == ref.launch_order(p, 64 * cs)).all(), cs
    st.close()


INDEX_ARRAYS = ("perm", "keys", "kpos", "lo", "hi", "box_lo", "box_hi", "sb2", "sup_lo", "sup_hi", "pad")


@pytest.mark.parametrize("case", range(5), ids=["i", "ii", "iii", "iv", "v"])
def test_non_finite_coordinates_take_no_part_in_the_index(capi, case):
    """A non-finite coordinate (the reference's readers pass them through) must not cost the finite points their boxes,
    nor the scan its key grid: at every level every finite coordinate lies inside its box, the header is the header of
    the finite coordinates, every wholly finite point has its key -- alone, in a batch beside a clean scan (whose index
    keeps every bit), and after the kd re-sort."""
    name, c = ref.nonfinite_clouds()[case]
    fin = np.isfinite(c).all(1)
    clean = ref.uniform_cloud(700, 8)
    st = capi.ScanStore()
    alone = fetch(st, st.add(c))
    clean_alone = fetch(st, st.add(clean))
    ids = st.add_batch([clean, c])
    clean_b, batch = fetch(st, ids[0]), fetch(st, ids[1])
    for k in INDEX_ARRAYS:
        assert same_bits(clean_alone[k], clean_b[k]), k
    assert all(same_bits(clean_alone["orders"][cs], clean_b["orders"][cs]) for cs in (1, 2, 4))
    st.build_target_index_batch(ids)
    clean_k, kd = fetch(st, ids[0]), fetch(st, ids[1])
    one = capi.ScanStore()
    clean_k1 = fetch(one, one.build_target_index(one.add(clean)))
    for k in INDEX_ARRAYS:
        assert same_bits(clean_k1[k], clean_k[k]), k
    one.close()
    st.close()
    for d in (alone, batch, kd):
        check_boxes(c, d, tight=False)
        h = check_header(c, d, finite_only=True)
        assert all(np.isfinite(h[k]) for k in ("ox", "oy", "oz", "inv_cell"))
        check_keys(c, d, rows=fin)
