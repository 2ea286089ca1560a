"""GPU: the split planes a target index keeps of its kd order (KdRecord, scan_index.hpp) against numpy.

The table is downloaded (gloc_scan_store_debug_kd_table) with the sorted points and the descent re-derived on the host:
one record of seven planes per three levels, right iff coordinate > split, +inf planes where the right half holds no
real point.  Checked: every finite target point is located in the sub-block that holds it, or in one that holds an
exact duplicate of it; the cells rebuilt from the planes alone (top down, no query involved) hold the finite points of
their sub-blocks; every random query point ends in a leaf whose rebuilt cell contains it and that has a real point;
no path leaves the table, whatever the query (NaN and infinities included).

The clouds have distinct coordinates per axis (a split by position cannot separate two different points that tie on
the split axis: such a point may be located on the other side, which costs a looser bound and nothing else) plus
exact copies of whole points, which the rule above allows for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SB = 16


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    c = np.stack([(rng.permutation(n) + rng.uniform(0.1, 0.9, n)) * s for s in (0.05, 0.03, 0.004)], 1).astype(np.float32)
    c -= c.mean(0).astype(np.float32)
    if n >= 8:                                            # exact copies of whole points, scattered
        dst = rng.choice(n, n // 8, replace=False)
        c[dst] = c[rng.integers(0, n, n // 8)]
    return np.ascontiguousarray(c)


def special(kind):
    rng = np.random.default_rng(7)
    if kind == "identical":
        return np.tile(np.float32([1.5, -2.25, 0.75]), (300, 1))
    if kind == "plane":                                   # two degenerate axes: only y varies
        c = np.zeros((1000, 3), np.float32)
        c[:, 0], c[:, 2] = 3.0, -1.0
        c[:, 1] = (rng.permutation(1000) + rng.uniform(0.1, 0.9, 1000)) * 0.01
        return c
    c = cloud(1500, 11)                                   # non-finite records among ordinary points
    bad = rng.choice(1500, 60, replace=False)
    vals = np.float32([np.inf, -np.inf, np.nan, -np.nan])
    for k, i in enumerate(bad):
        c[i, k % 3] = vals[k % 4]
        if k % 5 == 0:
            c[i] = vals[(k // 5) % 4]
    return c


def level_records(n, R, r):
    return ((n - 1) >> (4 + 3 * (R - r))) + 1


def locate(tab, n, Q):
    """The descent as the search kernel does it: the sub-block index per row of Q, and that no path left the table."""
    R = tab["rounds"]
    split, axes = tab["split"], tab["axes"]
    node = np.zeros(len(Q), np.int64)
    first = 0
    rows = np.arange(len(Q))
    with np.errstate(invalid="ignore"):
        for r in range(R):
            cnt = level_records(n, R, r)
            assert (node < cnt).all(), "a path left the records of its level"
            rec = first + node
            ax, sp = axes[rec], split[rec]
            g0 = Q[rows, ax & 3] > sp[:, 0]
            h1 = 1 + g0
            g1 = Q[rows, (ax >> (2 * h1)) & 3] > sp[rows, h1]
            h2 = 3 + 2 * g0 + g1
            g2 = Q[rows, (ax >> (2 * h2)) & 3] > sp[rows, h2]
            node = node * 8 + (h2 - 3) * 2 + g2
            first += cnt
    assert first == len(split)
    return node


def leaf_cells(tab, n):
    """Cells of the leaves with real points, from the planes alone: lo < x <= hi per axis (top down over the records)."""
    R = tab["rounds"]
    firsts = np.cumsum([0] + [level_records(n, R, r) for r in range(R)])
    cells = {}

    def rec(r, i, lo, hi):
        if r == R:
            cells[i] = (lo, hi)
            return
        sp, ax = tab["split"][firsts[r] + i], int(tab["axes"][firsts[r] + i])
        stack = [(0, 0, lo, hi)]                          # (heap node, depth, cell)
        while stack:
            h, d, l, u = stack.pop()
            if d == 3:
                child = i * 8 + (h - 7)
                if child * (SB * 8 ** (R - r - 1)) < n:   # (a child without real positions has no record / no leaf)
                    rec(r + 1, child, l, u)
                continue
            a, s = (ax >> (2 * h)) & 3, sp[h]
            ul, lr = u.copy(), l.copy()
            ul[a] = min(u[a], s)
            lr[a] = max(l[a], s)
            stack.append((2 * h + 1, d + 1, l, ul))
            if s < np.inf:                                # nothing exceeds a +inf plane: the right side is empty
                stack.append((2 * h + 2, d + 1, lr, u))

    rec(0, 0, np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32))
    return cells


def points_locate_to_their_sub_blocks(tab, p):
    """Every finite point of the sorted points p: located in its own sub-block, or in one with an exact copy of it."""
    n = len(p)
    fin = np.isfinite(p).all(1)
    leaf = locate(tab, n, p)
    assert (leaf * SB < n).all()
    own = leaf == np.arange(n) // SB
    for j in np.nonzero(fin & ~own)[0]:
        blk = p[leaf[j] * SB:min(leaf[j] * SB + SB, n)]
        assert (blk == p[j]).all(1).any(), (j, p[j], leaf[j])


CASES = [("n", n) for n in (1, 15, 16, 17, 127, 128, 129, 2049, 5000)] + [("special", k) for k in ("identical", "plane", "nonfinite")]


@pytest.fixture(scope="module")
def store(capi):
    st = capi.ScanStore()
    yield st
    st.close()


@pytest.mark.parametrize("kind,arg", CASES)
def test_split_planes_locate_points_and_queries(store, kind, arg):
    c = cloud(arg, 100 + arg) if kind == "n" else special(arg)
    n = len(c)
    i = store.add(c)
    assert store.debug_kd_table(i)["rounds"] == 0, "a scan in curve order has no table"
    store.build_target_index(i)
    d = store.debug_index(i)
    tab = store.debug_kd_table(i)
    p = c[d["perm"]]                                      # the points in sorted (kd) order
    if n <= SB:                                           # one sub-block: nothing to descend
        assert tab["rounds"] == 0 and len(tab["split"]) == 0
        store.release(i)
        return
    L = int(np.ceil(np.log2(n / SB)))
    assert tab["rounds"] == (L + 2) // 3
    assert (tab["axes"] >> 14 == 0).all() and ((tab["axes"][:, None] >> (2 * np.arange(7))) & 3 < 3).all()
    assert not np.isnan(tab["split"]).any()

    fin = np.isfinite(p).all(1)
    points_locate_to_their_sub_blocks(tab, p)

    # the cells rebuilt from the planes hold the finite coordinates of their sub-blocks' points (closed: ties sit on a plane)
    cells = leaf_cells(tab, n)
    assert sorted(cells) == list(range((n + SB - 1) // SB)), "one cell per sub-block with real points, no other"
    for b, (lo, hi) in cells.items():
        blk = p[b * SB:min(b * SB + SB, n)]
        f = np.isfinite(blk)
        assert ((blk >= lo) | ~f).all() and ((blk <= hi) | ~f).all(), b

    # random queries -- inside, around and far outside the cloud, on the planes themselves, non-finite
    rng = np.random.default_rng(5)
    pf = p[fin]
    mid, ext = pf.mean(0), np.maximum(pf.max(0) - pf.min(0), 1.0)
    Q = np.concatenate([pf[rng.integers(0, len(pf), 400)] + rng.normal(0, 0.05, (400, 3)),
                        mid + rng.uniform(-1, 1, (400, 3)) * ext, mid + rng.uniform(-1, 1, (100, 3)) * 1e6]).astype(np.float32)
    sp = tab["split"][np.isfinite(tab["split"])]
    if len(sp):
        on = Q[:300].copy()
        on[np.arange(300), rng.integers(0, 3, 300)] = sp[rng.integers(0, len(sp), 300)]
        Q = np.concatenate([Q, on])
    weird = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.inf] * 3, [-np.inf] * 3, [np.nan] * 3, [3e38, -3e38, 3e38]])
    ql = locate(tab, n, np.concatenate([Q, weird]))
    assert (ql * SB < n).all(), "every path ends in a sub-block with a real point"
    for k in range(len(Q)):
        lo, hi = cells[int(ql[k])]
        assert (Q[k] > lo).all() and (Q[k] <= hi).all(), (k, Q[k], lo, hi)
    store.release(i)


def test_a_table_is_rebuilt_with_its_block_and_counted_in_the_store_bytes(store):
    """A released scan's block is reused by the next scan of its size: the table is the new scan's.  The table is part of
    the scan's one allocation, which gloc_scan_store_bytes counts."""
    a = cloud(2049, 1)
    i = store.add(a)
    store.build_target_index(i)
    ta = store.debug_kd_table(i)
    assert store.bytes()[0] >= a.nbytes + 32 * len(ta["split"])
    store.release(i)
    b = cloud(2049, 2)
    j = store.add(b)
    assert store.debug_kd_table(j)["rounds"] == 0
    store.build_target_index(j)
    tb = store.debug_kd_table(j)
    points_locate_to_their_sub_blocks(tb, b[store.debug_index(j)["perm"]])
    assert ta["split"].shape == tb["split"].shape and not (ta["split"] == tb["split"]).all()
    store.release(j)
