"""CPU: the restatement tests/cluster_ref.py on the shared cases tests/cluster_cases.py -- against an independent
breadth-first search over the dense adjacency, and against the properties E2 - E4 state; the fuzz generator reaches both
extremes; the filters' restatement against direct statements."""
import numpy as np
import pytest

import cluster_cases as K
import cluster_ref as E

NONE = E.NONE


def bfs_roots(xyz, tolerance):
    """Components by breadth-first search, seeded in ascending index: the seed is its component's smallest index."""
    A = E.adjacency(xyz, tolerance)
    n = len(A)
    root = np.full(n, NONE, np.uint32)
    fin = E.finite_rows(xyz)
    for s in range(n):
        if root[s] != NONE or not fin[s]:
            continue
        seen = np.zeros(n, bool)
        seen[s] = True
        frontier = np.array([s])
        while len(frontier):
            nxt = A[frontier].any(axis=0) & ~seen
            seen |= nxt
            frontier = np.flatnonzero(nxt)
        root[seen] = s
    return root


def check_properties(xyz, r, min_size=1, max_size=0):
    root, label, n = r["root"], r["cluster"], len(xyz)
    fin = E.finite_rows(xyz)
    assert (root[~fin] == NONE).all() and (label[~fin] == NONE).all() and (root[fin] != NONE).all()
    live = np.flatnonzero(fin)
    assert (root[root[live]] == root[live]).all()                          # roots are fixed points
    assert (root[live] <= live).all()
    for c in np.unique(root[live]):
        assert np.flatnonzero(root == c).min() == c                        # the root is the minimum of its component
    sizes = np.bincount(root[live], minlength=n + 1)
    assert sizes.sum() == fin.sum() and r["n_components"] == (sizes > 0).sum()
    kept = (sizes >= max(min_size, 1)) & ((sizes <= max_size) if max_size else True)
    assert r["n_kept"] == kept.sum() == len(r["size"]) == len(r["cluster_root"])
    assert sorted(r["cluster_root"].tolist()) == np.flatnonzero(kept).tolist()   # the ranks are a permutation of the kept
    assert (r["size"] == sizes[r["cluster_root"]]).all()
    key = list(zip((-r["size"].astype(np.int64)).tolist(), r["cluster_root"].tolist()))
    assert key == sorted(key)                                              # descending size, ties by ascending root
    for c, cr in enumerate(r["cluster_root"]):
        assert (label[root == cr] == c).all()
    assert (label[live][~kept[root[live]]] == NONE).all()
    if r["n_kept"]:
        assert sorted(np.unique(label[label != NONE]).tolist()) == list(range(r["n_kept"]))


@pytest.mark.parametrize("name", list(K.CASES))
def test_ref_equals_bfs_and_has_the_properties(name):
    xyz, prm = K.cloud(name), K.CASES[name][1]
    r = K.ref(name)
    assert (r["root"] == bfs_roots(xyz, prm["tolerance"])).all()
    check_properties(xyz, r, prm.get("min_size", 1), prm.get("max_size", 0))
    for c in range(r["n_kept"]):
        p = xyz[r["cluster"] == c].astype(np.float64)
        assert np.allclose(r["centroid"][c], p.mean(0), rtol=1e-12, atol=1e-12)
        assert (r["lo"][c] == p.min(0)).all() and (r["hi"][c] == p.max(0)).all()


def test_the_cases_are_what_they_say():
    n = {name: (K.ref(name)["n_components"], K.ref(name)["n_kept"]) for name in K.CASES}
    assert n["one"] == (1, 1) and n["pair_at_r"] == (1, 1) and n["pair_beyond_r"] == (2, 2)
    assert n["chain"] == (1, 1) and n["chain_shuffled"] == (1, 1) and n["two_chains"] == (2, 2)
    assert K.ref("chain_shuffled")["root"].tolist() == [0] * 130
    assert sorted(K.ref("two_chains")["cluster_root"].tolist()) == [0, 1]
    assert n["duplicates"] == (1, 1) and n["isolated"] == (257, 257) and n["one_component"] == (1, 1)
    assert n["slab"] == (8, 8) and K.ref("slab")["size"][0] == 4193
    assert (~E.finite_rows(K.cloud("non_finite"))).sum() > 30
    assert sorted(K.ref("sizes_all")["size"].tolist()) == [1, 3, 4, 4, 5, 5, 6]
    s = K.ref("sizes_all")
    assert s["size"].tolist() == [6, 5, 5, 4, 4, 3, 1] and s["cluster_root"][1] < s["cluster_root"][2] and s["cluster_root"][3] < s["cluster_root"][4]
    assert K.ref("sizes_4_5")["size"].tolist() == [5, 5, 4, 4]
    assert K.ref("sizes_min6")["size"].tolist() == [6] and K.ref("sizes_max1")["size"].tolist() == [1] and n["sizes_none"] == (7, 0)


@pytest.mark.parametrize("seed", range(K.N_FUZZ))
def test_fuzz_ref_equals_bfs(seed):
    xyz, tol = K.fuzz(seed)
    r = K.fuzz_ref(seed)
    assert (r["root"] == bfs_roots(xyz, tol)).all()
    check_properties(xyz, r)


def test_fuzz_reaches_both_extremes():
    """One component of many points, every point on its own, and counts in between; all three layouts; sizes from a
    handful of points to thousands."""
    rows = [(len(K.fuzz(s)[0]), int(E.finite_rows(K.fuzz(s)[0]).sum()), K.fuzz_ref(s)["n_components"]) for s in range(K.N_FUZZ)]
    print(rows)
    assert any(f > 100 and c == 1 for _, f, c in rows)
    assert any(f > 100 and c == f for _, f, c in rows)
    assert sum(1 for _, f, c in rows if 1 < c < f) >= 10
    assert min(n for n, _, _ in rows) <= 10 and max(n for n, _, _ in rows) >= 2000
    assert any(f < n for n, f, _ in rows)                                  # some clouds carry non-finite rows


# ---- E5 - E7 -------------------------------------------------------------------------------------------------------------
def test_filters_against_direct_statements():
    xyz = K.filter_cloud()
    fin = E.finite_rows(xyz)
    p64 = xyz.astype(np.float64)
    with np.errstate(all="ignore"):
        D = np.sqrt(((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1))
    D[~fin] = np.inf
    D[:, ~fin] = np.inf
    # E5: neighbours within the radius, self excluded (the margin keeps fp32 and fp64 on the same side)
    cnt = (D <= 0.6).sum(1) - 1
    keep = E.ror_keep(xyz, 0.6, 3)
    safe = np.abs(D - 0.6).min(1) > 1e-5
    assert (keep[safe & fin] == (cnt >= 3)[safe & fin]).all() and not keep[~fin].any()
    # E6: the mean distance to the 8 nearest others, against mu + sigma
    m, mu, sigma, f2 = E.sor_stats(xyz, 8)
    Ds = np.sort(D[fin][:, fin], axis=1)
    md = Ds[:, 1:9].mean(1)
    assert (f2 == fin).all() and np.allclose(m[fin], md, rtol=1e-5, atol=1e-6)
    assert np.isclose(mu, md.mean(), rtol=1e-6) and np.isclose(sigma, md.std(), rtol=1e-5)
    k = E.sor_keep(xyz, 8, 1.0)
    assert 0.6 < k.sum() / fin.sum() < 0.99 and not k[~fin].any()
    # the range crop
    rr = np.sqrt((p64 ** 2).sum(1))
    safe = fin & (np.abs(rr - 1.5) > 1e-4) & (np.abs(rr - 30.0) > 1e-3)
    assert (E.range_keep(xyz, 1.5, 30.0)[safe] == ((rr >= 1.5) & (rr <= 30.0))[safe]).all()
    assert not E.range_keep(xyz, 1.5, 30.0)[~fin].any()


def test_the_chain_is_its_stages_one_after_the_other():
    xyz = K.filter_cloud()
    index, info = E.filtered(xyz, K.FILTER_PARAMS)
    cur = np.arange(len(xyz))
    counts = []
    for stage in E.STAGES:
        cur = cur[E.stage_keep(xyz[cur], stage, K.FILTER_PARAMS)]
        counts.append(len(cur))
    assert (index == cur).all() and [info["after_" + s] for s in E.STAGES] == counts and info["points_in"] == len(xyz)
    assert len(xyz) > counts[0] > counts[1] > counts[2] > counts[3] > 500             # every stage removes something
    for name, p in K.SINGLE_STAGES.items():
        idx1, info1 = E.filtered(xyz, p)
        assert 0 < len(idx1) < len(xyz), name
    assert len(E.filtered(xyz, K.SINGLE_STAGES["ror_none_needed"])[0]) == E.finite_rows(xyz).sum()
    with pytest.raises(ValueError):
        E.filtered(xyz, dict(max_range=30.0, cluster_tolerance=0.05, cluster_min_size=50))   # the crop leaves points, the clusters none
    with pytest.raises(ValueError):
        E.sor_stats(xyz[:5], 8)
