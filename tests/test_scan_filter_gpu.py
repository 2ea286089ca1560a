"""GPU: the outlier filters and derived scans (gloc_scan_store_add_filtered, gloc_scan_store_add_subset; E5 - E7) against
tests/cluster_ref.py on tests/cluster_cases.py's filter cloud.  A derived scan is the rows the restatement keeps, in upload
order, bit for bit; the combined entry equals the chain of its single-stage calls; a derived scan is a resident scan like
any other."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as K
import cluster_ref as E
from util import bits

pytestmark = pytest.mark.gpu
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)


@pytest.fixture(scope="module")
def env(capi):
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    base = store.add(K.filter_cloud())
    yield dict(store=store, reg=reg, capi=capi, base=base)
    reg.close()
    store.close()


def _rows_equal(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


@pytest.mark.parametrize("name", list(K.SINGLE_STAGES))
def test_one_stage_equals_the_restatement(env, name):
    store, xyz, p = env["store"], K.filter_cloud(), K.SINGLE_STAGES[name]
    index, info = E.filtered(xyz, p)
    sid, got = store.add_filtered(env["base"], want_info=True, **p)
    out = store.download(sid)
    print(name, "in", len(xyz), "kept", len(out), "expected", len(index), got)
    assert got == info and store.points(sid) == len(index)
    assert _rows_equal(out, xyz[index])
    store.release(sid)


def test_statistics_over_more_than_64_runs(env):
    """4 200 points are 66 runs of 64: E6's second level, the sum of the runs' sums, goes round more than once."""
    store, xyz, p = env["store"], K.cloud("slab"), dict(sor_mean_k=4, sor_std_mul=0.5)
    index, info = E.filtered(xyz, p)
    base = store.add(xyz)
    sid, got = store.add_filtered(base, want_info=True, **p)
    print("slab: in", len(xyz), "kept", got["after_sor"], "expected", len(index))
    assert got == info and 0 < len(index) < len(xyz) and _rows_equal(store.download(sid), xyz[index])
    store.release(sid)
    store.release(base)


def test_all_stages_equal_the_chain_of_single_calls(env):
    store, xyz, p = env["store"], K.filter_cloud(), K.FILTER_PARAMS
    index, info = E.filtered(xyz, p)
    before = len(store)
    sid, got = store.add_filtered(env["base"], want_info=True, **p)
    assert len(store) == before + 1                        # the intermediate scans are gone
    out = store.download(sid)
    print("combined", got, "expected", info)
    assert got == info and _rows_equal(out, xyz[index])
    stages = (dict(min_range=p["min_range"], max_range=p["max_range"]), dict(ror_radius=p["ror_radius"], ror_min_neighbors=p["ror_min_neighbors"]),
              dict(sor_mean_k=p["sor_mean_k"], sor_std_mul=p["sor_std_mul"]),
              dict(cluster_tolerance=p["cluster_tolerance"], cluster_min_size=p["cluster_min_size"], cluster_max_size=p["cluster_max_size"]))
    cur, made, counts = env["base"], [], []
    for st in stages:
        cur = store.add_filtered(cur, **st)
        made.append(cur)
        counts.append(store.points(cur))
    assert counts == [info["after_range"], info["after_ror"], info["after_sor"], info["after_cluster"]]
    assert _rows_equal(store.download(cur), out)
    # ... and the same with a target index on the base scan: nothing depends on it
    twin = store.add(xyz)
    store.build_target_index(twin)
    sid2 = store.add_filtered(twin, **p)
    assert _rows_equal(store.download(sid2), out)
    for s in made + [sid, sid2, twin]:
        store.release(s)


def test_no_stage_is_a_copy(env):
    store, xyz = env["store"], K.filter_cloud()
    sid, info = store.add_filtered(env["base"], want_info=True)
    assert set(info.values()) == {len(xyz)}
    assert (store.download(sid).view(np.uint32) == xyz.view(np.uint32)).all()       # (NaN rows and all)
    store.release(sid)


def test_a_chain_that_leaves_nothing_is_refused(env):
    store, capi, L = env["store"], env["capi"], env["capi"].lib()
    before = len(store)
    cases = (dict(max_range=30.0, cluster_tolerance=0.05, cluster_min_size=50), dict(min_range=500.0), dict(ror_radius=0.01, ror_min_neighbors=50),
             dict(max_range=0.5, sor_mean_k=15))           # (the last: fewer than 16 finite points reach the statistical stage)
    for p in cases:
        prm, sid, info = capi.default_scan_filter_params(**p), C.c_uint32(7), capi.ScanFilterInfo()
        rc = L.gloc_scan_store_add_filtered(store._h, env["base"], C.byref(prm), C.cast(C.pointer(sid), C.c_void_p), C.cast(C.pointer(info), C.c_void_p))
        print(p, rc, info.as_dict())
        assert rc == INV and sid.value == 7 and len(store) == before and info.points_in == len(K.filter_cloud())
    with pytest.raises(ValueError):
        E.filtered(K.filter_cloud(), cases[0])
    empty = store.add(np.zeros((0, 3), np.float32))
    with pytest.raises(Exception):
        store.add_filtered(empty, max_range=5.0)
    with pytest.raises(Exception):
        store.add_filtered(empty)
    store.release(empty)
    with pytest.raises(Exception):
        store.add_filtered(empty, max_range=5.0)           # an unknown id
    assert len(store) == before


def test_subset_is_a_gather_in_the_order_given(env):
    store, xyz = env["store"], K.filter_cloud()
    n = len(xyz)
    for idx in (np.arange(n)[::-1], np.array([5, 5, 5, 0, n - 1, 5]), np.array([n - 1]), np.random.default_rng(3).integers(0, n, 700)):
        sid = store.add_subset(env["base"], idx)
        assert (store.download(sid).view(np.uint32) == xyz[idx].view(np.uint32)).all()
        store.release(sid)
    before = len(store)
    for bad in (np.array([0, n]), np.array([0xFFFFFFFF]), np.zeros(0, np.uint32)):
        with pytest.raises(Exception):
            store.add_subset(env["base"], bad)
    assert len(store) == before


def test_a_derived_scan_is_a_full_citizen(env):
    """Normals and one point-to-plane row on a derived scan equal the same calls on an uploaded copy of its points."""
    store, reg, xyz = env["store"], env["reg"], K.filter_cloud()
    index, _ = E.filtered(xyz, K.FILTER_PARAMS)
    derived = store.add_filtered(env["base"], **K.FILTER_PARAMS)
    copy = store.add(xyz[index])
    for s in (derived, copy):
        store.build_normals(s, 10)
    assert _rows_equal(store.normals(derived), store.normals(copy))
    c, s_ = np.cos(0.02), np.sin(0.02)
    T = np.array([[c, -s_, 0, 0.05], [s_, c, 0, -0.03], [0, 0, 1, 0.01], [0, 0, 0, 1]], np.float32)
    src = store.add((xyz[index].astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]).astype(np.float32))
    store.build_target_index(derived)
    store.build_target_index(copy)
    a = reg.p2l_pairs([src], [derived])
    b = reg.p2l_pairs([src], [copy])
    print("p2l on the derived scan: rmse", a[1], "iterations", a[2], "status", a[3])
    assert all((np.asarray(x).view(np.uint32) == np.asarray(y).view(np.uint32)).all() for x, y in zip(a, b))
    assert a[2][0] >= 1 and np.isfinite(a[1][0]) and a[1][0] < 0.1         # it did register: the source is the scan moved by 5 cm
    for s in (derived, copy, src):
        store.release(s)
