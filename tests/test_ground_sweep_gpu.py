"""GPU: the ground pre-alignment through the C ABI against the oracle (oracle/ground_oracle.c) over the case table of
tests/ground_cases.py -- cloud shapes and sizes for the k-NN and the normals, estimate scenes that reach one branch each, the
parameter rows, strides, refusals, and one handle re-used across sizes and both forms of the search.  Indices, distances, normals,
bins, counts, histograms and planes are compared exactly (tests/test_ground_cases_cpu.py proves the table itself on the CPU)."""
import numpy as np
import pytest

import ground_cases as gc
from util import bits

pytestmark = pytest.mark.gpu
INFO_INTS = ("n_near", "ground_bin", "n_ground", "best_hyp", "inliers", "iters_used", "found")
NORMALS_KS = tuple(k for k in gc.K_ENTRY if k >= 3)

_expected = {}          # the oracle's answers, computed once and shared by both forms of the search


def _once(key, make):
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def _oracle_lists(oracle_mod, name, k):
    return _once(("knn", name, k), lambda: oracle_mod.ground_knn(gc.shape(name), k))


def _oracle_normals(oracle_mod, name, k):
    return _once(("normals", name, k), lambda: oracle_mod.ground_normals(gc.shape(name), _oracle_lists(oracle_mod, name, k)[0]))


def _oracle_estimate(oracle_mod, name, row):
    return _once(("estimate", name, gc.row_id(row)), lambda: oracle_mod.ground_estimate(gc.scene(name), **row))


@pytest.fixture(scope="module", params=["culled", "exhaustive"])
def est(capi, request):
    """Every test runs on both forms of the k-NN search: the lists must not differ."""
    g = capi.GroundEstimator()
    g.set_option(capi.GROUND_OPT_KNN_EXHAUSTIVE, 1 if request.param == "exhaustive" else 0)
    yield g
    g.close()


# ---- 1. lists, normals and bins over the shapes and sizes ----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(gc.SHAPES))
def test_knn_equals_the_oracle(est, oracle_mod, name):
    p = gc.shape(name)
    for k in gc.K_ENTRY:
        gi, gd = est.knn(p, k)
        oi, od = _oracle_lists(oracle_mod, name, k)
        assert (gi == oi).all(), (name, k, np.flatnonzero((gi != oi).any(1))[:8])
        assert (bits(gd) == bits(od)).all(), (name, k, np.flatnonzero((bits(gd) != bits(od)).any(1))[:8])


@pytest.mark.parametrize("name", sorted(gc.SHAPES))
def test_normals_and_bins_equal_the_oracle(est, oracle_mod, name):
    p = gc.shape(name)
    for k in NORMALS_KS:
        gn, gb = est.normals(p, k)
        on, ob = _oracle_normals(oracle_mod, name, k)
        assert (bits(gn) == bits(on)).all(), (name, k, np.flatnonzero((bits(gn) != bits(on)).any(1))[:8])
        assert (gb == ob).all(), (name, k, np.flatnonzero(gb != ob)[:8])


# ---- 2. estimate scenes x parameter rows ---------------------------------------------------------------------------------

def _check_estimate(est, capi, oracle_mod, name, row):
    cloud = gc.scene(name)
    T, info, moved = est.estimate(cloud, capi.default_ground_params(**row), want_cloud=True)
    oT, oinfo = _oracle_estimate(oracle_mod, name, row)
    what = (name, gc.row_id(row))
    for key in INFO_INTS:
        assert info[key] == oinfo[key], what + (key, info[key], oinfo[key])
    assert (info["hist"] == oinfo["hist"]).all(), what
    assert (bits(info["plane"]) == bits(oinfo["plane"])).all(), what
    assert np.abs(T - oT).max() < 1e-6, what          # a few libm calls on four numbers, on the host in both
    if not oinfo["found"]:
        assert (T == np.eye(4)).all(), what
    assert moved.shape == cloud.shape and np.abs(moved[:, :3] - gc.moved_fp64(cloud, T)).max() < 1e-4, what
    if cloud.shape[1] > 3:
        assert (bits(moved[:, 3:]) == bits(cloud[:, 3:])).all(), what          # the other channels are carried along
    return info


@pytest.mark.parametrize("name", sorted(gc.SCENES))
def test_estimate_equals_the_oracle(est, capi, oracle_mod, name):
    for row in gc.rows_of(name):
        _check_estimate(est, capi, oracle_mod, name, row)


def test_estimate_device_at_stride_16(est, capi, oracle_mod):
    import torch
    cloud = gc.scene("lidar16")
    d_in = torch.from_numpy(np.array(cloud)).cuda()
    for row in (gc.DEFAULTS, gc.PARAM_ROWS[-3]):
        d_out = torch.full_like(d_in, 7.0)
        T, info = est.estimate_device(d_in.data_ptr(), cloud.shape[0], 16, d_out.data_ptr(), capi.default_ground_params(**row))
        torch.cuda.synchronize()
        oT, oinfo = _oracle_estimate(oracle_mod, "lidar16", row)
        for key in INFO_INTS:
            assert info[key] == oinfo[key], key
        assert (info["hist"] == oinfo["hist"]).all() and (bits(info["plane"]) == bits(oinfo["plane"])).all()
        assert np.abs(T - oT).max() < 1e-6
        moved = d_out.cpu().numpy()
        assert np.abs(moved[:, :3] - gc.moved_fp64(cloud, T)).max() < 1e-4
        assert (bits(moved[:, 3:]) == bits(cloud[:, 3:])).all()
    # without an output buffer: the same transform
    T2, info2 = est.estimate_device(d_in.data_ptr(), cloud.shape[0], 16, None, capi.default_ground_params(**gc.PARAM_ROWS[-3]))
    assert (bits(T2) == bits(T)).all() and info2["inliers"] == info["inliers"]


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_usable(est, capi, oracle_mod):
    import torch
    cloud = gc.scene("lidar3")
    p = gc.shape("size321")
    d_in = torch.from_numpy(np.array(gc.scene("lidar16"))).cuda()

    def usable():
        _check_estimate(est, capi, oracle_mod, "lidar3", gc.DEFAULTS)
        gi, gd = est.knn(p, 10)
        oi, od = _oracle_lists(oracle_mod, "size321", 10)
        assert (gi == oi).all() and (bits(gd) == bits(od)).all()

    usable()
    wide = np.zeros((cloud.shape[0], 17), np.float32)
    wide[:, :3] = cloud
    refused = [lambda: est.estimate(np.ascontiguousarray(cloud[:, :2])), lambda: est.estimate(wide),
               lambda: est.estimate(np.ascontiguousarray(cloud[:, :2]), want_cloud=True), lambda: est.estimate(wide, want_cloud=True),
               lambda: est.estimate_device(d_in.data_ptr(), d_in.shape[0], 2), lambda: est.estimate_device(d_in.data_ptr(), d_in.shape[0], 17),
               lambda: est.estimate(cloud, capi.default_ground_params(knn=2)), lambda: est.estimate(cloud, capi.default_ground_params(knn=17)),
               lambda: est.estimate_device(d_in.data_ptr(), d_in.shape[0], 16, None, capi.default_ground_params(knn=17)),
               lambda: est.estimate(cloud, capi.default_ground_params(ransac_iters=0)),
               lambda: est.estimate(cloud, capi.default_ground_params(ransac_iters=65537)),
               lambda: est.knn(p, 0), lambda: est.knn(p, 17), lambda: est.normals(p, 2), lambda: est.normals(p, 17)]
    for n, call in enumerate(refused):
        with pytest.raises(capi.GlocError):
            call()
        if n % 2 == 1:
            usable()
    usable()


# ---- 4. one handle across sizes and both forms ---------------------------------------------------------------------------

def _flat(*arrays):
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrays]


def _run_estimate(g, cloud):
    T, info, moved = g.estimate(cloud, want_cloud=True)
    return _flat(T, np.array([info[k] for k in INFO_INTS], np.int64), info["hist"], info["plane"], moved)


def _run_shape(g, p):
    idx, d2 = g.knn(p, 10)
    nrm, b = g.normals(p, 16)
    return _flat(idx, d2, nrm, b) + _run_estimate(g, p)


@pytest.mark.parametrize("start", (0, 1), ids=("culled_first", "exhaustive_first"))
def test_one_handle_across_a_sequence(capi, start):
    """The handle's buffers only grow and keep the last call's lists: big, small, all ties, the other form of the search, big
    again, nothing, the tile edges -- every answer is the one a fresh handle gives."""
    big = gc.big_scene()
    steps = [("big", lambda g: _run_estimate(g, big)),
             ("size63", lambda g: _run_shape(g, gc.shape("size%d" % gc.SIZES[2]))),
             ("identical", lambda g: _run_shape(g, gc.shape("identical"))),
             ("flip", None),
             ("big again", lambda g: _run_estimate(g, big)),
             ("empty", lambda g: _run_estimate(g, np.zeros((0, 3), np.float32)))]
    steps += [(n, lambda g, n=n: _run_estimate(g, gc.scene(n))) for n in sorted(gc.SCENES) if n.startswith("tile_edges")]
    steps += [("size4097", lambda g: _run_shape(g, gc.shape("size4097"))), ("size257", lambda g: _run_shape(g, gc.shape("size257")))]
    form = start
    one = capi.GroundEstimator()
    try:
        one.set_option(capi.GROUND_OPT_KNN_EXHAUSTIVE, form)
        for name, run in steps:
            if run is None:
                form = 1 - form
                one.set_option(capi.GROUND_OPT_KNN_EXHAUSTIVE, form)
                continue
            fresh = capi.GroundEstimator()
            try:
                fresh.set_option(capi.GROUND_OPT_KNN_EXHAUSTIVE, form)
                want = run(fresh)
            finally:
                fresh.close()
            got = run(one)
            assert len(got) == len(want)
            for n, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and (a == b).all(), (name, n)
    finally:
        one.close()
