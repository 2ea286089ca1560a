"""GPU: the cold 1-NN pass that takes its starting bounds from the target's kd tree, against the brute-force kernel.

A cold wave locates its sources in the target's split planes (KdRecord) and starts from the distance to the leaf's
points; a bound only decides which pairs are evaluated, so correspondences AND squared distances must equal the
exhaustive kernel's bit for bit.  Targets of 17, 129, 2 049 and 5 000 points in kd order, one of 2 049 without a kd index
(the fallback: curve neighbours) and a dense plane of 8 192 points under sources 1 m above it (every chunk within every
source's bound: waves give up and the second launch finishes them); sources of 1, 127, 128, 129 and 3 000 points made of:
points near the targets, points equal to target points, points exactly on split planes, points far outside the targets'
boxes and non-finite points.  Each pair with RANSAC in front (the pairs pass is the cold one) and without (the first ICP
pass is), through the library and, in a child pytest, through its small-queue variant."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "gloc3d_amd", "lib", "libgloc3d_smallq.so")

TARGET_SIZES = (17, 129, 2049, 5000)
SOURCE_SIZES = (1, 127, 128, 129, 3000)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def target(n, seed):
    """A slab of n points, 12 m x 9 m x 1.5 m, some of them exact copies of others."""
    rng = np.random.default_rng(seed)
    c = (rng.uniform(-1, 1, (n, 3)) * (6.0, 4.5, 0.75)).astype(np.float32)
    c[rng.choice(n, n // 10, replace=False)] = c[rng.integers(0, n, n // 10)]
    return np.ascontiguousarray(c)


@pytest.fixture(scope="module")
def world(capi):
    """The store with every target and every source of the module, made once."""
    store = capi.ScanStore()
    tg = [target(n, 40 + n) for n in TARGET_SIZES]
    tids = [store.add(t) for t in tg]
    store.build_target_index_batch(tids)
    tg.append(target(2049, 77))                            # no kd index: no table, the curve neighbours
    tids.append(store.add(tg[-1]))
    assert not store.debug_index(tids[-1])["kd"] and store.debug_kd_table(tids[-1])["rounds"] == 0
    gx, gy = np.meshgrid(np.arange(128, dtype=np.float32) * 0.02, np.arange(64, dtype=np.float32) * 0.02)
    plane = np.ascontiguousarray(np.stack([gx.ravel(), gy.ravel(), np.zeros(8192, np.float32)], 1))
    tg.append(plane)
    tids.append(store.add(plane))
    store.build_target_index(tids[-1])

    rng = np.random.default_rng(3)
    planes = []                                            # (axis, split) of the real nodes of every table
    for i in tids:
        tab = store.debug_kd_table(i)
        for h in range(7):
            ok = np.isfinite(tab["split"][:, h]) if len(tab["split"]) else np.zeros(0, bool)
            planes += list(zip(((tab["axes"][ok] >> (2 * h)) & 3).tolist(), tab["split"][ok, h].tolist()))
    allp = np.concatenate(tg[:5])

    def source(m):
        s = np.empty((m, 3), np.float32)
        for k in range(m):
            kind = k % 5 if m >= 127 else 0
            base = allp[rng.integers(0, len(allp))]
            if kind == 0:                                  # near a target point
                s[k] = base + rng.normal(0, 0.05, 3).astype(np.float32)
            elif kind == 1:                                # a target point itself
                s[k] = base
            elif kind == 2:                                # exactly on a split plane
                a, v = planes[rng.integers(0, len(planes))]
                s[k] = base + rng.normal(0, 0.3, 3).astype(np.float32)
                s[k, a] = v
            elif kind == 3:                                # far outside every box
                s[k] = rng.choice([-1.0, 1.0], 3) * rng.uniform(50, 5000, 3)
            else:                                          # 1 m above the dense plane
                s[k] = (rng.uniform(0, 2.54), rng.uniform(0, 1.26), 1.0)
        if m >= 127:                                       # non-finite points, one per kind and place
            for k, v in enumerate([np.nan, np.inf, -np.inf]):
                s[5 + 7 * k, k] = v
            s[40] = np.nan
        return np.ascontiguousarray(s)

    srcs = {m: source(m) for m in SOURCE_SIZES}
    sids = {m: store.add(srcs[m]) for m in SOURCE_SIZES}
    yield dict(store=store, tids=tids, targets=tg, srcs=srcs, sids=sids)
    store.close()


def run(capi, world, m, mode, ransac, icp):
    r = capi.Registrar(store=world["store"])
    r.set_option(capi.REG_OPT_NN_MODE, mode)
    if m < 3:
        # A source of fewer than three points is never registered -- a batch runs no pass for it -- so it is searched through
        # gloc_reg_nn: one cold pass against a temporary target, in kd order with its table (the case with RANSAC) or in
        # curve order (the case without).
        r.set_option(capi.REG_OPT_TEMP_TARGET_INDEX, 1 if ransac else 0)
        corr = [r.nn(world["srcs"][m], t) for t in world["targets"]]
        r.close()
        return corr
    r.batch_ids(world["sids"][m], world["tids"], params=capi.default_reg_params(ransac_iters=ransac, icp_iters=icp))
    corr = [r.debug_corr(j, m) for j in range(len(world["tids"]))]
    r.close()
    return corr


_nearest = {}


def nearest(world, m, j):
    """Distance of every finite source of size-m's scan to target j, float64, computed once."""
    if (m, j) not in _nearest:
        s = world["srcs"][m]
        s = s[np.isfinite(s).all(1)].astype(np.float64)
        t = world["targets"][j].astype(np.float64)
        _nearest[(m, j)] = np.concatenate([np.sqrt(((s[a:a + 256, None] - t[None]) ** 2).sum(2).min(1)) for a in range(0, len(s), 256)])
    return _nearest[(m, j)]


@pytest.mark.parametrize("ransac,icp", [(64, 0), (0, 1)], ids=["pairs_pass", "first_icp_pass"])
@pytest.mark.parametrize("m", SOURCE_SIZES)
def test_cold_pass_equals_the_brute_force_kernel(capi, world, m, ransac, icp):
    got = run(capi, world, m, capi.REG_NN_CULLED, ransac, icp)
    want = run(capi, world, m, capi.REG_NN_EXHAUSTIVE, ransac, icp)
    fin = np.isfinite(world["srcs"][m]).all(1)
    for j, t in enumerate(world["targets"]):
        assert (got[j][0] == want[j][0]).all(), (m, j)
        assert (bits(got[j][1]) == bits(want[j][1])).all(), (m, j)
        # (and the brute-force kernel itself against numpy, in float64: the neighbour is a nearest one)
        assert (want[j][0][fin] < len(t)).all(), (m, j)
        s64, t64 = world["srcs"][m][fin].astype(np.float64), t.astype(np.float64)
        near = np.linalg.norm(s64 - t64[want[j][0][fin].astype(np.int64)], axis=1)
        assert (near <= nearest(world, m, j) * (1 + 1e-6) + 1e-9).all(), (m, j)


def test_cold_pass_through_the_small_queue_library():
    """The same cases through lib/libgloc3d_smallq.so (every queued item evaluated before every test step)."""
    if not os.path.exists(VARIANT):
        pytest.fail("gloc3d_amd/lib/libgloc3d_smallq.so is missing: run __graft_entry__.build() (gloc3d_amd.build.build_test_variant)")
    env = dict(os.environ, GLOC3D_LIB_PATH=VARIANT)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "brute_force",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-1500:]
    assert r.returncode == 0, tail
    assert "10 passed" in r.stdout, tail
