"""A warm pass of the culled search writes its distances only where they are read: launch by launch, every warm moments
pass but a batch's last leaves `d2` alone (launch_nn's keep_d2).  What gloc_reg_debug_corr brings down after a culled
batch of 1, 2 and 5 ICP passes -- the last pass's matches and distances -- must be those of the exhaustive mode, which
writes them in every pass, bit for bit: a batch above the chaining limit (52 jobs: one launch per pass), a small batch
whose passes are chained, and with the RANSAC stage in front."""
import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 15, (n, 3))
    p[: n // 2, 2] = 0.0  # a floor under a box of points
    return p.astype(np.float32)


@pytest.fixture(scope="module")
def world(capi):
    store = capi.ScanStore()
    tgt = cloud(3000, 1)
    q = (tgt[::2] + np.float32([0.2, -0.1, 0.03])).astype(np.float32)
    cands = [tgt, np.ascontiguousarray(tgt[1::2]), cloud(2500, 2)]
    cands += [cloud(2500 + 10 * i, 10 + i) if i % 3 == 2 else np.ascontiguousarray(tgt[i % 5 :: 2]) for i in range(3, 52)]
    qid = store.add(q)
    cids = [store.add(c) for c in cands]
    yield store, qid, cids, len(q)
    store.close()


@pytest.mark.parametrize("ransac", (0, 64))
@pytest.mark.parametrize("n_jobs", (3, 52))
def test_debug_corr_after_a_culled_batch_equals_the_exhaustive_modes(capi, world, n_jobs, ransac):
    store, qid, cids, n_src = world
    for icp in (1, 2, 5):
        prm = capi.default_reg_params(ransac_iters=ransac, icp_iters=icp, seed=7)
        r = capi.Registrar(store=store)  # (culled: the default)
        r.batch_ids(qid, cids[:n_jobs], params=prm)
        culled = [r.debug_corr(j, n_src) for j in range(n_jobs)]
        # the pose the culled run's last pass searched at: what the same run leaves after one pass fewer (None: the identity)
        T_prev = None
        if icp > 1 or ransac:
            T_prev = r.batch_ids(qid, cids[:n_jobs], params=capi.default_reg_params(ransac_iters=ransac, icp_iters=icp - 1, seed=7))["T"]
        r.close()
        # ... and the exhaustive kernel's single pass from there
        r = capi.Registrar(store=store)
        r.set_option(capi.REG_OPT_NN_MODE, capi.REG_NN_EXHAUSTIVE)
        r.batch_ids(qid, cids[:n_jobs], init_T=T_prev, params=capi.default_reg_params(ransac_iters=0, icp_iters=1))
        exhaustive = [r.debug_corr(j, n_src) for j in range(n_jobs)]
        r.close()
        for j in range(n_jobs):
            a, b = culled[j], exhaustive[j]
            assert (a[0] == b[0]).all(), (icp, j)
            assert (bits(a[1]) == bits(b[1])).all(), (icp, j)
