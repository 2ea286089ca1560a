"""GPU: the cold 1-NN pass of a batch WITHOUT a split plan -- what a large batch runs first -- is a kernel of its own at two
sources per lane (nn_compact_cold_kernel<PAIRS>: the cold search held to the registers of six waves per SIMD).  A small batch
reaches it with the split plan switched off.  Both instantiations -- the pairs pass in front of RANSAC and the first ICP pass
without it -- against the brute-force kernel: correspondences and squared distances equal bit for bit.  Targets of 17 points
(two kd leaves, one nearly empty), 2 049 and 5 000; sources of 129 and 3 000 points with target points themselves, far points
and non-finite points among them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TARGET_SIZES = (17, 2049, 5000)
SOURCE_SIZES = (129, 3000)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def world(capi):
    rng = np.random.default_rng(11)
    store = capi.ScanStore()
    tg = [np.ascontiguousarray((rng.uniform(-1, 1, (n, 3)) * (6.0, 4.5, 0.75)).astype(np.float32)) for n in TARGET_SIZES]
    tids = [store.add(t) for t in tg]
    store.build_target_index_batch(tids)
    allp = np.concatenate(tg)
    srcs = {}
    for m in SOURCE_SIZES:
        s = allp[rng.integers(0, len(allp), m)] + rng.normal(0, 0.05, (m, 3)).astype(np.float32)
        s[1::5] = allp[rng.integers(0, len(allp), len(s[1::5]))]                      # target points themselves
        s[3::17] = (rng.choice([-1.0, 1.0], (len(s[3::17]), 3)) * rng.uniform(50, 5000, (len(s[3::17]), 3))).astype(np.float32)
        s[5, 0], s[12, 1], s[19, 2] = np.nan, np.inf, -np.inf
        s[40] = np.nan
        srcs[m] = np.ascontiguousarray(s.astype(np.float32))
    sids = {m: store.add(srcs[m]) for m in SOURCE_SIZES}
    yield dict(store=store, tids=tids, sids=sids)
    store.close()


def run(capi, world, m, mode, ransac, icp):
    r = capi.Registrar(store=world["store"])
    r.set_option(capi.REG_OPT_NN_MODE, mode)
    r.set_option(capi.REG_OPT_NN_SPLIT_HELPERS, 0)
    r.batch_ids(world["sids"][m], world["tids"], params=capi.default_reg_params(ransac_iters=ransac, icp_iters=icp))
    corr = [r.debug_corr(j, m) for j in range(len(world["tids"]))]
    r.close()
    return corr


@pytest.mark.parametrize("ransac,icp", [(64, 0), (0, 1)], ids=["pairs_pass", "first_icp_pass"])
@pytest.mark.parametrize("m", SOURCE_SIZES)
def test_cold_pass_without_a_split_plan_equals_the_brute_force_kernel(capi, world, m, ransac, icp):
    got = run(capi, world, m, capi.REG_NN_CULLED, ransac, icp)
    want = run(capi, world, m, capi.REG_NN_EXHAUSTIVE, ransac, icp)
    for j in range(len(world["tids"])):
        assert (got[j][0] == want[j][0]).all(), (m, j)
        assert (bits(got[j][1]) == bits(want[j][1])).all(), (m, j)
