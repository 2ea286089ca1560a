"""gloc_reg_profile on a profiled batch: the families and their launch counts are what they were before spans began to share
events (a scope that starts where another ended takes that scope's end event as its start; "nn_cold" is counted on "nn"'s two
events) -- one "nn" per pass, the batch's first pass also as "nn_cold", a "solve" for the refit and one per ICP pass -- every
time is positive, and together they fit into the wall time of the call that ran them."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ICP = 5


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 15, (n, 3))
    p[: n // 2, 2] = 0.0  # a floor under a box of points
    return p.astype(np.float32)


@pytest.mark.parametrize("ransac", (64, 0))
def test_families_launches_and_times_of_one_batch(capi, ransac):
    tgt = cloud(3000, 1)
    q = (tgt[::2] + np.float32([0.2, -0.1, 0.03])).astype(np.float32)
    cands = [tgt, np.ascontiguousarray(tgt[1::2]), cloud(2500, 2)]
    r = capi.Registrar()
    r.set_option(capi.REG_OPT_PROFILE, 1)
    prm = capi.default_reg_params(ransac_iters=ransac, icp_iters=ICP, seed=7)
    ref = r.batch(q, cands, params=prm)  # (first call: code objects, workspaces)
    r.profile_reset()
    t0 = time.perf_counter()
    out = r.batch(q, cands, params=prm)
    wall_ms = (time.perf_counter() - t0) * 1e3
    assert (out["T"].view(np.uint32) == ref["T"].view(np.uint32)).all()
    passes = ICP + (1 if ransac else 0)
    want = {"nn": passes, "nn_cold": 1, "solve": passes}
    if ransac:
        want.update({"accum": 1, "ransac_hyp": 2, "ransac_score": 2})  # (phases [0, 16) and [16, 64) of the adaptive rule)
    got = {k: r.profile(k) for k in want}
    for k, n in want.items():
        print(k, got[k])
        assert got[k][1] == n, (k, got[k], n)
        assert got[k][0] > 0.0, (k, got[k])
    assert got["nn_cold"][0] < got["nn"][0]
    assert got["nn"][0] + got["nn_cold"][0] + got["solve"][0] <= wall_ms, (got, wall_ms)
    assert sum(ms for k, (ms, _) in got.items() if k != "nn_cold") <= wall_ms, (got, wall_ms)  # (nn_cold lies inside nn)
    r.close()
