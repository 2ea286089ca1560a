"""The per-pass solve (solve_kernel<0>, the refit's solve_kernel<1>) sums a job's wave partials in ONE order, whoever does it:
the 16 waves of a 1024-thread work-group (a small batch, launch by launch: the planner runs beside it), the four waves of the
256-thread work-group of a batch without a split plan (each wave makes four of the 16 rows in turn), or the chained launch's 16
reducer waves (chain_reduce_solve).  One job, run

  alone                      -> the chained launch,
  as one of 49 copies        -> launch by launch, 1024-thread work-groups,
  alone with the profiler on -> launch by launch, 1024-thread work-groups, events between the launches,
  as one of 49 copies with the split plan off -> launch by launch, 256-thread work-groups (what a large batch runs),

must give the same pose, rmse, inlier count, verdict and final step in every bit.  Source sizes: 1, 63, 64, 65, 1023, 1024
and 1025 source groups of 128 points -- the edges of a row (64 partials), of a turn of all rows (1024) and one beyond.  With
and without RANSAC (the refit's solve); a job with fewer than three sources (frozen) and one with an empty target ride along in
a batch of their own.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GROUPS = (1, 63, 64, 65, 1023, 1024, 1025)
GROUP_POINTS = 128  # two sources per lane
COPIES = 49         # the smallest batch that does not chain
ICP = 3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def room(n, seed):
    """n points on a floor and two walls of a 20 m x 16 m room, 2 cm of noise."""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, 4, n)  # floor twice as likely
    u, v = rng.uniform(0, 20, n), rng.uniform(0, 16, n)
    h = rng.uniform(0, 3, n)
    p = np.stack([u, v, np.zeros(n)], 1)
    p[which == 2] = np.stack([u, np.zeros(n), h], 1)[which == 2]
    p[which == 3] = np.stack([np.zeros(n), v, h], 1)[which == 3]
    return (p + rng.normal(0, 0.02, (n, 3))).astype(np.float32)


def moved(p):
    c, s = np.cos(np.radians(2.0)), np.sin(np.radians(2.0))
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return (p.astype(np.float64) @ R.T + np.array([0.3, -0.2, 0.05])).astype(np.float32)


@pytest.fixture(scope="module")
def world(capi):
    store = capi.ScanStore()
    tgt = store.add(room(6000, 1))
    store.build_target_index_batch([tgt])
    src = {g: store.add(moved(room(g * GROUP_POINTS - 5, 100 + g))) for g in GROUPS}
    tiny = store.add(moved(room(2, 7)))
    empty = store.add(np.zeros((0, 3), np.float32))
    yield dict(store=store, tgt=tgt, src=src, tiny=tiny, empty=empty)
    store.close()


def run(capi, world, q_ids, cand_rows, ransac, profile=False, helpers=None):
    r = capi.Registrar(store=world["store"])
    if profile:
        r.set_option(capi.REG_OPT_PROFILE, 1)
    if helpers is not None:
        r.set_option(capi.REG_OPT_NN_SPLIT_HELPERS, helpers)
    prm = capi.default_reg_params(ransac_iters=ransac, icp_iters=ICP, seed=12345)
    cand = np.array(cand_rows, np.uint32)
    # (one RANSAC stream for every job: a copy draws the samples of the job it copies, wherever it sits in the batch)
    out = r.batch_multi(q_ids, cand, params=prm, stream_ids=np.zeros(cand.size, np.uint32))
    out = {k: v.reshape((-1,) + v.shape[2:]) for k, v in out.items()}
    out["steps"] = np.array(r.final_steps(cand.size), np.float32)
    chained, timed_out = r.debug_chain()
    r.close()
    assert timed_out == 0
    return out, chained


def same(a, b, ia, ib, what):
    assert (bits(a["T"][ia]) == bits(b["T"][ib])).all(), what
    assert (bits(a["rmse"][ia]) == bits(b["rmse"][ib])).all(), what
    assert (bits(a["steps"][ia]) == bits(b["steps"][ib])).all(), what
    assert (a["inliers"][ia] == b["inliers"][ib]).all() and (a["ok"][ia] == b["ok"][ib]).all(), what


@pytest.mark.parametrize("ransac", (0, 64))
@pytest.mark.parametrize("groups", GROUPS)
def test_one_job_four_ways(capi, world, groups, ransac):
    q, t = world["src"][groups], world["tgt"]
    alone, chained = run(capi, world, [q], [[t]], ransac)
    assert chained == 1, "one job alone runs its warm passes as one launch"
    assert np.isfinite(alone["T"]).all() and np.isfinite(alone["steps"]).all()
    for how, kw, n in (("49 copies", {}, COPIES), ("profiler on", dict(profile=True), 1), ("49 copies, no split plan", dict(helpers=0), COPIES)):
        out, chained = run(capi, world, [q], [[t] * n], ransac, **kw)
        assert chained == 0, how
        for j in range(n):
            same(out, alone, j, 0, (groups, ransac, how, j))


@pytest.mark.parametrize("ransac", (0, 64))
def test_frozen_job_and_empty_target_four_ways(capi, world, ransac):
    """Jobs (real source, target), (real source, empty target), (two sources: frozen, target), (frozen, empty target) in one batch."""
    q_ids = [world["src"][65], world["tiny"]]
    pair = [world["tgt"], world["empty"]]
    alone, chained = run(capi, world, q_ids, [pair, pair], ransac)
    assert chained == 1
    eye = np.eye(4, dtype=np.float32)
    for j in (1, 2, 3):  # nothing to estimate from: the initial guess stays
        assert (alone["T"][j] == eye).all() and not alone["ok"][j], j
    assert not (alone["T"][0] == eye).all()
    wide = [pair * 13, pair * 13]  # 52 jobs
    for how, kw, rows in (("52 jobs", {}, wide), ("profiler on", dict(profile=True), [pair, pair]), ("52 jobs, no split plan", dict(helpers=0), wide)):
        out, chained = run(capi, world, q_ids, rows, ransac, **kw)
        assert chained == 0, how
        n = len(rows[0])
        for j in range(2 * n):
            same(out, alone, j, 2 * (j // n) + (j % n) % 2, (ransac, how, j))
