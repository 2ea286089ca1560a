"""gloc_reg_profile on a registration batch whose time line is stamped on the device (Profiler::open_stamps): no event
lies between the batch's kernels, the first work-group of every scope's first kernel leaves the device clock in the scope's
slot, and the slots come down with the states.  The families, their launch counts and what a time means are what the
event profiler gave (tests/test_reg_profile_gpu.py), and profiling changes no bit of a result.

The counts, from the structure of a batch: one "nn" per 1-NN pass -- RANSAC's pairs pass, if there is one, and the ICP
passes -- the first of them also "nn_cold"; one "solve" behind every ICP pass and one for RANSAC's refit, whose moments are
the one "accum" -- in the exhaustive mode (REG_NN_EXHAUSTIVE) every ICP pass has an "accum" of its own between its search and
its solve; and one "ransac_hyp" and one "ransac_score" per phase of the adaptive rule, whose phases end at 16, at 64 and at the
cap: a cap of 64 hypotheses has the phases [0, 16) and [16, 64) -- two.  (A first phase [0, 8) was built and measured with this
profiler and not kept -- alone it gained nothing at the step, LAB_NOTES.md -- so the count is not the three it would have made.)"""
import threading
import time

import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu

ICP = 5
PHASE_ENDS = (16, 64)  # of the adaptive rule (enqueue_ransac); a last phase ends at the cap


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 15, (n, 3))
    p[: n // 2, 2] = 0.0  # a floor under a box of points
    return p.astype(np.float32)


def clouds(n_jobs):
    tgt = cloud(3000, 1)
    q = (tgt[::2] + np.float32([0.2, -0.1, 0.03])).astype(np.float32)
    base = [tgt, np.ascontiguousarray(tgt[1::2]), cloud(2500, 2)]
    cands = [base[i] if i < 3 else cloud(2500 + 10 * i, 10 + i) if i % 3 == 2 else np.ascontiguousarray(tgt[i % 5 :: 2]) for i in range(n_jobs)]
    return q, cands


def expected(ransac, icp=ICP, exhaustive=False):
    passes = icp + (1 if ransac else 0)
    want = {"nn": passes, "nn_cold": 1, "solve": passes}
    if ransac:
        phases = len([e for e in PHASE_ENDS if e < ransac]) + 1  # the phases that end below the cap, and the one that ends at it
        want.update({"accum": 1, "ransac_hyp": phases, "ransac_score": phases})
    if exhaustive:
        want["accum"] = want.get("accum", 0) + icp
    return want


def check_figures(got, want, wall_ms, times=1):
    for k, n in want.items():
        assert got[k][1] == n * times, (k, got, n, times)
        assert got[k][0] > 0.0, (k, got)
    assert got["nn_cold"][0] < got["nn"][0], got
    assert sum(ms for k, (ms, _) in got.items() if k != "nn_cold") <= wall_ms, (got, wall_ms)  # (nn_cold lies inside nn)


def same_bits(a, b):
    return ((bits(a["T"]) == bits(b["T"])).all() and (bits(a["rmse"]) == bits(b["rmse"])).all()
            and (a["inliers"] == b["inliers"]).all() and (a["ok"] == b["ok"]).all())


@pytest.mark.parametrize("ransac", (64, 0))
@pytest.mark.parametrize("n_jobs", (3, 52))
def test_counts_times_and_bits_of_a_stamped_batch(capi, n_jobs, ransac):
    q, cands = clouds(n_jobs)
    prm = capi.default_reg_params(ransac_iters=ransac, icp_iters=ICP, seed=7)
    r = capi.Registrar()
    plain = r.batch(q, cands, params=prm)  # profiling off (and the first call: code objects, workspaces)
    r.set_option(capi.REG_OPT_PROFILE, 1)
    want = expected(ransac)
    if ransac:
        assert want["ransac_hyp"] == 2
    for _ in range(2):  # twice on one handle: after the reset the second batch's figures hold nothing of the first's
        r.profile_reset()
        t0 = time.perf_counter()
        out = r.batch(q, cands, params=prm)
        wall_ms = (time.perf_counter() - t0) * 1e3
        assert same_bits(out, plain)
        check_figures({k: r.profile(k) for k in want}, want, wall_ms)
    # without a reset the figures add up
    out = r.batch(q, cands, params=prm)
    assert same_bits(out, plain)
    assert {k: r.profile(k)[1] for k in want} == {k: 2 * n for k, n in want.items()}
    r.set_option(capi.REG_OPT_PROFILE, 0)
    assert same_bits(r.batch(q, cands, params=prm), plain)
    assert {k: r.profile(k)[1] for k in want} == {k: 2 * n for k, n in want.items()}  # (an unprofiled batch adds nothing)
    r.close()


@pytest.mark.parametrize("mode", ("exhaustive", "culled"))
@pytest.mark.parametrize("ransac,icp", ((64, 20), (0, 20), (300, 40), (0, 17)))
def test_many_passes_in_either_search_mode_all_have_their_slot(capi, mode, ransac, icp):
    """The time line has a slot for every scope the batch opens, however many passes: three scopes per ICP pass in the
    exhaustive mode (search, accum, solve), two in the culled one.  A scope without a slot would be counted with no time
    and the family of the last slot would take it: here every family's time, divided by its launches, must be that of a
    short batch of the same kind (5 passes) to within a factor of two, besides the counts and the wall time."""
    q, cands = clouds(3)
    r = capi.Registrar()
    r.set_option(capi.REG_OPT_NN_MODE, capi.REG_NN_EXHAUSTIVE if mode == "exhaustive" else capi.REG_NN_CULLED)
    r.set_option(capi.REG_OPT_PROFILE, 1)
    per_launch = {}
    for n in (min(icp, 5), icp):
        prm = capi.default_reg_params(ransac_iters=ransac, icp_iters=n, seed=7)
        want = expected(ransac, n, mode == "exhaustive")
        r.batch(q, cands, params=prm)  # (code objects, workspaces)
        r.profile_reset()
        t0 = time.perf_counter()
        r.batch(q, cands, params=prm)
        wall_ms = (time.perf_counter() - t0) * 1e3
        got = {k: r.profile(k) for k in want}
        check_figures(got, want, wall_ms)
        per_launch[n] = {k: (got[k][0] - (got["nn_cold"][0] if k == "nn" else 0.0)) / max(got[k][1] - (1 if k == "nn" else 0), 1) for k in ("nn", "solve")}
    short, long_ = per_launch[min(icp, 5)], per_launch[icp]
    for k in short:
        assert 0.5 * short[k] < long_[k] < 2.0 * short[k], (k, per_launch)
    r.close()


def test_two_handles_profiling_at_once_keep_their_own_counts(capi):
    q, cands = clouds(3)
    runs = {64: 3, 0: 2}  # ransac -> batches
    regs = {}
    for ransac in runs:
        regs[ransac] = capi.Registrar()
        regs[ransac].batch(q, cands, params=capi.default_reg_params(ransac_iters=ransac, icp_iters=ICP, seed=7))
        regs[ransac].set_option(capi.REG_OPT_PROFILE, 1)
    errors = []

    def work(ransac):
        try:
            prm = capi.default_reg_params(ransac_iters=ransac, icp_iters=ICP, seed=7)
            for _ in range(runs[ransac]):
                regs[ransac].batch(q, cands, params=prm)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(ransac,)) for ransac in runs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for ransac, times in runs.items():
        want = expected(ransac)
        got = {k: regs[ransac].profile(k) for k in want}
        for k, n in want.items():
            assert got[k][1] == n * times and got[k][0] > 0.0, (ransac, k, got[k])
        if not ransac:
            assert regs[ransac].profile("ransac_score") == (0.0, 0)
        regs[ransac].close()


@pytest.mark.parametrize("ransac", (64, 0))
def test_a_batch_on_the_callers_stream_through_begin_and_end(capi, ransac):
    import torch
    q, cands = clouds(3)
    store = capi.ScanStore()
    qid = store.add(q)
    cids = np.array([[store.add(c) for c in cands]], np.uint32)
    prm = capi.default_reg_params(ransac_iters=ransac, icp_iters=ICP, seed=7)
    r = capi.Registrar(store=store)
    plain = r.batch_multi([qid], cids, params=prm)
    stream = torch.cuda.Stream()
    r.set_stream(stream.cuda_stream)
    r.set_option(capi.REG_OPT_PROFILE, 1)
    want = expected(ransac)
    for _ in range(2):
        r.profile_reset()
        t0 = time.perf_counter()
        r.batch_multi_begin([qid], cids, params=prm)
        out = r.batch_multi_end()
        wall_ms = (time.perf_counter() - t0) * 1e3
        assert same_bits(out, plain)
        check_figures({k: r.profile(k) for k in want}, want, wall_ms)
    # the figures asked for while the batch is in flight: the profile waits for the stream and holds the whole batch
    r.profile_reset()
    r.batch_multi_begin([qid], cids, params=prm)
    assert r.profile("nn")[1] == want["nn"]
    assert same_bits(r.batch_multi_end(), plain)
    assert {k: r.profile(k)[1] for k in want} == want
    r.set_stream(None)
    r.close()
    store.close()
