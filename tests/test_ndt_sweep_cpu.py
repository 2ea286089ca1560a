"""CPU: the alignment cases of tests/ndt_cases.py judged by the float64 restatement alone, before any of them is held
against the device (tests/test_ndt_sweep_gpu.py): at least 90 % of the cases are stable under a second summation order,
and the stable ones between them take every branch of the Newton / More-Thuente loop that ndt_ref.EVENTS names.

Three events are exempt, because no input reaches them:
  * trial_case_4 -- with finite values PCL's loop never gets there.  A selection follows either the first trial (I is
    the point 0 on both sides: psi_t > 0 is case 1; psi_t <= 0 keeps the loop going only with dphi_t > 0, which is case
    2), or update_interval's outcome 1 (a_l unchanged and f_t > f_l: case 1 again), or its outcomes 2 / 3, which move
    a_l to the trial itself, so that a_t == a_l, f_t == f_l, g_t == g_l: case 3 in its degenerate form (NaN
    interpolants, the bound a_t + 0.66 (a_u - a_t) returned).  Case 4 needs f_t <= f_l and |g_t| > |g_l|.
  * dphi0_zero and end_nan_step -- a direction exactly orthogonal to the gradient, and a NaN Newton step, which finite
    cells and points do not produce.
trial_clamped_max is reached only where step_min = trans_eps / 2 exceeds step_size (0.02 with 0.2, both values the sweep
is asked to cover): between the bounds every selection interpolates inside [0, first trial] <= step_size.

The end pose cannot see everything: trial-value case 4 is never taken, and the `+ mu * dphi_0` of the open -> closed
switch moves a slope by 1e-4 of itself, inside the 1e-3 m the device is held to.  So the scalar pieces of the line search
in csrc/ndt_kernels.hpp (plain fp64, built for the host as well) are also held to the restatement's bit for bit on
hand-made inputs, through gloc_ndt_debug_line_search -- no device needed.

Run time: about 70 s on one core (two ndt_ref.align runs per case, N_AZ = 200)."""
import ctypes as C

import numpy as np

import ndt_cases as NC
import ndt_ref as R

UNREACHABLE = ("trial_case_4", "dphi0_zero", "end_nan_step")


def test_cases_span_the_issue_grid():
    names = [c["name"] for c in NC.CASES]
    assert len(set(names)) == len(names) >= 30
    assert {c["world"] for c in NC.CASES} >= set(NC.WORLDS)                   # three synth seeds
    grid = dict(step_size={0.02, 0.1, 1.0}, trans_eps={0.001, 0.01, 0.2}, max_iters={1, 3, 35},
                resolution={0.5, 1.0, 2.0}, outlier_ratio={0.2, 0.55})
    for k, want in grid.items():
        assert {NC.ref_params(c["params"])[k] for c in NC.CASES} >= {NC.ref_params({k: v})[k] for v in want}, k
    off = np.array([np.linalg.norm(c["off"][1]) for c in NC.CASES if c["name"] != "a_out_of_reach"])
    assert off.min() <= 0.051 and off.max() >= 1.45
    yaw = np.array([abs(c["off"][0]) for c in NC.CASES])
    assert (yaw <= 0.5).any() and ((yaw >= 11.9) & (yaw < 90)).any() and (yaw > 160).sum() >= 3
    assert sum(1 for c in NC.CASES if c["off"][2] or c["off"][3]) >= 5       # roll / pitch


def test_most_cases_are_stable_and_every_branch_is_taken():
    refs = NC.references()
    stable = [c["name"] for c in NC.CASES if refs[c["name"]]["stable"]]
    unstable = [c["name"] for c in NC.CASES if not refs[c["name"]]["stable"]]
    share = len(stable) / len(NC.CASES)
    print("\nstable: %d of %d cases (%.1f %%); unstable: %s" % (len(stable), len(NC.CASES), 100 * share, unstable or "none"))
    hits = {e: sum(1 for n in stable if e in refs[n]["events"]) for e in R.EVENTS}
    print("%-22s %s" % ("event", "stable cases that take it"))
    for e in R.EVENTS:
        print("%-22s %d%s" % (e, hits[e], "   (unreachable, see the module docstring)" if e in UNREACHABLE else ""))
    assert share >= 0.9
    for e in R.EVENTS:
        if e in UNREACHABLE:
            assert hits[e] == 0, e          # (if one of them is ever taken, the docstring's argument is wrong: look)
        else:
            assert hits[e] >= 1, e
    # the exits the device is held to exactly
    capped = [n for n in stable if "end_iteration_cap" in refs[n]["events"]]
    assert all(not refs[n]["ref"]["converged"] for n in capped)
    assert {refs[n]["ref"]["iters"] for n in capped} >= {3, 5}                # max_iters 1 and 3: max_iters + 2 iterations
    assert refs["a_out_of_reach"]["ref"]["iters"] == 0 and refs["a_out_of_reach"]["ref"]["prob"] == 0.0


def test_recording_events_changes_nothing():
    c = NC.CASES[0]
    prm = NC.ref_params(c["params"])
    x = NC.filtered(c["world"], c["src"], prm["source_leaf"])
    cells = NC.cells(c["world"], c["tgt"], prm["resolution"], prm["min_points_per_cell"], prm["min_covar_eigvalue_mult"])
    a = R.align(x, cells, init_T=NC.guess(c), params=prm)
    b = NC.references()[c["name"]]["ref"]
    assert (a["T"] == b["T"]).all() and a["iters"] == b["iters"] and a["prob"] == b["prob"] and a["evals"] == b["evals"]


# ---- the header's line-search pieces on the host, bit for bit ---------------------------------------------------------
def _host(capi, op, I, x):
    f = capi.lib().gloc_ndt_debug_line_search
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    I = np.array(I, np.float64)
    x, out = np.array(x, np.float64), np.zeros(1, np.float64)
    assert f(op, I.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    return out[0], I


def _same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _line_search_inputs():
    """(I, a_t, f_t, g_t) as np.float64: random intervals and trials, and the shapes the loop produces -- the trial
    equal to a_l in position, value and slope (after update_interval's outcomes 2 and 3), ties and zeros."""
    rng = np.random.default_rng(5)
    rows = []
    for _ in range(4000):
        I = rng.normal(size=6) * rng.choice([0.01, 1.0, 30.0])
        I[0], I[3] = abs(I[0]), abs(I[3])
        t = rng.normal(size=3) * rng.choice([0.01, 1.0, 30.0])
        t[0] = abs(t[0])
        kind = rng.integers(0, 8)
        if kind == 0:
            t = I[0:3].copy()                        # a_t == a_l, f_t == f_l, g_t == g_l
        elif kind == 1:
            t[1] = I[1] - abs(t[1])                  # f_t <= f_l: cases 2 - 4
            t[2] = np.sign(I[2]) * abs(t[2])         # same sign of slope: cases 3 and 4
        elif kind == 2:
            t[0] = I[0]                              # g_t (a_l - a_t) == 0: the interval has converged
            t[1] = I[1] - abs(t[1])
        elif kind == 3:
            t[2] = 0.0
        rows.append((np.float64(I), np.float64(t[0]), np.float64(t[1]), np.float64(t[2])))
    return rows


def test_header_line_search_pieces_equal_the_restatement_bit_for_bit(capi):
    tv, ui = {}, {}
    for I, a_t, f_t, g_t in _line_search_inputs():
        ev = []
        want = R.trial_value(*I, a_t, f_t, g_t, events=ev)
        got, I_after = _host(capi, 0, I, [a_t, f_t, g_t])
        assert _same_bits(got, want) and _same_bits(I_after, I), (ev, I, a_t, f_t, g_t, got, want)
        tv[ev[0]] = tv.get(ev[0], 0) + 1
        ev, I_ref = [], [np.float64(v) for v in I]
        want = R.update_interval(I_ref, a_t, f_t, g_t, events=ev)
        got, I_after = _host(capi, 1, I, [a_t, f_t, g_t])
        assert bool(got) == want and _same_bits(I_after, I_ref), (ev, I, a_t, f_t, g_t)
        ui[ev[0]] = ui.get(ev[0], 0) + 1
        # the open -> closed switch, as ndt_ref.align states it (mu = 1e-4; phi_0, dphi_0 taken from the trial's numbers)
        mu, phi_0, dphi_0 = 1e-4, f_t, -abs(g_t)
        J = [np.float64(v) for v in I]
        J[1] = J[1] + phi_0 - mu * dphi_0 * J[0]
        J[2] = J[2] + mu * dphi_0
        J[4] = J[4] + phi_0 - mu * dphi_0 * J[3]
        J[5] = J[5] + mu * dphi_0
        _, I_after = _host(capi, 2, I, [phi_0, dphi_0, mu])
        assert _same_bits(I_after, J)
        assert not _same_bits(I_after[[2, 5]], I[[2, 5]]) or dphi_0 == 0
    print("\ntrial_value cases:", tv, "\nupdate_interval outcomes:", ui)
    assert all(tv.get("trial_case_%d" % k, 0) >= 100 for k in (1, 2, 3, 4)), tv
    assert all(ui.get(k, 0) >= 100 for k in ("interval_case_1", "interval_case_2", "interval_case_3", "interval_converged")), ui
    # the clamp: max(min(a, step_max), step_min), NaN stays NaN, step_min wins where it exceeds step_max
    for a, lo, hi in ((0.5, 0.005, 0.1), (0.001, 0.005, 0.1), (0.05, 0.005, 0.1), (np.nan, 0.005, 0.1), (0.05, 0.1, 0.02),
                      (0.5, 0.1, 0.02), (-1.0, 0.0, 0.1), (np.inf, 0.005, 0.1)):
        got, _ = _host(capi, 3, np.zeros(6), [a, lo, hi])
        assert _same_bits(got, max(min(a, hi), lo)), (a, lo, hi, got)
