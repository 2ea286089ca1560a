"""CPU: proof that the NetVLAD-FC case table (vlad_cases.py) can fail -- its tolerances come from the reference's own
float32 error, stay inside the suite's old 2e-5, and every mutant of vlad_ref.py moves the float64 result by at
least ten times the tolerance of the cases it applies to.  No GPU, no kernel output anywhere in this file."""
import numpy as np
import pytest

import vlad_cases as T
import vlad_ref as R
from test_oracle_vlad import CASES as GOLDENS, load, load_gating


def _have(attr):
    return {attr(c) for c in T.CASES}


def test_table_has_the_shapes_the_kernels_branch_on():
    assert _have(lambda c: c.K) >= {1, 15, 16, 17, 33, 48, 49, 63, 64}
    assert _have(lambda c: c.C) >= {1, 3, 15, 16, 17, 127, 128, 129, 130, 257, 512}
    assert _have(lambda c: (c.K, c.C)) >= {(64, 557), (48, 560)}
    assert _have(lambda c: c.H * c.W) >= {1, 63, 64, 65, 72, 128, 130}
    assert _have(lambda c: c.n) >= {1, 7, 8, 9, 16, 17}
    assert _have(lambda c: c.out) >= {1, 3, 255, 256, 257, 300}
    assert _have(lambda c: c.K * c.C) >= {6, 512, 513, 1024, 2400}
    assert sum("nonorm" in c.flags for c in T.CASES) >= 3 and any("x30" in c.flags for c in T.CASES)
    assert {c.bias for c in T.CASES if c.flags == "zero_img"} == {False, True}
    assert any("zero_cent" in c.flags and "zero_img" in c.flags for c in T.CASES)
    assert _have(lambda c: (c.n, c.K, c.C, c.H, c.W, c.out)) >= {(1, 64, 512, 48, 48, 512), (2, 64, 128, 8, 24, 128)}
    gated = [c for c in T.CASES if "gate" in c.flags]
    assert {c.out for c in gated} >= {1, 63, 64, 65, 130, 512} and {c.n for c in gated} == {1, 9}
    assert all(c.branch for c in T.CASES)
    assert T.BY_NAME[T.PRODUCTION].bias           # mutant 4 has to be caught there


def test_selection_fc_is_indexing():
    rng = np.random.default_rng(3)
    for K, C in ((3, 5), (27, 19), (64, 512), (64, 557)):
        rows = R.rows_of_interest(K, C)
        assert len(rows) <= 4096 and rows[0] == 0 and rows[-1] == K * C - 1 and (np.diff(rows) > 0).all()
        if K * C > 4096:
            for lo in list(range(0, K * C, C)) + list(range(0, K * C, R.SLAB)):
                assert lo in rows and lo + 1 in rows
            for hi in [k * C + C for k in range(K)] + [min(j + R.SLAB, K * C) for j in range(0, K * C, R.SLAB)]:
                assert hi - 1 in rows and hi - 2 in rows
        fc = R.selection_fc(K, C, rows)
        assert fc.shape == (K * C, len(rows)) and (fc.sum(axis=0) == 1).all() and fc.sum() == len(rows)
        v = rng.standard_normal((2, K * C))
        assert (v @ fc.astype(np.float64) == v[:, rows]).all()      # what head64(rows=...) relies on


def test_zero_image_with_zero_centroids_is_exactly_zero():
    case = next(c for c in T.CASES if "zero_cent" in c.flags)
    for kind in T.KINDS:
        ref = T.bounds(case)[kind].ref
        assert (ref[1] == 0.0).all() and np.abs(ref[0]).max() > 0 and np.isfinite(ref).all()


def test_tolerances_come_from_the_reference_and_stay_inside_the_old_bound():
    bad = []
    print("\ncase kind  |oracle32-f64| |ordered32-f64| 2^-23max|f64|  tol  max|f64|")
    for case in T.CASES:
        for kind in T.KINDS:
            b = T.bounds(case)[kind]
            mx = float(np.abs(b.ref).max())
            print(f"{case.name:14s} {kind:9s} {b.d_oracle:.2e} {b.d_ordered:.2e} {b.ulp:.2e} {b.tol:.2e} {mx:.3f}")
            assert np.isfinite(b.ref).all()
            if not b.tol == 4.0 * max(b.d_oracle, b.d_ordered, b.ulp):
                bad.append((case.name, kind, "tolerance is not the stated formula"))
            if not b.d_oracle <= b.tol / 4:            # conditioning: the reference alone stays inside the bound
                bad.append((case.name, kind, "oracle32 outside tol / 4"))
            if not b.tol <= 2e-5 * max(1.0, mx):       # the new bound never exceeds the suite's old one
                bad.append((case.name, kind, f"tol {b.tol:.2e} above the old 2e-5 bound"))
    assert not bad, bad


def test_every_mutant_moves_every_case_it_applies_to():
    caught = {m: [] for m in R.MUTANTS}
    missed = []
    print("\ncase: mutant -> move / tol (kind), the larger of the two kinds")
    for case in T.CASES:
        b = T.bounds(case)
        line = []
        for m in R.MUTANTS:
            if not T.applies(case, m):
                continue
            mut = T.reference64(case, m)
            ratio, kind = max((float(np.abs(mut[k] - b[k].ref).max()) / b[k].tol, k) for k in T.KINDS)
            line.append(f"{m}:{ratio:.0f}({kind[0]})")
            (caught[m].append(case.name) if ratio >= 10.0 else missed.append((case.name, m, kind, ratio)))
        print(f"{case.name:14s} " + " ".join(line))
    print("\ncatch counts per mutant:")
    for m, names in caught.items():
        print(f"  {m} {R.MUTANTS[m]}: {len(names)} cases")
    assert not missed, missed
    assert all(len(v) >= 3 for v in caught.values()), {m: len(v) for m, v in caught.items()}
    assert T.PRODUCTION in caught[R.M_LAST_CHANNEL] and T.PRODUCTION in caught[R.M_NO_BIAS]


@pytest.mark.parametrize("golden", GOLDENS)
def test_float64_reference_agrees_with_the_oracle_on_the_goldens(golden):
    from oracle import vlad_oracle
    x, w, b, c, fc, y = load(golden)
    gate = load_gating(golden)
    got32 = vlad_oracle.netvlad_fc_forward(x, w, b, c, fc)
    if gate is not None:
        got32 = vlad_oracle.gating_forward(got32, *gate)
    got64 = R.forward64(x, w, b, c, fc, True, gate)
    lim = 2e-6 * max(1.0, np.abs(y).max())
    assert np.abs(got32 - got64).max() < lim and np.abs(got64 - y).max() < lim
    assert np.abs(R.forward32_ordered(x, w, b, c, fc, True, gate) - got64).max() < lim
