"""CPU: the case table of the point-to-point evaluation (tests/eval_cases.py) and its float64 restatement
(tests/eval_ref.py), proved before a device sees them: every case reaches the branch it is there for, the restatement
equals an independent statement of the same sums (scipy's kd tree for the pairs, G^T G of stacked 3 x 6 blocks for the
information matrix), and on the integer lattice it equals exact integer arithmetic."""
import numpy as np
import pytest

import eval_cases as EC
import eval_ref as E


def _ref(row, oracle_mod):
    return EC.reference(row, oracle_mod)


def test_lattice_rows_count_every_point_with_zero_residual(oracle_mod):
    assert [len(EC.cloud(r["src"])) for r in EC.rows("a")] == list(EC.SIZES) and len(EC.cloud("lat")) == 729
    for row in EC.rows("a"):
        r = _ref(row, oracle_mod)
        n = len(EC.cloud(row["src"]))
        assert r["count"] == n and r["fitness"] == 1 and r["rmse"] == 0 and r["sum"] == 0 and not r["g"].any()
        assert (r["j"] == np.arange(n)).all()                 # the sources are the lattice's first points


def test_tie_rows_are_all_ties_on_both_sides_of_the_gate(oracle_mod):
    lat = EC.cloud("lat").astype(np.float64)
    assert np.float32(EC.TIE_GATE) * np.float32(EC.TIE_GATE) == np.float32(0.25)
    assert np.float32(EC.BELOW_TIE_GATE) * np.float32(EC.BELOW_TIE_GATE) < np.float32(0.25) and EC.BELOW_TIE_GATE > 0.4999
    for row in EC.rows("b"):
        r = _ref(row, oracle_mod)
        src = EC.cloud(row["src"]).astype(np.float64)
        p = src + [0.5, 0.0, 0.0]
        d2 = ((p[:, None, :] - lat[None, :, :]) ** 2).sum(2)
        assert (d2.min(1) == 0.25).all() and ((d2 == 0.25).sum(1) == 2).all()          # every point: exactly two nearest
        first = np.argmax(d2 == 0.25, axis=1)
        assert r["count"] == len(src) and (r["j"] == first).all()                        # the smaller index wins
        left = lat[first, 0] < p[:, 0]
        assert len(src) == 1 or (left.any() and (~left).any())                           # ... on either side of p
        assert r["fitness"] == 1 and r["rmse"] == np.float32(0.5) and r["sum"] == 0.25 * len(src)
        assert r["g"][3] == 0.5 * (int(left.sum()) - int((~left).sum()))
    for row in EC.rows("b0"):
        r = _ref(row, oracle_mod)
        assert r["count"] == 0 and r["fitness"] == 0 and r["rmse"] == 0 and not r["S"].any() and not r["info"].any()


def test_scene_rows_reach_their_branches(oracle_mod):
    n_t = len(EC.cloud("t"))
    assert 6000 <= n_t <= 7000
    fit = {}
    for row in EC.rows("c"):
        r = _ref(row, oracle_mod)
        n = len(EC.cloud(row["src"]))
        assert 6000 <= n <= 7000 and r["fitness"] == np.float32(r["count"] / n)
        fit[(row["src"], row["gate"])] = r["count"]
        print(f"(c) {row['src']} gate {row['gate']:.1f}: {r['count']} of {n} pairs, rmse {r['rmse']:.4f}")
    for s in ("s1", "s2", "s3"):
        c = [fit[(s, float(np.float32(g)))] for g in EC.GATES]
        assert 1000 < c[0] < c[1] < c[2] <= len(EC.cloud(s))                             # every gate cuts somewhere else
    # (d) the non-finite rows: never counted, always in the denominator
    odd = EC.cloud("s1_odd")
    bad = ~np.isfinite(odd).all(1)
    assert bad[0] and bad[-1] and 0.009 * len(odd) <= bad.sum() <= 0.012 * len(odd)
    assert np.isnan(odd).any() and (odd == np.inf).any() and (odd == -np.inf).any()
    for row in EC.rows("d"):
        r = _ref(row, oracle_mod)
        clean = _ref(dict(row, src="s1"), oracle_mod)
        assert not r["mask"][bad].any() and (r["mask"][~bad] == clean["mask"][~bad]).all()
        assert r["count"] == clean["count"] - int(clean["mask"][bad].sum()) and r["fitness"] == np.float32(r["count"] / len(odd))
    # (e) another world (the ground plane is the one thing the two share): a smaller share of pairs than any source of the
    # same world finds under the same gate
    low = min(fit[(s, float(np.float32(0.6)))] / len(EC.cloud(s)) for s in ("s1", "s2", "s3"))
    for row in EC.rows("e"):
        r = _ref(row, oracle_mod)
        print(f"(e) {row['src']} in {row['tgt']}: fitness {r['fitness']:.3f} against {low:.3f}")
        assert 0 < r["fitness"] < low


def test_mixed_list_holds_what_it_is_there_for(oracle_mod):
    rows = EC.MIXED
    sizes = [len(EC.cloud(r["src"])) for r in rows]
    assert {1, 257} <= set(sizes) and max(sizes) >= 6000
    assert any(r["tgt"] is None for r in rows) and any(r["tgt"] == "empty" for r in rows) and any(r["src"] == r["tgt"] for r in rows)
    a, b = EC.TWICE
    assert rows[a]["src"] == rows[b]["src"] and rows[a]["tgt"] == rows[b]["tgt"] and (rows[a]["T"] == rows[b]["T"]).all() and b - a > 1
    for r in rows:
        ref = _ref(r, oracle_mod)
        if r["tgt"] in (None, "empty"):
            assert ref["count"] == 0 and not ref["S"].any() and ref["fitness"] == 0 and ref["rmse"] == 0
        else:
            assert ref["count"] >= 1
    assert _ref(rows[5], oracle_mod)["count"] == len(EC.cloud("t"))                    # a scan against itself 5 cm off: every point


def _independent(row, ref):
    """The same sums stated another way: the pairs from scipy's kd tree in float64 wherever the nearest distance is unique
    and clear of the gate (the restatement's own pair elsewhere), info = G^T G, g = G^T e."""
    from scipy.spatial import cKDTree
    src, tgt = EC.cloud(row["src"]), EC.cloud(row["tgt"])
    p = E.move(np.eye(4) if row["T"] is None else row["T"], src).astype(np.float64)
    fin_t = np.flatnonzero(np.isfinite(tgt).all(1))
    fin_p = np.isfinite(p).all(1)
    g2 = float(np.float32(row["gate"]) * np.float32(row["gate"]))
    d, j = cKDTree(tgt[fin_t].astype(np.float64)).query(p[fin_p], k=2)
    d2 = d ** 2
    unique = (d2[:, 1] - d2[:, 0] > 1e-5 * np.maximum(d2[:, 1], 1e-12)) & (np.abs(d2[:, 0] - g2) > 1e-5 * g2)
    rows_p = np.flatnonzero(fin_p)
    mask = ref["mask"].copy()
    jj = np.full(len(src), -1, np.int64)
    jj[ref["mask"]] = ref["j"]
    mask[rows_p[unique]] = d2[unique, 0] <= g2
    jj[rows_p[unique]] = fin_t[j[unique, 0]]
    agree = (mask == ref["mask"]).all() and (jj[mask] == ref["j"]).all()
    P, Q = p[mask], tgt[jj[mask]].astype(np.float64)
    G = np.zeros((len(P), 3, 6))
    G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = P[:, 2], -P[:, 1], -P[:, 2], P[:, 0], P[:, 1], -P[:, 0]
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    G = G.reshape(-1, 6)
    e = (P - Q).reshape(-1)
    return agree, int(unique.sum()), int(fin_p.sum()), G.T @ G, G.T @ e, float(e @ e), len(P)


@pytest.mark.parametrize("group", ["a", "b", "c", "d", "e"])
def test_restatement_equals_an_independent_statement(oracle_mod, group):
    for row in EC.rows(group):
        ref = _ref(row, oracle_mod)
        agree, n_unique, n_fin, info, g, s, count = _independent(row, ref)
        assert agree and count == ref["count"]                # wherever scipy's pair is unique it is the restatement's
        if group == "b":
            assert n_unique == 0                              # all ties
        elif group != "a":
            assert n_unique >= 0.99 * n_fin
        tol = E.bound(ref)
        got = np.concatenate([[info[r, c] for r, c in E.TRI], g, [s]])
        err = np.abs(got - ref["S"][:28])
        print(f"({group}) {row['src']} gate {row['gate']:.2f}: {count} pairs, {n_unique} of {n_fin} unique; "
              f"worst error / bound {np.max(err / np.maximum(tol[:28], 1e-300)):.3f}")
        assert (err <= tol[:28]).all()


def test_lattice_sums_equal_exact_integer_arithmetic(oracle_mod):
    for row in EC.rows("a"):
        ref = _ref(row, oracle_mod)
        P = [[int(v) for v in p] for p in EC.cloud(row["src"])]
        S = [0] * E.NSUM
        for x, y, z in P:
            J = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]]
            for k, (a, b) in enumerate(E.TRI):
                S[k] += sum(J[r][a] * J[r][b] for r in range(3))
            S[28] += 1                                        # e = 0: g and the squared residual stay 0
        assert max(abs(v) for v in S) < 2 ** 53
        assert [int(v) for v in ref["S"]] == S and (ref["S"] == np.floor(ref["S"])).all()
