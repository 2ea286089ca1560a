"""CPU: what tests/test_pcm_gpu.py takes for granted about its cases, shown on the reference (tests/pcm_ref.py) alone.

The margin condition: the GPU test compares the consistency matrix bit for bit, so no pair of a restated case may sit at
the threshold.  The cap is ZERO pairs with |s2 / chi2 - 1| < 1e-6 (fp64 rounding of s2 is about 1e-12 relative), and the
numpy.longdouble evaluation must take the same decisions.  Measured with the formula as it stands (closest pair per case):
n60_undrifted 9.5e-3, n60_drift0 9.4e-4, n60_own 3.0e-4, n120_drift0 1.1e-3, n120_own 2.9e-3, n200_drift0 2.7e-3,
n200_own 3.7e-5 -- the seeds of the first choice (5, 7, 9) all meet it, none was replaced.
"""
import numpy as np
import pytest

import pcm_cases as PC
import pcm_ref as M


@pytest.mark.parametrize("name", list(PC.NOISY))
def test_no_pair_sits_at_the_threshold_and_longdouble_decides_the_same(name):
    a, b = PC.restated(name), PC.restated(name, long=True)
    fin = np.isfinite(a["s2"])
    margin = float(np.abs(a["s2"][fin] / M.CHI2_99_6 - 1.0).min())
    scale = float(np.abs(a["s2"][fin].astype(PC.LD) - b["s2"][fin]).max())
    print(f"pcm {name}: L {len(a['mask'])} closest pair {margin:.2e} float64-vs-longdouble {scale:.2e} clique {a['clique_size']} consistent pairs {int(a['C'].sum()) // 2}")
    assert (np.abs(a["s2"][fin] / M.CHI2_99_6 - 1.0) < 1e-6).sum() == 0
    assert (fin == np.isfinite(b["s2"])).all() and (a["C"] == b["C"]).all()
    for k in ("degree", "score", "seeds", "clique_sizes", "mask"):
        assert (a[k] == b[k]).all(), k
    assert (a["winner_rank"], a["clique_size"], a["ok"]) == (b["winner_rank"], b["clique_size"], b["ok"])


def test_undrifted_inliers_are_consistent_and_outliers_with_nothing():
    c, _ = PC.noisy("n60_undrifted")
    r = PC.restated("n60_undrifted")
    inl = ~c["outlier"]
    ni = int(inl.sum())
    rate = r["C"][np.ix_(inl, inl)].sum() / (ni * (ni - 1))
    print(f"pcm undrifted: {ni} inliers of {len(inl)}, inlier-inlier pairs consistent {rate:.4f}, pairs with an outlier {int(r['C'][c['outlier']].sum())}, "
          f"clique {r['clique_size']}")
    assert c["outlier"].sum() >= 5 and rate >= 0.97
    assert r["C"][c["outlier"]].sum() == 0 and r["C"][:, c["outlier"]].sum() == 0


@pytest.mark.parametrize("name", list(PC.NOISY))
def test_the_winner_holds_no_outlier(name):
    c, _ = PC.noisy(name)
    r = PC.restated(name)
    print(f"pcm {name}: winner {r['clique_size']} of {int((~c['outlier']).sum())} inliers, seed rank {r['winner_rank']}")
    assert r["ok"] == 1 and r["clique_size"] >= 2 and r["mask"].sum() == r["clique_size"]
    assert r["mask"][c["outlier"]].sum() == 0


def test_the_matrix_is_symmetric_where_the_two_directions_disagree():
    """C3 evaluates (min, max) only.  Two closures; Omega_b scaled until s2 of (a, b) is above the threshold and s2 of the
    swapped pair below it: with the order swapped the first closure's frame and the transported covariance are other ones."""
    c, _ = PC.noisy("n60_undrifted")
    inl = np.flatnonzero(~c["outlier"])
    def both(a, b, scale):
        info = c["info"].copy()
        info[b] = info[b] * scale
        S = M.setup(c["poses"], c["src"], c["tgt"], c["Z"], info, c["path"])
        return float(M.pair_s2(S, [a], [b])[0]), float(M.pair_s2(S, [b], [a])[0]), info

    found = None
    for a, b in zip(*np.triu_indices(len(inl), 1)):           # the first pair whose mean statistic crosses chi2 as Omega_b grows
        a, b = int(inl[a]), int(inl[b])
        lo, hi = 1e-3, 1e6
        if not (sum(both(a, b, lo)[:2]) < 2 * M.CHI2_99_6 < sum(both(a, b, hi)[:2])):
            continue
        for _ in range(60):                                   # bisect the scale in its logarithm
            mid = np.sqrt(lo * hi)
            ab, ba, info = both(a, b, mid)
            if min(ab, ba) < M.CHI2_99_6 * (1 - 1e-6) and M.CHI2_99_6 * (1 + 1e-6) < max(ab, ba):
                found = (a, b, mid, ab, ba, info)
                break
            lo, hi = (mid, hi) if ab + ba < 2 * M.CHI2_99_6 else (lo, mid)
        if found:
            break
    assert found, "no straddling pair among the inliers"
    a, b, scale, ab, ba, info = found
    print(f"pcm one direction: closures {a}, {b}, Omega_b x {scale}: s2_ab {ab:.3f} s2_ba {ba:.3f} chi2 {M.CHI2_99_6}")
    r = M.consistency(c["poses"], c["src"], c["tgt"], c["Z"], info, c["path"])
    assert (r["C"] == r["C"].T).all() and (r["s2"] == r["s2"].T).all()
    assert r["s2"][a, b] == r["s2"][b, a] == ab and bool(r["C"][a, b]) == (ab < M.CHI2_99_6)


def test_the_batched_statistic_is_the_headers_formula():
    """pair_s2 (arrays, the device's operation order) against pair_s2_scalar (pgo_ref's residual, numpy's inverses).  They
    differ by rounding and by what a float32 Z is short of a rotation (1e-7 of the lever arm)."""
    c, prm = PC.noisy("n60_own")
    S = M.setup(c["poses"], c["src"], c["tgt"], c["Z"], c["info"], c["path"])
    worst = 0.0
    for a, b in ((0, 1), (3, 40), (10, 64), (17, 18), (2, 63)):
        v = float(M.pair_s2(S, [a], [b], **prm)[0])
        w = M.pair_s2_scalar(c["poses"], c["src"], c["tgt"], c["Z"], c["info"], a, b, c["path"], **prm)
        worst = max(worst, abs(v - w) / w)
    print(f"pcm batched vs scalar: worst relative difference {worst:.2e}")
    assert worst < 1e-5


def test_the_closed_form_family_is_decided_by_construction():
    c = PC.cliques()
    S = M.setup(c["poses"], c["src"], c["tgt"], c["Z"], c["info"])
    s2 = M.s2_matrix(S)
    same = c["group"][:, None] == c["group"][None, :]
    off = ~same
    np.fill_diagonal(same, False)
    print(f"pcm cliques: within a group s2 <= {s2[same].max():.2e}, across groups >= {s2[off].min():.2e}")
    assert s2[same].max() < 1e-4 and s2[off].min() > 1e3
    r = M.select(M.consistency_matrix(s2, M.CHI2_99_6), n_seeds=1024)
    e = PC.cliques_expected(c)
    assert (r["degree"] == e["degree"]).all() and (r["score"] == e["score"]).all() and (r["mask"] == e["mask"]).all()
    assert r["seeds"][r["winner_rank"]] == e["winner_seed"] and r["winner_rank"] == 0 and r["clique_size"] == e["clique_size"]
    for rank, s in enumerate(r["seeds"][:len(c["group"])]):
        assert r["clique_sizes"][rank] == c["sizes"][c["group"][s]]
    assert (r["seeds"][len(c["group"]):] == M.NONE).all() and (r["clique_sizes"][len(c["group"]):] == 0).all()
    for L in (1025, 4097):
        sizes = PC.scaled_groups(L)
        assert sum(sizes) == L and sizes[0] > sizes[1] and min(sizes) >= 1


def test_a_zero_information_matrix_is_status_1_and_a_zero_row():
    c, _ = PC.noisy("n60_undrifted")
    info = c["info"].copy()
    info[7] = 0.0
    r = M.consistency(c["poses"], c["src"], c["tgt"], c["Z"], info, c["path"])
    assert r["status"][7] == 1 and r["status"].sum() == 1 and not r["C"][7].any() and not r["C"][:, 7].any() and np.isinf(r["s2"][7]).all()
