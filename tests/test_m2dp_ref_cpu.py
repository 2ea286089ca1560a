"""CPU: the numpy restatement of the M2DP contract (tests/m2dp_ref.py) has the properties the descriptor is used for, and
the case generator (tests/m2dp_cases.py) makes what the GPU tests rely on."""
import numpy as np
import pytest

import m2dp_cases as K
import m2dp_ref as R
import sc_cases
from gloc3d_amd import synth


def test_cases_assert_what_the_tolerances_rest_on():
    for i, prm in enumerate(K.PARAM_SETS):
        raw = sc_cases.raycast_scans()
        for s0, s in zip(raw, K.cleared_scans(i)):                # (assert their gaps themselves)
            assert s.shape == s0.shape
            moved = (s[:, :3] != s0[:, :3]).any(axis=1)
            assert moved.mean() <= 0.10 and np.abs(s[:, :3] - s0[:, :3]).max() < 0.2
            fr, fs, f = R.bin_coordinates(s, **prm)
            assert not K._on_border(fr, fs, R._prm(prm)["n_rings"]).any()
        for name, (s, generic) in K.special_scans(i).items():
            if generic:
                f, cnt = K.assert_generic(s, **prm)
                assert (cnt.sum(axis=1) == f["n"]).all(), name
                fr, fs, _ = R.bin_coordinates(s, **prm)
                assert not K._on_border(fr, fs, R._prm(prm)["n_rings"]).any(), name


def test_border_points_of_a_raw_scan():
    """What clearing is for: 2-3 % of a ray-cast scan's points lie within 1e-4 of a bin of some border."""
    for s in sc_cases.raycast_scans():
        fr, fs, _ = R.bin_coordinates(s)
        share = K._on_border(fr, fs, 8).mean()
        assert 0.005 <= share <= 0.10, share


def test_edges_of_the_contract():
    sp = K.special_scans(0)
    for name in ("one_point", "min_points_minus_1", "all_filtered"):
        d, f, cnt = R.describe(sp[name][0])
        assert not d.any() and not cnt.any() and (f == np.concatenate([np.eye(3).ravel(), np.zeros(3)])).all(), name
    d, f, cnt = R.describe(sp["all_equal"][0])                     # r = 0: everything in bin 0, the identity frame about p
    assert (cnt[:, 0] == 40).all() and cnt.sum() == 40 * 64
    assert (f[:9] == np.eye(3).ravel()).all() and (f[9:] == [3.0, -4.0, 1.5]).all()
    assert abs(np.linalg.norm(d[:64]) - 1) < 1e-6 and d[64] > 0.999 and not d[65:].any()
    a = R.describe(sp["stride4"][0])                                # the 4th column is not read
    b = R.describe(sp["257_points"][0])
    assert (a[0] == b[0]).all() and (a[2] == b[2]).all()
    used = R.used_points(sp["range_and_non_finite"][0])
    assert used[:10].tolist() == [False] * 4 + [True] * 2 + [False] * 4
    assert R.dim() == 192 and R.dim(**K.PARAM_SETS[1]) == 26 and R.dim(**K.PARAM_SETS[2]) == 3


def test_plane_basis_is_a_unit_pair():
    for prm in K.PARAM_SETS:
        u, v = R.plane_basis(**prm)
        assert np.abs((u * u).sum(1) - 1).max() < 1e-15 and np.abs((v * v).sum(1) - 1).max() < 1e-15
        assert np.abs((u * v).sum(1)).max() < 1e-15


def test_jacobi_is_an_eigendecomposition():
    rng = np.random.default_rng(3)
    for _ in range(20):
        M = rng.standard_normal((3, 3))
        C = M @ M.T
        lam, V = R.jacobi_eig3(C)
        assert np.abs(V @ np.diag(lam) @ V.T - C).max() < 1e-12 and np.abs(V.T @ V - np.eye(3)).max() < 1e-14


def test_descriptor_is_invariant_under_rigid_motion():
    """The frame turns with the cloud, so the signature -- and the descriptor -- of a moved cloud is the same, to the
    rounding of the moved points (kept in float64 here; every point stays inside max_range)."""
    s = K.cleared_scans(0)[0][:, :3].astype(np.float64)
    s = s[np.linalg.norm(s, axis=1) < 60.0]
    d0, f0, _ = _describe64(s)
    for yaw, pitch, roll, t in ((35.0, 0, 0, (4.0, -2.0, 0.5)), (180.0, 0, 0, (0, 0, 0)), (-120.0, 7.0, -4.0, (-6.0, 3.0, 0.1))):
        T = synth.se3(yaw, t, pitch, roll)
        moved = s @ T[:3, :3].T + T[:3, 3]
        assert np.linalg.norm(moved, axis=1).max() < 80.0
        d1, f1, _ = _describe64(moved)
        assert np.abs(d1 - d0).max() < 1e-9, (yaw, np.abs(d1 - d0).max())
        seed = R.frame_to_seed(f0, f1)                             # and the two frames give the motion back
        assert np.abs(seed[:3, :3] - T[:3, :3]).max() < 1e-6 and np.abs(seed[:3, 3] - T[:3, 3]).max() < 1e-4


def _describe64(p):
    """R.describe on float64 points as they are (the contract's inputs are fp32; the invariance is a property of the
    arithmetic, so the moved cloud is not rounded to fp32 first)."""
    n = p.shape[0]
    c = p.sum(axis=0) / n
    d = p - c
    lam, V = R.jacobi_eig3(d.T @ d / n)
    order = np.argsort(-lam, kind="stable")
    V = V[:, order]
    e1 = -V[:, 0] if ((d @ V[:, 0]) ** 3).sum() < 0 else V[:, 0]
    e2 = -V[:, 1] if ((d @ V[:, 1]) ** 3).sum() < 0 else V[:, 1]
    Rm = np.stack([e1, e2, np.cross(e1, e2)], axis=1)
    f = dict(R=Rm, c=c, r=float(np.sqrt((d * d).sum(axis=1).max())), n=n)
    fr, fs = R.coordinates_in_frame(d, f)
    ring = np.minimum(np.floor(fr).astype(np.int64), 7)
    sec = np.minimum(np.floor(fs).astype(np.int64), 15)
    cnt = np.zeros((64, 128), np.uint32)
    np.add.at(cnt, (np.broadcast_to(np.arange(64), ring.shape), ring * 16 + sec), 1)
    U, S, Vt = np.linalg.svd(cnt / n, full_matrices=False)
    sg = -1.0 if U[:, 0].sum() < 0 else 1.0
    return np.concatenate([sg * U[:, 0], sg * Vt[0]]), np.concatenate([Rm.ravel(), c]), cnt


def test_signature_svd_of_made_up_counts():
    for name, (cnt, n) in K.made_up_counts().items():
        d, s1, s2 = R.signature_svd(cnt, n)
        if name == "all_zero":
            assert not d.any() and s1 == 0 and s2 == 0
            continue
        assert d.min() >= -1e-7 and abs(np.linalg.norm(d[:64]) - 1) < 1e-6 and abs(np.linalg.norm(d[64:]) - 1) < 1e-6
        if name == "sigma_ratio_0.9":
            assert abs(s2 / s1 - 0.9) < 1e-12
        else:
            assert s2 < 1e-12 * s1


def test_two_worlds_are_told_apart_and_the_frames_give_the_rotation():
    """8 places x 2 worlds that share ground and road; 64 queries, one per place, world and yaw, 0.5 m off.  Every query
    ranks its own place in its own world first, the runner-up is at least 3 x as far in squared distance, and the two
    frames give the rotation query -> place within 5 degrees."""
    db = [R.describe(s) for s in K.place_scans()]
    D = np.stack([d[0] for d in db]).astype(np.float64)
    ratios, angles = [], []
    for place, world, yaw, scan in K.query_scans():
        d, fq, _ = R.describe(scan)
        d2 = ((D - d.astype(np.float64)) ** 2).sum(axis=1)
        order = np.argsort(d2, kind="stable")
        want = sc_cases.database_row(place, world)
        assert order[0] == want, (place, world, yaw, order[:3], d2[order[:3]])
        ratios.append(d2[order[1]] / d2[want])
        seed = R.frame_to_seed(fq, db[want][1])
        angles.append(K.rotation_angle_deg(seed[:3, :3].astype(np.float64), K.true_rotation(place, yaw)))
    print(f"runner-up / own d2: {min(ratios):.2f} .. {max(ratios):.1f}; seed rotation error up to {max(angles):.2f} deg")
    assert min(ratios) >= 3.0 and max(angles) <= 5.0
