"""Inputs for the M2DP tests, generated once per process and shared: scans whose (point, plane) pairs keep clear of the
bin borders, the special scans of the contract's edges, made-up count matrices, and the two-world query set.  Every case
asserts what the tolerances of tests/test_m2dp_gpu.py rest on."""
import functools

import numpy as np

import m2dp_ref as R
import sc_cases

PARAM_SETS = [dict(), dict(n_azimuth=2, n_elevation=3, n_rings=4, n_sectors=5), dict(n_azimuth=1, n_elevation=1, n_rings=1, n_sectors=2)]
PRM_IDS = ["4x16x8x16", "2x3x4x5", "1x1x1x2"]
MARGIN = 1e-4          # of a bin
MIN_GAP = 0.02         # (l1 - l2) / l1 and (l2 - l3) / l2 of every generic case
MIN_M3 = 1e-3          # normalised third moments on e1 and e2, in magnitude
MAX_SIGMA_RATIO = 0.9  # sigma2 / sigma1 of the signature
MAX_PASSES = 6


def assert_generic(pts, **prm):
    """What the frame and descriptor tolerances rest on: separated eigenvalues, third moments away from 0, a separated
    first singular value.  Returns the restated (frame dict, counts)."""
    cnt, f = R.counts(pts, **prm)
    lam, m3 = f["lam"], f["m3"]
    assert f["n"] > 0
    assert (lam[0] - lam[1]) / lam[0] >= MIN_GAP and (lam[1] - lam[2]) / lam[1] >= MIN_GAP, lam
    assert np.abs(m3).min() >= MIN_M3, m3
    _, s1, s2 = R.signature_svd(cnt, f["n"])
    assert s2 / s1 <= MAX_SIGMA_RATIO, (s1, s2)
    return f, cnt


def _on_border(fr, fs, n_rings):
    """A ring coordinate within MARGIN of 1 .. l - 1 (l itself is no border: the ring is clamped to l - 1, and the farthest
    point sits there on every plane that holds it), a sector coordinate within MARGIN of any integer -- the turn closes at
    0 -- unless it is exactly 0 (rho = 0, or atan2(0, x > 0), exact in any precision)."""
    k = np.round(fr)
    ring = (np.abs(fr - k) < MARGIN) & (k >= 1) & (k <= n_rings - 1)
    sector = (np.abs(fs - np.round(fs)) < MARGIN) & (fs != 0)
    return (ring | sector).any(axis=1)


def clear_of_borders(pts, max_dropped=0.10, **prm):
    """The scan with no used point that has, on any plane, a fractional ring or sector coordinate (float64) within MARGIN
    of a bin border (_on_border); points M1 leaves out stay as they are.  At most `max_dropped` of the points are touched.

    A border point is not taken out but moved by millimetres to where it is clear on every plane.  Taking 2.5 % of a
    scan out moves its centroid by centimetres -- 1e-3 of a bin, ten margins -- so the next pass would find as many fresh
    border points as the first and the clearing would never end; moving them by a few millimetres moves the frame by
    1e-7 of a bin, and the second pass finds a handful.  The passes are repeated until one finds nothing, within
    MAX_PASSES.  A point is only moved to within r = max |p - c|: every ring coordinate scales with r."""
    pts = np.ascontiguousarray(pts, np.float32).copy()
    touched = np.zeros(pts.shape[0], bool)
    rng = np.random.default_rng(pts.shape[0])
    for _ in range(MAX_PASSES):
        fr, fs, f = R.bin_coordinates(pts, **prm)
        if f["n"] == 0:
            return pts
        used = np.flatnonzero(R.used_points(pts, **prm))
        l = R._prm(prm)["n_rings"]
        todo = used[_on_border(fr, fs, l)]
        if not len(todo):
            assert touched.sum() <= max_dropped * pts.shape[0], f"{touched.mean():.1%} of the points lie on a bin border"
            return pts
        for i in todo:
            for step in range(1, 40):
                cand = (pts[i, :3].astype(np.float64) + 2e-3 * step * rng.standard_normal(3) / np.sqrt(3)).astype(np.float32)
                d = cand.astype(np.float64)[None, :] - f["c"]
                ok = R.used_points(cand[None, :], **prm)[0] and (d * d).sum() < f["r"] ** 2
                if ok and not _on_border(*R.coordinates_in_frame(d, f, **prm), l)[0]:
                    pts[i, :3] = cand
                    break
            else:
                raise AssertionError("no clear place near a border point")
        touched[todo] = True
    raise AssertionError(f"clearing the bin borders did not end within {MAX_PASSES} passes")


@functools.lru_cache(maxsize=None)
def cleared_scans(prm_index):
    """The three ray-cast scans of sc_cases (x y z i, ~30 000 returns), cleared for PARAM_SETS[prm_index]."""
    prm = PARAM_SETS[prm_index]
    out = [clear_of_borders(s, **prm) for s in sc_cases.raycast_scans()]
    for s in out:
        assert_generic(s, **prm)
    return out


def stride4(xyz):
    """x y z i rows with a 4th column that would show if it were read as a coordinate."""
    out = np.full((xyz.shape[0], 4), 1e4, np.float32)
    out[:, :3] = xyz[:, :3]
    return out


@functools.lru_cache(maxsize=None)
def special_scans(prm_index=0):
    """name -> (scan [n, 3|4], generic?): the edges of M1 and of the reductions.  Generic cases are cleared of the bin
    borders and assert their gaps; the others are decided exactly (zero rows, or every point in bin 0)."""
    prm = PARAM_SETS[prm_index]
    mp = R.DEFAULTS["min_points"]
    base = np.ascontiguousarray(sc_cases.raycast_scans()[0][:, :3])
    rng = np.random.default_rng(2016)
    pick = lambda n: np.ascontiguousarray(base[np.sort(rng.choice(base.shape[0], n, replace=False))])
    out = {"one_point": (np.array([[3.0, 4.0, 1.5]], np.float32), False),
           "min_points_minus_1": (pick(mp - 1), False),
           "all_equal": (np.tile(np.array([[3.0, -4.0, 1.5]], np.float32), (40, 1)), False)}
    for n in (mp, 63, 64, 65, 257):
        for _ in range(50):                       # a random subset may have a third moment near 0: take the first that has not
            s = clear_of_borders(pick(n), max_dropped=1.0, **prm)
            f = R.frame(s, **prm)
            gaps_ok = f["n"] >= mp and min((f["lam"][0] - f["lam"][1]) / f["lam"][0], (f["lam"][1] - f["lam"][2]) / f["lam"][1]) >= 2 * MIN_GAP
            if gaps_ok and np.abs(f["m3"]).min() >= 2 * MIN_M3:
                cnt = R.counts(s, **prm)[0]
                _, s1, s2 = R.signature_svd(cnt, f["n"])
                if s2 / s1 <= MAX_SIGMA_RATIO:
                    break
        assert_generic(s, **prm)
        out[f"{n}_points"] = (s, True)
    # the range limit from both sides: |p| = max_range is out, the next float below is in; non-finite rows are out
    mr = np.float32(R.DEFAULTS["max_range"])
    below, above = np.nextafter(mr, np.float32(0)), np.nextafter(mr, np.float32(np.inf))
    body = pick(300)
    edge = np.array([[mr, 0, 0], [0, above, 0], [0, 0, -mr], [200.0, 100.0, 1.0], [below, 0, 0], [0, 0, below],
                     [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf], [2.0, 2.5, np.nan]], np.float32)
    assert R.used_points(edge, **prm).tolist() == [False] * 4 + [True] * 2 + [False] * 4
    scan = clear_of_borders(np.concatenate([edge, body]), max_dropped=1.0, **prm)
    assert_generic(scan, **prm)
    out["range_and_non_finite"] = (scan, True)
    out["all_filtered"] = (np.ascontiguousarray(edge[[0, 1, 2, 3, 6, 7, 8, 9] * 3]), False)
    out["stride4"] = (stride4(out["257_points"][0]), True)
    return out


def made_up_counts(n_planes=64, n_bins=128):
    """name -> (counts [n_planes, n_bins] uint32, n_points): what the SVD kernel is held to beyond real signatures."""
    rng = np.random.default_rng(64128)
    a, b = rng.integers(1, 9, n_planes), rng.integers(0, 7, n_bins)
    b[0] = 3
    one = np.zeros((n_planes, n_bins), np.uint32)
    one[n_planes // 3, n_bins - 1] = 17
    two = np.zeros((n_planes, n_bins), np.uint32)                 # two rank-one blocks on separate rows and columns:
    h, w = max(n_planes // 2, 1), n_bins // 2                     # sigma = 10 sqrt(h w) and 9 sqrt(h w): a ratio of 0.9
    two[:h, :w] = 10
    if n_planes >= 2:
        two[h:2 * h, w:2 * w] = 9
    return {"rank_one": (np.outer(a, b).astype(np.uint32), 1000), "one_entry": (one, 17),
            "all_zero": (np.zeros((n_planes, n_bins), np.uint32), 5), "sigma_ratio_0.9": (two, 4096)}


# ---- the two-world place set (sc_cases): 8 places x 2 worlds, a query at each of 4 yaws per place --------------------

def place_scans():
    return sc_cases.cpu_place_scans()


@functools.lru_cache(maxsize=None)
def query_scans():
    """[(place, world, yaw_deg, scan)] for all 64 queries."""
    return [(p, w, yaw, sc_cases.cpu_query_scan(p, w, yaw)) for w in range(2) for p in range(8) for yaw in sc_cases.QUERY_YAWS]


def true_rotation(place, yaw_deg):
    """The rotation query -> place of a query pose."""
    T = np.linalg.inv(sc_cases.two_worlds()[0][place]) @ sc_cases.query_pose(place, yaw_deg)
    return T[:3, :3]


def rotation_angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
