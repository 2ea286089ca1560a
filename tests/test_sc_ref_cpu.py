"""CPU: the numpy restatement of the Scan Context contract (tests/sc_ref.py) has the properties the descriptor is used
for, and the case generator (tests/sc_cases.py) makes what the GPU tests rely on."""
import numpy as np
import pytest

import sc_cases as K
import sc_ref as R


@pytest.fixture(scope="module")
def desc():
    return R.describe(K.clear_of_borders(K.raycast_scans()[0]))


def test_generator_drops_few_points_and_only_border_points():
    for prm in K.PARAM_SETS:
        for s in K.raycast_scans():
            kept = K.clear_of_borders(s, **prm)                  # (asserts the 10 % limit itself)
            assert kept.shape[0] >= 0.9 * s.shape[0]
            _, fr, fs = R.bin_coordinates(kept, **prm)
            for f in (fr, fs):
                assert ((np.abs(f - np.round(f)) >= K.MARGIN) | (f == 0)).all()
    e = K.clear_of_borders(K.special_scans()["edges"], max_dropped=1.0)
    assert (np.hypot(e[:, 0], e[:, 1]) == 0).sum() == 3           # the points at r = 0 stay


def test_describe_edges():
    D = R.describe(K.special_scans()["edges"])
    assert D[0, 0] == np.float32(3.0)                             # r = 0: ring 0, sector 0, max(1 + 2, 0.5 + 2, 0)
    assert D[19].max() == np.float32(2.9)                         # just inside the range: the last ring; beyond: dropped
    assert np.count_nonzero(D) == 5 and D.min() >= 0              # at / below -sensor_height: 0, like an empty bin
    one = R.describe(K.special_scans()["one_point"])
    assert np.count_nonzero(one) == 1 and one[1, 8] == np.float32(3.5)   # r = 5 of 80 m: ring 1; 53.13 degrees: sector 8


def test_ring_key_is_the_row_mean(desc):
    assert np.allclose(R.ring_keys(desc), desc.astype(np.float64).mean(axis=1), rtol=1e-5)


def test_roll_is_found(desc):
    for s in (0, 1, 15, 30, 59):
        d, got = R.distance(desc, np.roll(desc, s, axis=1))       # np.roll(query, s) is the row
        assert got == s and d < 1e-12


def test_equal_columns_score_the_same_at_every_shift():
    rows, _, names = K.distance_pairs()
    eq = rows[names.index("equal_columns")]
    by = R.by_shift(eq, eq)
    assert np.ptp(by) < 1e-12 and R.distance(eq, eq)[1] == 0
    by = R.by_shift(eq, rows[0])
    assert np.ptp(by) < 1e-12 and R.distance(eq, rows[0])[1] == 0


def test_empty_column_rules(desc):
    S = desc.shape[1]
    q = np.zeros_like(desc)
    q[:, 3] = desc[:, 3]
    c = np.zeros_like(desc)
    c[:, 10] = desc[:, 3]
    by = R.by_shift(q, c)
    assert by[7] < 1e-12 and (np.delete(by, 7) == 1.0).all()      # only shift 7 brings the two columns together
    assert R.distance(q, c) == (by[7], 7)
    assert (R.by_shift(q, c, min_common_columns=2) == 1.0).all()  # one common column is below the minimum: 1.0 everywhere
    assert R.distance(q, c, min_common_columns=2) == (1.0, 0)
    # a column that is empty on one side is left out of the mean instead of counting as cosine 0
    half = desc.copy()
    half[:, ::2] = 0
    assert R.by_shift(half, desc)[0] < 1e-12
    zero = np.zeros_like(desc)
    for a, b in ((zero, desc), (desc, zero), (zero, zero)):
        assert (R.by_shift(a, b) == 1.0).all() and R.distance(a, b) == (1.0, 0)
    assert R.by_shift(desc, desc).shape == (S,)


def test_vectorised_restatement_equals_the_plain_one():
    rows, queries, _ = K.distance_pairs()
    assert np.abs(R.by_shift_many(queries[0], rows[3:4])[0] - R.by_shift(queries[0], rows[3])).max() < 1e-12
    assert R.distance(queries[0], rows[3]) [1] == 7              # scan0 against its copy rolled by 7
    for mc in (1, 3):
        for q in queries:
            many = R.by_shift_many(q, rows, mc)
            for i, c in enumerate(rows):
                assert np.abs(many[i] - R.by_shift(q, c, mc)).max() < 1e-12


def test_shift_to_yaw():
    assert R.shift_to_yaw(0) == 0 and abs(R.shift_to_yaw(15) - np.pi / 2) < 1e-15
    assert abs(R.shift_to_yaw(30) - np.pi) < 1e-15                # pi itself is in (-pi, pi]
    assert abs(R.shift_to_yaw(52) - np.deg2rad(-48.0)) < 1e-12
    assert [K.expected_shift(y) for y in K.QUERY_YAWS] == [0, 15, 30, 52]


def test_search_cases_are_decidable():
    for n in (1, 63, 64, 65):
        rows, queries, best, shift, _ = K.search_case(n)          # (asserts the gaps itself)
        assert rows.shape[0] == n and best.shape == (5, n)


def test_two_worlds_are_told_apart():
    """8 places cast in two worlds that share the ground and the road corridor; 16 queries = 4 places x 4 yaws, each
    0.4 m / -0.3 m off its place.  Every query ranks its own place in its own world first, at the right shift (within a
    sector), and the second row -- the same pose in the other world included -- is at least twice as far."""
    db = np.stack([R.describe(s) for s in K.cpu_place_scans()])
    for place in range(4):
        for yaw in K.QUERY_YAWS:
            world = place % 2
            q = R.describe(K.cpu_query_scan(place, world, yaw))
            by = R.by_shift_many(q, db)
            best, shift = by.min(axis=1), by.argmin(axis=1)
            order = np.argsort(best, kind="stable")
            want = K.database_row(place, world)
            assert order[0] == want, (place, yaw, order[:3], best[order[:3]])
            off = (int(shift[want]) - K.expected_shift(yaw)) % 60
            assert off in (0, 1, 59), (place, yaw, shift[want])
            assert best[order[1]] >= 2.0 * best[want], (place, yaw, best[order[:3]])


def test_yaw_seed_is_inside_the_registration_basin(oracle_mod):
    """What tests/test_sc_gpu.py's end-to-end case relies on, checked with the CPU statement of the registration: from the
    yaw-only seed of the -47 degree query (shift 52 = -48 degrees: 1 degree and 0.5 m off) the registration lands within
    the success bound of 1 m / 5 degrees."""
    from gloc3d_amd import loop_detector as L
    place, world, yaw = 3, 1, -47.0
    q = K.cpu_query_scan(place, world, yaw)[:, :3]
    tgt = K.cpu_place_scans()[K.database_row(place, world)][:, :3]
    seed = L.RpyPCLoopDetector.embed_3d((0.0, 0.0, R.shift_to_yaw(K.expected_shift(yaw))))
    out = oracle_mod.reg_one(q, tgt, init_T=seed, ransac_iters=300)
    truth = np.linalg.inv(K.two_worlds()[0][place]) @ K.query_pose(place, yaw)
    er, ep = L.pose_error(truth, out["T"])
    assert out["ok"] and ep < 1.0 and er < 5.0, (er, ep)
