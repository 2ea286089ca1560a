"""CPU: the numpy restatement of the local-submap contract (tests/submap_ref.py) against a second, independent statement
(np.unique over integer cells, float64 means), its edge cases, and what a submap is for: a query registers closer to the
truth against the submap of a place than against the place's own scan."""
import numpy as np
import pytest

import submap_cases as cases
import submap_ref as ref
from util import bits

EYE = np.eye(4, dtype=np.float32)


def unique_statement(members, leaf):
    """Cells by np.unique on float64-computed integer coordinates, means in float64 (no statement about order inside a
    cell).  Only for inputs whose float64 and float32 cell indices agree: the callers check the cell sets."""
    pts = []
    for xyz, T in members:
        p = np.ascontiguousarray(xyz, np.float32)[:, :3]
        T = np.asarray(T, np.float32)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        pts.append(np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1))
    q = np.concatenate(pts)
    k = np.floor(q * (np.float32(1.0) / np.float32(leaf))).astype(np.int64)       # the fp32 product: cells are the contract
    cells, inverse, counts = np.unique(k, axis=0, return_inverse=True, return_counts=True)
    mean = np.zeros((len(cells), 3), np.float64)
    np.add.at(mean, inverse.reshape(-1), q.astype(np.float64))
    return cells, mean / counts[:, None], counts


def small_members():
    places, P, _, _ = cases.trajectory()
    js = [1, 2, 3]
    T = cases.member_poses(P, cases.ANCHOR, js)
    return [(places[j][::6], T[m]) for m, j in enumerate(js)]


@pytest.mark.parametrize("leaf", [0.2, 0.5])
def test_restatement_against_the_unique_statement(leaf):
    members = small_members()
    out, info = ref.submap(members, leaf=leaf)
    cells, mean, counts = unique_statement(members, leaf)
    assert info["cells"] == info["kept"] == len(cells) == out.shape[0]
    assert (info["cell_keys"] == cells).all()                        # same cell set, same (kx, ky, kz) order
    assert info["points_in"] == info["points_used"] == counts.sum()
    assert np.abs(out.astype(np.float64) - mean).max() <= 1e-6 * max(1.0, np.abs(mean).max())


def test_identity_single_member_is_the_voxel_grid_filter():
    places, _, _, _ = cases.trajectory()
    p = places[0][::4]
    out, info = ref.submap([(p, EYE)], leaf=0.2)
    assert (bits(ref._keys(p, EYE, 0.2, 0.0)[0]) == bits(p)).all()    # the identity pose moves nothing, not a bit
    k = np.floor(p * (np.float32(1.0) / np.float32(0.2))).astype(np.int64)
    cells = np.unique(k, axis=0)
    assert (info["cell_keys"] == cells).all() and out.shape[0] == len(cells)
    for c in (0, len(cells) // 2, len(cells) - 1):                    # a cell's centroid: its points, summed in index order
        rows = p[(k == cells[c]).all(axis=1)].astype(np.float64)
        s = np.zeros(3)
        for r in rows:
            s = s + r
        assert (bits((s / len(rows)).astype(np.float32)) == bits(out[c])).all()


def test_cell_order_with_negative_coordinates():
    pts = np.array([[0.1, 0.1, 0.1], [-0.1, 0.1, 0.1], [-0.1, -0.1, 0.1], [-0.1, -0.1, -0.1], [0.1, -0.1, -0.1], [-0.3, 0.5, 0.0],
                    [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [-0.2, 0.0, 0.0], [0.2, 0.0, -0.2]], np.float32)
    out, info = ref.submap([(pts, EYE)], leaf=0.2)
    keys = info["cell_keys"]
    assert [tuple(k) for k in keys] == sorted(tuple(k) for k in keys)             # lexicographic in (kx, ky, kz), signed
    assert tuple(keys[0]) == (-2, 2, 0) and tuple(keys[-1]) == (1, 0, -1)
    assert (0, 0, 0) in {tuple(k) for k in keys}
    zero = [tuple(k) for k in keys].index((0, 0, 0))                              # +0.0 and -0.0 share cell 0 with (0.1, 0.1, 0.1)
    assert np.allclose(out[zero], np.float32(0.1) / 3)
    # a coordinate on a cell face: the fp32 product q * (1.0f / leaf) decides, nothing else does
    f = np.floor(np.float32(-0.2) * (np.float32(1.0) / np.float32(0.2)))
    assert (int(f), 0, 0) in {tuple(k) for k in keys}


def test_point_order_matters_only_through_the_summation_order():
    rng = np.random.default_rng(5)
    pts = (rng.uniform(0.0, 0.2, (4000, 3)) + (1.0, 2.0, 0.4)).astype(np.float32)   # a few cells, long runs
    a, ia = ref.submap([(pts, EYE)], leaf=0.2)
    perm = rng.permutation(len(pts))
    b, ib = ref.submap([(pts[perm], EYE)], leaf=0.2)
    assert (ia["cell_keys"] == ib["cell_keys"]).all()                 # the cells and their order never depend on it
    assert np.abs(a.astype(np.float64) - b).max() <= 2.0 ** -22       # the centroids: by an fp64 sum's rounding, then fp32's
    # splitting the same points over two members in the same order is the same sum, bit for bit
    c, _ = ref.submap([(pts[:1500], EYE), (pts[1500:], EYE)], leaf=0.2)
    assert (bits(a) == bits(c)).all()
    # ... and the documented order is the one used: the other order of the two members is the other sum
    d, _ = ref.submap([(pts[1500:], EYE), (pts[:1500], EYE)], leaf=0.2)
    e, _ = ref.submap([(np.concatenate([pts[1500:], pts[:1500]]), EYE)], leaf=0.2)
    assert (bits(d) == bits(e)).all()


def test_ordered_sums_are_sequential():
    rng = np.random.default_rng(9)
    v = (rng.standard_normal((3000, 3)) * 1e3).astype(np.float32).astype(np.float64)
    start = np.array([0, 1, 3, 1000, 2999])
    length = np.array([1, 2, 997, 1999, 1])
    got = ref.ordered_sums(v, start, length)
    for r in range(len(start)):
        s = np.zeros(3)
        for row in v[start[r]:start[r] + length[r]]:
            s = s + row
        assert (got[r] == s).all()


def test_min_points_min_scans_max_range():
    members = small_members()
    full, info = ref.submap(members, leaf=0.2)
    cells, _, counts = unique_statement(members, 0.2)
    out3, i3 = ref.submap(members, leaf=0.2, min_points=3)
    assert i3["cells"] == info["cells"] and i3["kept"] == int((counts >= 3).sum()) == out3.shape[0]
    assert (i3["cell_keys"] == cells[counts >= 3]).all()
    assert ref.submap(members, leaf=0.2, min_points=0)[1]["kept"] == info["kept"]            # 0 means 1
    # min_scans: distinct member POSITIONS per cell (an id listed twice counts twice)
    per_member = [{tuple(k) for k in ref.submap([m], leaf=0.2)[1]["cell_keys"]} for m in members]
    seen = {}
    for s in per_member:
        for k in s:
            seen[k] = seen.get(k, 0) + 1
    for ms in (2, 3):
        _, im = ref.submap(members, leaf=0.2, min_scans=ms)
        assert {tuple(k) for k in im["cell_keys"]} == {k for k, c in seen.items() if c >= ms}
    twice, it = ref.submap([members[0], members[0]], leaf=0.2, min_scans=2)
    once, io = ref.submap([members[0]], leaf=0.2)
    assert it["kept"] == io["kept"] and ref.submap([members[0]], leaf=0.2, min_scans=2)[1]["kept"] == 0
    # max_range: by the point's distance from its OWN sensor, (x x + y y) + z z in fp32, before the pose
    p, T = members[0]
    r2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    near = ~(r2 > np.float32(20.0) * np.float32(20.0))
    a, ia = ref.submap([(p, T)], leaf=0.2, max_range=20.0)
    b, ib = ref.submap([(p[near], T)], leaf=0.2)
    assert 0 < near.sum() < len(p) and ia["points_used"] == near.sum() and ia["points_in"] == len(p)
    assert (bits(a) == bits(b)).all()
    # non-finite rows and rows outside the key range are left out, and nothing else changes
    bad = np.concatenate([p[:50], [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e5, 0, 0], [0, -3e5, 0]], p[50:]]).astype(np.float32)
    c, ic = ref.submap([(bad, T)], leaf=0.2)
    d, _ = ref.submap([(p, T)], leaf=0.2)
    assert ic["points_in"] == len(p) + 5 and ic["points_used"] == len(p) and (bits(c) == bits(d)).all()
    assert ref.submap([(bad[50:55], T)], leaf=0.2)[1]["kept"] == 0


def test_queries_register_closer_against_the_submap(oracle_mod):
    """The issue's table: four queries around place 2 of a five-place trajectory, the CPU checker's RANSAC + ICP against the
    place's own scan and against its submap (all five places, leaf 0.2 m)."""
    places, P, queries, Q = cases.trajectory()
    js = list(range(5))
    T = cases.member_poses(P, cases.ANCHOR, js)
    sub, info = ref.submap([(places[j], T[m]) for m, j in enumerate(js)], leaf=0.2)
    assert info["kept"] == sub.shape[0] > max(len(p) for p in places)
    for qi, q in enumerate(queries):
        gt = cases.truth(P, Q, qi)
        one = oracle_mod.reg_one(q, places[cases.ANCHOR], ransac_iters=3000, icp_iters=30)
        many = oracle_mod.reg_one(q, sub, ransac_iters=3000, icp_iters=30)
        e1, e2 = cases.position_error(one["T"], gt), cases.position_error(many["T"], gt)
        print(f"query {qi}: position error {e1:.3f} m against the anchor scan, {e2:.3f} m against the submap; "
              f"rmse {one['rmse']:.3f} / {many['rmse']:.3f}, rotation error {cases.rotation_error_deg(one['T'], gt):.2f} / "
              f"{cases.rotation_error_deg(many['T'], gt):.2f} deg")
        assert e2 < e1
