"""CPU: the ground sweep's case table (tests/ground_cases.py) is sound before a GPU sees it -- on the oracle
(oracle/ground_oracle.c) every named case reaches the branch it is named for, and the oracle itself agrees with two independent
references on the new shapes: the k-NN stated in fp32 numpy, bit for bit, and numpy.linalg.eigh of the fp64 covariance for the
normals, by angle, wherever the smallest eigenvalue is separated."""
import numpy as np
import pytest

import ground_cases as gc
from util import bits

ADMISSIBLE = [b for b in range(18) if not 4 < b < 13]

# The eigh comparison.  SEPARATION: a normal is compared where (l1 - l0) / l2 of its neighbourhood's covariance is above it.
# ANGLE_BOUND: ten times the largest angle measured between the oracle's normal and eigh's over every shape of the table
# (4.66e-8 rad, size4033): the oracle hands its fp64 normal out as float32, and that rounding (up to 2^-24 * sqrt(3) / 2 =
# 5.2e-8 rad) is all of the figure; cyclic Jacobi against LAPACK is eps * l2 / gap <= 2.2e-16 / 1e-4, five orders below.
SEPARATION = 1e-4
ANGLE_BOUND = 4.7e-7
EXCLUDED_CAP = 0.10


def _lists(oracle_mod, name, k):
    return oracle_mod.ground_knn(gc.shape(name), k)


def test_param_rows_cover_the_listed_values():
    assert len({gc.row_id(r) for r in gc.PARAM_ROWS}) == len(gc.PARAM_ROWS) <= 24
    for f, values in gc.REQUIRED_VALUES.items():
        assert set(values) <= {row[f] for row in gc.PARAM_ROWS}, f
    for row in gc.PARAM_ROWS:
        assert set(row) == set(gc.FIELDS) and 3 <= row["knn"] <= 16 and 1 <= row["ransac_iters"] <= 65536
    for name in gc.SCENES:
        rows = gc.rows_of(name)
        assert gc.DEFAULTS in rows and (len(rows) >= len(gc.PARAM_ROWS) or name in gc.FEW_ROWS)
    for name, rows in gc.FEW_ROWS.items():
        assert len(rows) == 2 and rows[0] == gc.DEFAULTS and rows[1] == dict(gc.DEFAULTS, seed=rows[1]["seed"])


def test_the_table_holds_the_sizes_and_edges_it_names():
    assert {(m + 63) // 64 % 4 for m in gc.SIZES if m > 256} == {0, 1, 2, 3}       # idle waves in the last work-group: 0..3
    assert {(m + 63) // 64 for m in gc.SIZES} >= {64, 65, 66} and {m % 64 for m in gc.SIZES} >= {1, 63, 0}
    assert {256, 257} <= set(gc.SIZES)                                             # the dispatch switches above 4 * KCH
    for m in gc.SIZES:
        assert gc.shape("size%d" % m).shape == (m, 3)
    assert all(gc.shape(n).shape[0] <= 3000 or n.startswith("size") for n in gc.SHAPES)
    assert (gc.shape("identical") == gc.shape("identical")[0]).all() and gc.shape("identical").shape[0] == 1000
    lat = gc.shape("lattice")
    assert lat.shape[0] == 12 ** 3 and (lat == np.round(lat)).all() and np.unique(lat, axis=0).shape[0] == 12 ** 3
    assert np.unique(gc.shape("sheet")[:, 2]).size == 1 and np.unique(gc.shape("line")[:, 1:], axis=0).shape[0] == 1
    far = gc.shape("far_offset")
    assert (np.abs(far) >= 7999).all() and (np.abs(far) <= 8001).all()
    co = gc.shape("clusters_outliers")
    r = np.linalg.norm(co, axis=1)
    assert (r > 900).sum() == 40 and (r < 10).sum() == co.shape[0] - 40
    nf, bad = gc.shape("nonfinite"), gc.nonfinite_rows()
    rows = np.flatnonzero(~np.isfinite(nf).all(1))
    assert set(rows.tolist()) == set(bad) and 0 in bad and nf.shape[0] - 1 in bad and 0.005 < len(bad) / nf.shape[0] < 0.015
    assert np.isnan(nf).any() and (nf == np.inf).any() and (nf == -np.inf).any()
    whole = (~np.isfinite(nf[rows])).all(1)
    assert whole.any() and (~whole).any()                                          # whole rows and single coordinates
    # many_tiles: the rows within range sit where the compaction's seams are
    rows = gc.many_tiles_rows()
    n, t = 530000, gc.SEL_TILE
    assert rows[0] == 0 and rows[-1] == n - 1 and 2900 <= rows.shape[0] <= 3100 and n > 256 * t + t
    have = set(rows.tolist())
    assert all({j * t - 1, j * t} <= have for j in (1, 2, 3, 4, 5, 6, 255, 256, 257, 258))
    assert all(np.count_nonzero(rows // t == tile) > 100 for tile in (255, 256, 257, 258))
    cloud = gc.scene("many_tiles")
    near = np.einsum("ij,ij->i", cloud, cloud) < 400
    assert cloud.shape == (n, 3) and (np.flatnonzero(near) == rows).all() and (cloud[~near] == gc.FAR_ROW).all()
    last = gc.scene("tile_edges_last")
    near = np.flatnonzero(np.einsum("ij,ij->i", last, last) < 400)
    assert last.shape[0] == 2 * t and set(near.tolist()) == set(gc.TILE_LAST_ROWS) >= {t - 1, 2 * t - 1} and near.size == 4
    for m in (2047, 2048, 2049):
        c = gc.scene("tile_edges%d" % m)
        assert c.shape[0] == m and (np.einsum("ij,ij->i", c[:, :3], c[:, :3]) < 400).all()
    assert {gc.scene(n).shape[1] for n in gc.SCENES} >= {3, 5, 16}
    assert all(gc.scene(n).shape[0] <= 20000 for n in gc.SCENES if n != "many_tiles")


# ---- the lists -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(gc.SHAPES))
def test_lists_equal_the_numpy_statement(oracle_mod, name):
    p = gc.shape(name)
    for k in (16, 1):
        oi, od = _lists(oracle_mod, name, k)
        ri, rd = gc.knn_numpy(p, k)
        assert (oi == ri).all() and (bits(od) == bits(rd)).all(), (name, k)
    if p.shape[0] < 16:                                                            # fewer points than k: the padding
        oi, od = _lists(oracle_mod, name, 16)
        assert (oi[:, p.shape[0]:] == gc.NONE).all() and (od[:, p.shape[0]:] == gc.FLT_MAX).all()
        assert (oi[:, :p.shape[0]] != gc.NONE).all()


def test_ties_at_the_kth_distance(oracle_mod):
    for k in (3, 10, 16):
        assert gc.tie_share(gc.shape("lattice"), k) >= 0.20, k
        assert gc.tie_share(gc.shape("identical"), k) == 1.0, k
        oi, od = _lists(oracle_mod, "identical", k)
        assert (oi == np.arange(k, dtype=np.uint32)[None, :]).all() and (od == 0).all()    # the k smallest indices, not "itself first"
    oi, _ = _lists(oracle_mod, "identical", 10)
    assert (oi[500] != 500).all()


def test_non_finite_points_are_nobodys_neighbours(oracle_mod):
    p, bad = gc.shape("nonfinite"), sorted(gc.nonfinite_rows())
    for k in (1, 10, 16):
        oi, od = _lists(oracle_mod, "nonfinite", k)
        assert not np.isin(oi, bad).any()
        assert (oi[bad] == gc.NONE).all() and (od[bad] == gc.FLT_MAX).all()
        good = np.setdiff1d(np.arange(p.shape[0]), bad)
        assert (oi[good] != gc.NONE).all() and (oi[good, 0] == good).all()
    nrm, bins = oracle_mod.ground_normals(p, _lists(oracle_mod, "nonfinite", 10)[0])
    assert (nrm[bad] == 0).all() and (bins[bad] == 9).all() and np.isfinite(nrm).all()


# ---- the normals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(gc.SHAPES))
def test_normals_against_eigh(oracle_mod, name):
    p = gc.shape(name)
    oi, _ = _lists(oracle_mod, name, gc.NORMALS_K.get(name, 10))
    nrm, bins = oracle_mod.ground_normals(p, oi)
    w, v, cnt = gc.normals_eigh(p, oi)
    has = cnt >= 3
    assert (nrm[~has] == 0).all() and (bins[~has] == 9).all()                      # fewer than three neighbours: no normal
    keep = has & (gc.separation(w) > SEPARATION)
    if name in gc.DEGENERATE or not has.any():
        assert not keep.any()
        return
    assert 1.0 - keep.sum() / has.sum() <= EXCLUDED_CAP, name
    angle = gc.angle_between(nrm[keep], v[keep])
    print("%s: %d of %d normals compared, largest angle to eigh %.3e rad" % (name, keep.sum(), has.sum(), angle.max()))
    assert angle.max() < ANGLE_BOUND
    assert np.abs(np.linalg.norm(nrm[keep].astype(np.float64), axis=1) - 1).max() < 1e-6
    away = np.einsum("ij,ij->i", nrm[keep].astype(np.float64), p[keep].astype(np.float64))
    assert (away <= 1e-6 * np.linalg.norm(p[keep], axis=1)).all()                  # flipped towards the origin (float32 output)
    sin_el = nrm[keep, 2].astype(np.float64)
    clear = np.abs(sin_el[:, None] - np.sin(np.deg2rad(np.arange(-80, 90, 10)))[None, :]).min(1) > 1e-6
    assert (bins[keep][clear] == np.floor((np.degrees(np.arcsin(sin_el[clear])) + 90) / 10).clip(0, 17)).all()


def test_degenerate_neighbourhoods(oracle_mod):
    """C = 0 and two zero eigenvalues ("ties keep the lower column"), normals exactly along +-z, fewer than three neighbours."""
    def normals(name, k=10):
        return oracle_mod.ground_normals(gc.shape(name), _lists(oracle_mod, name, k)[0])
    for k in (3, 10, 16):
        nrm, b = normals("identical", k)                   # C = 0: column 0, flipped towards the origin from x = 1.5
        assert (nrm == np.float32([-1, 0, 0])).all() and (b == 9).all()
        nrm, b = normals("line", k)                        # eigenvalues (c, 0, 0): column 1 is the lower of the two zeros
        assert (np.abs(nrm) == np.float32([0, 1, 0])).all() and (b == 9).all()
        nrm, b = normals("sheet", k)                       # below the sensor: exactly +z, the clamp of bin 17
        assert (nrm == np.float32([0, 0, 1])).all() and (b == 17).all()
        nrm, b = normals("sheet_above", k)                 # above it: exactly -z, bin 0
        assert (nrm == np.float32([0, 0, -1])).all() and (b == 0).all()
    nrm, b = normals("size2")
    assert (nrm == 0).all() and (b == 9).all()
    nrm, b = normals("size3")
    assert (np.abs(np.linalg.norm(nrm, axis=1) - 1) < 1e-6).all()


# ---- the estimate scenes -------------------------------------------------------------------------------------------------

def _estimate(oracle_mod, name, **over):
    prm = dict(gc.SCENE_PARAMS.get(name, gc.DEFAULTS), **over)
    return oracle_mod.ground_estimate(gc.scene(name), **prm)


def _max_admissible(info):
    return int(info["hist"][ADMISSIBLE].max())


@pytest.mark.parametrize("stride", (3, 5, 16))
def test_lidar_scene(oracle_mod, stride):
    T, info = _estimate(oracle_mod, "lidar%d" % stride)
    T3, info3 = _estimate(oracle_mod, "lidar3")
    assert gc.scene("lidar%d" % stride).shape[1] == stride and info["found"] == 1 and info["ground_bin"] == 17
    assert (T == T3).all() and info["n_ground"] == info3["n_ground"] > 3000 and abs(T[2, 3] - 1.73) < 0.05


def test_ceiling_wins(oracle_mod):
    T, info = _estimate(oracle_mod, "ceiling_wins")
    assert info["found"] == 1 and info["ground_bin"] == 0 and info["plane"][2] < 0
    assert info["hist"][0] > info["hist"][17] >= 3                                 # a floor is there, the ceiling is fuller
    cloud = gc.scene("ceiling_wins")
    moved = gc.moved_fp64(cloud, T)
    ceiling = cloud[:, 2] > 2.0
    # the reference turns the plane's normal upward and lifts by |d|: the ceiling (2.5 m above) lands 5 m up, not at 0
    assert ceiling.sum() == info["n_ground"] and np.abs(moved[ceiling, 2] - 5.0).max() < 0.05 and T[2, 2] > 0.99


def test_bin_tie(oracle_mod):
    _, info = _estimate(oracle_mod, "bin_tie")
    top = _max_admissible(info)
    assert [b for b in ADMISSIBLE if info["hist"][b] == top] == [0, 17] and info["ground_bin"] == 0 and info["found"] == 1
    assert info["n_ground"] == top == 800


@pytest.mark.parametrize("name", ("collinear_ground", "duplicate_ground"))
def test_ground_sets_without_a_plane(oracle_mod, name):
    for iters in (1, 255, 1000):
        _, info = _estimate(oracle_mod, name, ransac_iters=iters)
        assert info["found"] == 0 and info["ground_bin"] == 17 and info["best_hyp"] == gc.NONE and info["inliers"] == 0
        assert info["n_ground"] >= 3 and info["iters_used"] == iters
    cloud = gc.scene(name)[:, :3]
    oi, _ = oracle_mod.ground_knn(cloud, 10)
    ground = cloud[oracle_mod.ground_normals(cloud, oi)[1] == 17]
    assert ground.shape[0] == info["n_ground"]
    if name == "duplicate_ground":
        assert (ground == ground[0]).all()
    else:
        assert np.unique(ground, axis=0).shape[0] == ground.shape[0] and np.unique(ground[:, 1:], axis=0).shape[0] == 1


def test_tiny_bin(oracle_mod):
    T, info = _estimate(oracle_mod, "tiny_bin")
    assert info["ground_bin"] == -1 and info["n_near"] >= 3 and info["found"] == 0 and 0 < _max_admissible(info) < 3
    assert (T == np.eye(4)).all() and info["n_ground"] == 0


def test_multi_slab(oracle_mod):
    _, info = _estimate(oracle_mod, "multi_slab")
    ng = info["n_ground"]
    slabs = min(64, (ng + 4095) // 4096)
    assert 8200 <= ng <= 13000 and info["n_near"] <= 16000 and slabs >= 3 and ng % slabs != 0
    assert info["found"] == 1 and 0.3 * ng < info["inliers"] < 0.9 * ng           # hypotheses differ in their counts


def test_compaction_scenes(oracle_mod):
    _, info = _estimate(oracle_mod, "many_tiles")
    assert info["n_near"] == gc.many_tiles_rows().shape[0] and info["found"] == 1 and info["n_ground"] > 2000
    for m in (2047, 2048, 2049):
        _, info = _estimate(oracle_mod, "tile_edges%d" % m)
        assert info["n_near"] == m and info["found"] == 1
    _, info = _estimate(oracle_mod, "tile_edges_last")
    assert info["n_near"] == 4 and info["hist"].sum() == 4                         # four points: every list is short of k


def test_adaptive_stop(oracle_mod):
    for name in ("lidar3", "ceiling_wins"):
        for conf in gc.REQUIRED_VALUES["ransac_conf"]:
            for iters in gc.REQUIRED_VALUES["ransac_iters"] if name == "lidar3" else (255, 1000):
                _, info = _estimate(oracle_mod, name, ransac_conf=conf, ransac_iters=iters)
                assert info["found"] == 1
                if 0 < conf < 1 and iters > 1:
                    assert info["iters_used"] < iters, (name, conf, iters)
                else:
                    assert info["iters_used"] == iters, (name, conf, iters)
