"""CPU: the coarse matcher's case table (tests/coarse_cases.py) is sound before a GPU sees it -- the restatement
(oracle/coarse_oracle.c) builds the grids the independent numpy statement builds, its dilation is the stated one as seen
through the public result, and the known answers, the 1.2 x rule and the acceptance edges come out as constructed."""
import numpy as np
import pytest

import coarse_cases as cc


def _grid(oracle_mod, case):
    return oracle_mod.CoarseGrid(case["img"], case["ox"], case["oy"], case["res"], case["cell_px"])


def _match(oracle_mod, q, d, prm):
    return oracle_mod.coarse_match(q, d, prm["n_yaw"], prm["max_shift"], prm["top_yaw"], prm["refine"], prm["min_overlap"])


def test_param_rows_cover_the_listed_values_inside_the_bounds():
    assert 20 <= len(cc.PARAM_ROWS) <= 28 and len({cc.row_id(r) for r in cc.PARAM_ROWS}) == len(cc.PARAM_ROWS)
    for row in cc.PARAM_ROWS:
        assert set(row) == set(cc.FIELDS)
        assert any(row[f] != cc.DEFAULTS[f] for f in cc.FIELDS), row
        for f, (lo, hi) in cc.BOUNDS.items():
            assert lo <= row[f] <= hi, (f, row)
        assert row["top_yaw"] <= row["n_yaw"], row
    for f, values in cc.REQUIRED_VALUES.items():
        assert set(values) <= {row[f] for row in cc.PARAM_ROWS}, f
    assert any(row["top_yaw"] == row["n_yaw"] for row in cc.PARAM_ROWS)
    assert 2 <= sum(row["n_yaw"] == 3600 for row in cc.PARAM_ROWS) <= 3
    # every cell_px of the sweep has every pair of the sweep
    for cp in cc.CELL_PX:
        for q, d in cc.SWEEP_PAIRS:
            assert "%s:%d" % (q, cp) in cc.GRID_CASES and "%s:%d" % (d, cp) in cc.GRID_CASES


def test_the_table_holds_the_sizes_and_edges_it_names():
    count = lambda name: len(cc.grid_numpy(*[cc.grid_case(name)[k] for k in ("img", "ox", "oy", "res", "cell_px")])[0])
    assert [count("cells%d:1" % n) for n in (4096, 4097, 10000)] == [4096, 4097, 10000]
    assert count("one:2") == 1 and count("empty:2") == 0 and count("n15:3") == 15 and count("n16:3") == 16
    for cp in (1, 3):
        cells = cc.grid_numpy(*[cc.grid_case("border:%d" % cp)[k] for k in ("img", "ox", "oy", "res", "cell_px")])[0]
        assert set(cc.BORDER) <= set((cells & 0xFFFF).tolist()) and set(cc.BORDER) <= set((cells >> 16).tolist())
    over = cc.grid_case("oversize:1")
    cells = cc.grid_numpy(over["img"], over["ox"], over["oy"], over["res"], 1)[0]
    assert len(cells) < np.count_nonzero(over["img"] < 100)            # pixels were dropped
    assert cells[0] == 0 and cells[-1] == (511 << 16 | 511)           # and the grid's corners are kept
    thr = cc.grid_case("threshold:2")["img"]
    assert (thr == 99).any() and (thr == 100).any()


@pytest.mark.parametrize("name", sorted(cc.GRID_CASES))
def test_grid_equals_the_numpy_statement(oracle_mod, name):
    case = cc.grid_case(name)
    cells, _ = cc.grid_numpy(case["img"], case["ox"], case["oy"], case["res"], case["cell_px"])
    if case["want"] is not None:                                         # the builder made the cells it was asked for
        assert np.array_equal(cells, case["want"]), name
    got = _grid(oracle_mod, case).cells()
    assert got.dtype == cells.dtype and np.array_equal(got, cells), name


@pytest.mark.parametrize("name", sorted(cc.GRID_CASES))
def test_dilation_through_the_public_result(oracle_mod, name):
    """The probe holds every cell within one cell of the grid's cells, the halo every cell two away: matched with one rotation, no
    lag and one shift, the overlap is the number of their cells on the dilated map -- all of the probe, none of the halo."""
    case = cc.grid_case(name)
    cp = case["cell_px"]
    cells, dil = cc.grid_numpy(case["img"], case["ox"], case["oy"], case["res"], cp)
    d = _grid(oracle_mod, case)
    for which, pattern in zip(("probe", "halo"), cc.probe_patterns(cells)):
        pc = cc.case_of_pattern(pattern, cp, 5)
        q_cells = cc.grid_numpy(pc["img"], pc["ox"], pc["oy"], pc["res"], cp)[0]
        assert np.array_equal(q_cells, cc.pack(pattern))
        want = cc.overlap_numpy(q_cells, dil, 0, 1, 0, 0, cp)
        assert want == (len(q_cells) if which == "probe" else 0), (name, which)
        assert np.count_nonzero(dil) == len(cc.probe_patterns(cells)[0])
        r = _match(oracle_mod, _grid(oracle_mod, pc), d, cc.PROBE_PARAMS)
        assert r["overlap"] == want and r["k"] == 0 and (r["xy_yaw"] == 0).all(), (name, which, r, want)


def _yaw_error(yaw, turns):
    return abs((yaw - turns * np.pi / 2 + np.pi) % (2 * np.pi) - np.pi)


@pytest.mark.parametrize("kid,cell_px,prm,turns,shift", cc.known_cases(), ids=[k[0] for k in cc.known_cases()])
def test_known_answers(oracle_mod, kid, cell_px, prm, turns, shift):
    qc, dc = cc.known_pair(cell_px, turns, shift)
    q_cells = cc.grid_numpy(qc["img"], qc["ox"], qc["oy"], qc["res"], cell_px)[0]
    r = _match(oracle_mod, _grid(oracle_mod, qc), _grid(oracle_mod, dc), prm)
    assert 250 <= len(q_cells) <= 350
    assert r["overlap"] == len(q_cells) and r["ok"], r
    n_yaw = prm["n_yaw"]
    if n_yaw in (1, 4, 8, 360):
        assert r["k"] == turns * n_yaw // 4, r
    elif n_yaw == 3600:
        # one cell of dilation plus half a cell of rounding, seen from the farthest query cell
        r_max = np.sqrt((cc.unpack(q_cells).astype(np.float64) ** 2).sum(1).max())
        assert _yaw_error(float(r["xy_yaw"][2]), turns) <= 1.5 / r_max, r
    cell_m = np.float32(cell_px) * np.float32(qc["res"])
    t = np.rint(r["xy_yaw"][:2].astype(np.float64) / float(cell_m))
    assert abs(t[0] - shift[0]) <= 1 and abs(t[1] - shift[1]) <= 1, (r, shift)
    assert abs(r["scale"] - 1.0) < 0.02, r


@pytest.mark.parametrize("cell_px", cc.CELL_PX)
def test_rule_pair_keeps_the_identity_up_to_1p2(oracle_mod, cell_px):
    for n, k, overlap in ((12, 0, 10), (13, 1, 13)):                    # 12 * 5 is not greater than 10 * 6; 13 * 5 is
        qc, dc = cc.rule_pair(n, cell_px)
        q_cells = cc.grid_numpy(qc["img"], qc["ox"], qc["oy"], qc["res"], cell_px)[0]
        dil = cc.grid_numpy(dc["img"], dc["ox"], dc["oy"], dc["res"], cell_px)[1]
        assert len(q_cells) == 10 + n
        # the construction, by the numpy statement: the identity overlaps P1 only, the quarter turn P2 only
        assert [cc.overlap_numpy(q_cells, dil, kk, 4, 0, 0, cell_px) for kk in range(4)] == [10, n, 0, 0]
        r = _match(oracle_mod, _grid(oracle_mod, qc), _grid(oracle_mod, dc), cc.RULE_PARAMS)
        assert (r["k"], r["overlap"], r["ok"]) == (k, overlap, True), (n, r)


@pytest.mark.parametrize("cell_px", cc.CELL_PX)
@pytest.mark.parametrize("name", sorted(cc.EDGE_PAIRS))
def test_acceptance_edges(oracle_mod, name, cell_px):
    nq, _, overlap, ok = cc.EDGE_PAIRS[name]
    qc, dc = cc.edge_pair(name, cell_px)
    q_cells = cc.grid_numpy(qc["img"], qc["ox"], qc["oy"], qc["res"], cell_px)[0]
    dil = cc.grid_numpy(dc["img"], dc["ox"], dc["oy"], dc["res"], cell_px)[1]
    assert len(q_cells) == nq and cc.overlap_numpy(q_cells, dil, 0, 1, 0, 0, cell_px) == overlap
    r = _match(oracle_mod, _grid(oracle_mod, qc), _grid(oracle_mod, dc), cc.EDGE_PARAMS)
    assert r["overlap"] == overlap and r["ok"] == ok and r["scale"] == 1.0, r
    assert np.float32(r["ratio"]) == np.float32(overlap) / np.float32(nq)


@pytest.mark.parametrize("cell_px", cc.CELL_PX)
def test_stretched_query_is_withdrawn_at_the_end_of_the_scale_range(oracle_mod, cell_px):
    qc, dc = cc.stretch_pair(1.3, cell_px)
    r = _match(oracle_mod, _grid(oracle_mod, qc), _grid(oracle_mod, dc), cc.STRETCH_PARAMS)
    assert np.float32(r["scale"]) == np.float32(0.88) and not r["ok"], r          # min_overlap = 0: only the scale withdraws it
    qc, dc = cc.stretch_pair(1.0, cell_px)                                          # unstretched: the same pair is accepted
    same = _match(oracle_mod, _grid(oracle_mod, qc), _grid(oracle_mod, dc), cc.STRETCH_PARAMS)
    assert same["ok"] and same["overlap"] == len(_grid(oracle_mod, qc).cells()) and abs(same["scale"] - 1.0) < 0.1, same


def test_window_search_of_the_numpy_statement_agrees_on_ties(oracle_mod):
    """Symmetric patterns, where most shifts tie: with the identity alone the restatement's (overlap, shift) is the first largest
    of the numpy statement's window in row-major order."""
    for cp in cc.CELL_PX:
        for a in cc.SYMMETRIC:
            for b in cc.SYMMETRIC:
                qc, dc = cc.grid_case("%s:%d" % (a, cp)), cc.grid_case("%s:%d" % (b, cp))
                q_cells = cc.grid_numpy(qc["img"], qc["ox"], qc["oy"], qc["res"], cp)[0]
                dil = cc.grid_numpy(dc["img"], dc["ox"], dc["oy"], dc["res"], cp)[1]
                o, tx, ty = cc.best_window(q_cells, dil, 0, 1, 0, 0, 2, cp)
                r = _match(oracle_mod, _grid(oracle_mod, qc), _grid(oracle_mod, dc), dict(n_yaw=1, max_shift=0, top_yaw=0, refine=2,
                                                                                 min_overlap=0.25))
                cell_m = np.float32(cp) * np.float32(qc["res"])
                assert r["overlap"] == o and r["xy_yaw"][0] == np.float32(tx) * cell_m and r["xy_yaw"][1] == np.float32(ty) * cell_m
