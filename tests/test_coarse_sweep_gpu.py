"""GPU: the coarse (x, y, yaw) matcher against its CPU restatement over the case table of tests/coarse_cases.py -- grids,
parameters, ties, acceptance edges, the scan paths, batches and refusals.  Every comparison is exact: integers or float32
bit patterns (tests/test_coarse_cases_cpu.py proves the table itself on the CPU)."""
import numpy as np
import pytest

import coarse_cases as cc
from util import bits

pytestmark = pytest.mark.gpu
SEARCH = ("n_yaw", "max_shift", "top_yaw", "refine", "min_overlap")


class Rig:
    """One matcher of one cell_px (grids remember their cell_px and resolution), the grids it holds by case name, and the
    restatement's grids and results beside them."""

    def __init__(self, capi, oracle_mod, cell_px):
        self.capi, self.oracle, self.cell_px = capi, oracle_mod, cell_px
        self.cm = capi.CoarseMatcher(params=capi.default_coarse_params(resolution=cc.RESOLUTION[cell_px], cell_px=cell_px))
        self.gid, self.og, self.results = {}, {}, {}

    def add(self, name, case=None):
        if name not in self.gid:
            case = case or cc.grid_case(name)
            assert case["cell_px"] == self.cell_px
            self.gid[name] = self.cm.add_image(case["img"], case["ox"], case["oy"], case["res"])
            self.og[name] = self.oracle.CoarseGrid(case["img"], case["ox"], case["oy"], case["res"], self.cell_px)
        return self.gid[name]

    def drop(self, name):
        self.cm.release(self.gid.pop(name))
        del self.og[name]

    def set(self, prm):
        for f in SEARCH:
            setattr(self.cm.params, f, prm[f])

    def expect(self, q, d, prm):
        key = (q, d) + tuple(prm[f] for f in SEARCH)
        if key not in self.results:
            self.results[key] = self.oracle.coarse_match(self.og[q], self.og[d], *[prm[f] for f in SEARCH])
        return self.results[key]

    def device(self, q, d, prm):
        """The four outputs of one match, as bit patterns: (xy_yaw [3], ratio, ok, scale)."""
        self.set(prm)
        xyyaw, ratio, ok = self.cm.match(self.gid[q], [self.gid[d]])
        return bits(xyyaw[0]).copy(), int(bits(ratio)[0]), bool(ok[0]), int(bits(self.cm.last_scale)[0])

    def check(self, q, d, prm):
        """Device == restatement in every bit; returns the restatement's result and the device's overlap (ratio * n_query)."""
        self.add(q), self.add(d)
        o = self.expect(q, d, prm)
        xy, ratio, ok, scale = self.device(q, d, prm)
        what = (q, d, prm, o)
        assert (xy == bits(o["xy_yaw"])).all(), what + (xy.view(np.float32),)
        assert ratio == int(bits(np.float32(o["ratio"]))[0]), what
        assert ok == o["ok"], what
        assert scale == int(bits(np.float32(o["scale"]))[0]), what + (np.uint32(scale).view(np.float32),)
        nq = len(self.og[q].cells())
        return o, int(np.rint(np.float64(np.uint32(ratio).view(np.float32)) * nq))


@pytest.fixture(scope="module")
def rigs(capi, oracle_mod):
    out = {cp: Rig(capi, oracle_mod, cp) for cp in cc.CELL_PX}
    yield out
    for r in out.values():
        r.cm.close()


def _cp(name):
    return int(name.rsplit(":", 1)[1])


# ---- 1. grids ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cc.GRID_CASES))
def test_grid_cells_and_dilation_equal_the_oracle(rigs, name):
    """The border, the dropped pixels, the threshold, the lround halves, negative indices, the cell list's size classes: the same
    cells; and the dilation, seen through a probe of every cell within one cell of the grid's and a halo of those two away."""
    rig = rigs[_cp(name)]
    rig.add(name)
    cells = rig.og[name].cells()
    got = rig.cm.cells(rig.gid[name])
    assert got.shape == cells.shape and (np.sort(got) == cells).all()
    for which, pattern in zip(("probe", "halo"), cc.probe_patterns(cells)):
        pname = "%s/%s" % (which, name)
        rig.add(pname, cc.case_of_pattern(pattern, rig.cell_px, 5))
        assert (np.sort(rig.cm.cells(rig.gid[pname])) == cc.pack(pattern)).all()
        o, overlap = rig.check(pname, name, cc.PROBE_PARAMS)
        assert overlap == o["overlap"] == (len(pattern) if which == "probe" else 0), (name, which)
        rig.drop(pname)


# ---- 2. parameters -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", cc.SWEEP_PAIRS, ids=["-".join(p) for p in cc.SWEEP_PAIRS])
@pytest.mark.parametrize("row", cc.PARAM_ROWS, ids=[cc.row_id(r) for r in cc.PARAM_ROWS])
def test_parameter_sweep(rigs, row, pair):
    rig = rigs[row["cell_px"]]
    rig.check("%s:%d" % (pair[0], row["cell_px"]), "%s:%d" % (pair[1], row["cell_px"]), row)


@pytest.mark.parametrize("cell_px", (2, 3))
def test_n_yaw_changes_on_a_live_handle(rigs, cell_px):
    """The cos / sin table is cached by n_yaw: 360, 7, 360, 3600, 64 and back on one handle, every step against the restatement."""
    rig = rigs[cell_px]
    q, d = "lshape:%d" % cell_px, "lshape_turned:%d" % cell_px
    for n_yaw in (360, 7, 360, 3600, 64, 360, 1, 8):
        o, overlap = rig.check(q, d, dict(n_yaw=n_yaw, max_shift=5, top_yaw=min(12, n_yaw), refine=2, min_overlap=0.25))
        if n_yaw % 4 == 0:                              # the quarter turn is one of the rotations: it is found
            assert overlap == len(rig.og[q].cells())
            assert o["k"] == n_yaw // 4 or n_yaw == 3600     # (at 0.1 degrees the dilation ties neighbouring rotations)


# ---- 3. ties and rules ---------------------------------------------------------------------------------------------------

TIE_PARAMS = (dict(cc.DEFAULTS), dict(cc.DEFAULTS, n_yaw=8, max_shift=255, top_yaw=1, refine=8),
              dict(cc.DEFAULTS, n_yaw=64, max_shift=64, top_yaw=3, refine=0))


@pytest.mark.parametrize("cell_px", cc.CELL_PX)
def test_symmetric_patterns_tie_as_the_oracle_says(rigs, cell_px):
    """Squares, plus signs and stripes against themselves and each other, near (the identity reaches them) and far (only the rotation
    candidates do: four rotations tie on a quarter-turn symmetry, the lags tie on a period)."""
    rig = rigs[cell_px]
    for prm in TIE_PARAMS:
        for a in cc.SYMMETRIC:
            for b in cc.SYMMETRIC + cc.SYMMETRIC_FAR:
                rig.check("%s:%d" % (a, cell_px), "%s:%d" % (b, cell_px), prm)


@pytest.mark.parametrize("cell_px", cc.CELL_PX)
def test_known_answers_on_the_device(rigs, cell_px):
    rig = rigs[cell_px]
    for kid, cp, prm, turns, shift in cc.known_cases():
        if cp != cell_px:
            continue
        qn, dn = "known_q:%d" % cp, "known_d%d_%d_%d:%d" % (turns, shift[0], shift[1], cp)
        qc, dc = cc.known_pair(cp, turns, shift)
        rig.add(qn, qc), rig.add(dn, dc)
        o, overlap = rig.check(qn, dn, prm)
        assert overlap == len(rig.cm.cells(rig.gid[qn])) and o["ok"], (kid, o, overlap)


@pytest.mark.parametrize("cell_px", cc.CELL_PX)
def test_rules_and_acceptance_edges(rigs, cell_px):
    rig = rigs[cell_px]
    for n, k in ((12, 0), (13, 1)):                                      # the 1.2 x rule: 12 * 5 <= 10 * 6 < 13 * 5
        qc, dc = cc.rule_pair(n, cell_px)
        q, d = "rule%d_q:%d" % (n, cell_px), "rule%d_d:%d" % (n, cell_px)
        rig.add(q, qc), rig.add(d, dc)
        o, overlap = rig.check(q, d, cc.RULE_PARAMS)
        assert o["k"] == k and overlap == (10 if k == 0 else n)
        rig.check(q, d, dict(cc.RULE_PARAMS, n_yaw=360, top_yaw=12, max_shift=5, refine=2))
    for name, (nq, _, want, ok) in sorted(cc.EDGE_PAIRS.items()):        # n_query 15 / 16, overlap at and below min_overlap * n_query
        qc, dc = cc.edge_pair(name, cell_px)
        q, d = "%s_q:%d" % (name, cell_px), "%s_d:%d" % (name, cell_px)
        rig.add(q, qc), rig.add(d, dc)
        o, overlap = rig.check(q, d, cc.EDGE_PARAMS)
        assert overlap == want and o["ok"] == ok
        rig.check(q, d, dict(cc.EDGE_PARAMS, min_overlap=0.0))
        rig.check(q, d, cc.DEFAULTS)
    for f in (1.3, 1.0):                                                 # the stretched query: the scale at the end of its range
        qc, dc = cc.stretch_pair(f, cell_px)
        q, d = "stretch%g_q:%d" % (f, cell_px), "stretch_d:%d" % cell_px
        rig.add(q, qc), rig.add(d, dc)
        o, _ = rig.check(q, d, cc.STRETCH_PARAMS)
        assert o["ok"] == (f == 1.0)


@pytest.mark.parametrize("cell_px", cc.CELL_PX)
def test_empty_and_one_cell_grids(rigs, cell_px):
    rig = rigs[cell_px]
    e, one, other = "empty:%d" % cell_px, "one:%d" % cell_px, "random:%d" % cell_px
    for prm in (cc.DEFAULTS, dict(cc.DEFAULTS, n_yaw=65, max_shift=255, top_yaw=64, refine=8, min_overlap=0.0),
                dict(cc.DEFAULTS, n_yaw=1, max_shift=0, top_yaw=0, refine=0, min_overlap=0.0)):
        for q, d in ((e, other), (other, e), (e, e), (one, other), (other, one), (one, one), (one, e)):
            o, _ = rig.check(q, d, prm)
            assert not o["ok"] or q == other


# ---- 4. scan paths off the defaults --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_scan():
    from gloc3d_amd import synth
    scan = synth.lidar_scan(synth.make_world(1001), None, seed=4, n_az=300)
    assert scan.shape[1] == 4 and 5000 < scan.shape[0] <= 20000
    return scan


@pytest.mark.parametrize("resolution,cell_px", [(0.5, 1), (0.1, 4)])
def test_scan_paths_off_the_defaults(capi, oracle_mod, small_scan, resolution, cell_px):
    img, info = oracle_mod.bev_project(small_scan, resolution=resolution)
    want = oracle_mod.CoarseGrid(img, info["ox"], info["oy"], info["resolution"], cell_px).cells()
    assert len(want) > 100
    cm = capi.CoarseMatcher(params=capi.default_coarse_params(resolution=resolution, cell_px=cell_px))
    store = capi.ScanStore()
    try:
        for scan in (small_scan, np.ascontiguousarray(small_scan[:, :3])):       # (x, y, z, intensity) rows and (x, y, z) rows
            sid = store.add(scan)
            gids = [cm.add_scan(scan), cm.add_store_scan(store, sid)] + list(cm.add_store_scans(store, [sid, sid]))
            for g in gids:
                assert (np.sort(cm.cells(g)) == want).all()
        # a resolution the BEV projector refuses is refused by every scan path alike, and the handle goes on working
        bev = capi.BevProjector()
        with pytest.raises(capi.GlocError):
            bev.project(small_scan, capi.default_bev_params(resolution=0.02))
        bev.close()
        cm.params.resolution = 0.02
        for call in (lambda: cm.add_scan(small_scan), lambda: cm.add_store_scan(store, sid), lambda: cm.add_store_scans(store, [sid, sid])):
            with pytest.raises(capi.GlocError):
                call()
        cm.params.resolution = resolution
        assert (np.sort(cm.cells(cm.add_scan(small_scan))) == want).all()
        assert (np.sort(cm.cells(cm.add_store_scan(store, sid))) == want).all()
    finally:
        store.close()
        cm.close()


# ---- 5. batches and re-use -----------------------------------------------------------------------------------------------

def _bits3(res):
    xyyaw, ratio, ok = res
    return bits(xyyaw).copy(), bits(ratio).copy(), np.asarray(ok).copy()


def test_match_pairs_equals_single_matches(rigs):
    rig = rigs[2]
    names = cc.names_of(2)
    for n in names:
        rig.add(n)
    rig.set(cc.DEFAULTS)
    qs = [names[i % len(names)] for i in range(72)]
    ds = [names[(7 * i + 3) % len(names)] for i in range(72)]
    qs[5], ds[5], qs[6], ds[6] = names[0], names[0], "dense:2", "dense:2"  # the same grid as query and database
    qs[40:44], ds[40:44] = qs[10:14], ds[10:14]                          # repeated pairs
    assert sum(q == d for q, d in zip(qs, ds)) >= 2 and set(qs) == set(names)
    xy, ratio, ok = _bits3(rig.cm.match_pairs([rig.gid[q] for q in qs], [rig.gid[d] for d in ds]))
    scale = bits(rig.cm.last_scale).copy()
    for j, (q, d) in enumerate(zip(qs, ds)):
        x1, r1, ok1, s1 = rig.device(q, d, cc.DEFAULTS)
        assert (xy[j] == x1).all() and ratio[j] == r1 and bool(ok[j]) == ok1 and scale[j] == s1, (j, q, d)
    # one query against the same database id listed several times: equal rows
    d = rig.gid["random2:2"]
    xy, ratio, ok = _bits3(rig.cm.match(rig.gid["random:2"], [d, rig.gid["dense:2"], d, d]))
    scale = bits(rig.cm.last_scale)
    for j in (2, 3):
        assert (xy[j] == xy[0]).all() and ratio[j] == ratio[0] and ok[j] == ok[0] and scale[j] == scale[0]
    assert (xy[1] != xy[0]).any() or ratio[1] != ratio[0]


def test_results_survive_release_and_reuse_of_pooled_blocks(capi, oracle_mod):
    rig = Rig(capi, oracle_mod, 2)
    try:
        rows = (cc.PARAM_ROWS[0], cc.PARAM_ROWS[4], cc.PARAM_ROWS[9])
        assert all(r["cell_px"] == 2 for r in rows)
        pairs = [("%s:2" % q, "%s:2" % d) for q, d in cc.SWEEP_PAIRS]
        for q, d in pairs:
            rig.add(q), rig.add(d)
        before = {(q, d, cc.row_id(r)): rig.device(q, d, r) for r in rows for q, d in pairs}
        for r in rows:
            for q, d in pairs:
                rig.check(q, d, r)
        old_ids = set(rig.gid.values())
        for n in list(rig.gid):                                          # release every grid ...
            rig.drop(n)
        # ... and hand the pooled blocks out again: a dense grid (two size classes of cells), a sparse one, a dense one
        order = ["dense:2", "random2:2", "dense_again:2"]
        rig.add("dense:2"), rig.add("random2:2"), rig.add("dense_again:2", cc.grid_case("dense:2"))
        assert {rig.gid[n] for n in order} <= old_ids                    # ids are re-used
        for n in order:
            assert (np.sort(rig.cm.cells(rig.gid[n])) == rig.og[n].cells()).all()
        for q, d in pairs:
            rig.add(q), rig.add(d)
        for r in rows:
            for q, d in pairs:
                got = rig.device(q, d, r)
                want = before[(q, d, cc.row_id(r))]
                assert (got[0] == want[0]).all() and got[1:] == want[1:], (q, d, r)
            got, want = rig.device("random2:2", "dense_again:2", r), before[("random2:2", "dense:2", cc.row_id(r))]
            assert (got[0] == want[0]).all() and got[1:] == want[1:], r
    finally:
        rig.cm.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

BAD_PARAMS = (dict(cell_px=0), dict(cell_px=17), dict(n_yaw=0), dict(n_yaw=3601), dict(max_shift=256), dict(top_yaw=65),
              dict(n_yaw=7, top_yaw=8), dict(refine=9))


def test_refusals_leave_the_handle_usable(capi, oracle_mod):
    rig = Rig(capi, oracle_mod, 2)
    cm = rig.cm
    try:
        q, d = rig.add("random:2"), rig.add("lshape:2")
        case = cc.grid_case("one:2")
        want = rig.device("random:2", "lshape:2", cc.DEFAULTS)

        def usable():
            got = rig.device("random:2", "lshape:2", cc.DEFAULTS)
            assert (got[0] == want[0]).all() and got[1:] == want[1:]

        for bad in BAD_PARAMS:
            keep = {f: getattr(cm.params, f) for f in bad}
            for f, v in bad.items():
                setattr(cm.params, f, v)
            with pytest.raises(capi.GlocError):
                cm.match(q, [d])
            with pytest.raises(capi.GlocError):
                cm.match_pairs([q], [d])
            with pytest.raises(capi.GlocError):
                cm.add_image(case["img"], case["ox"], case["oy"], case["res"])
            for f, v in keep.items():
                setattr(cm.params, f, v)
            usable()
        with pytest.raises(capi.GlocError):                                  # an image of another resolution than the parameters'
            cm.add_image(case["img"], case["ox"], case["oy"], 0.25)
        usable()
        for f, v in (("cell_px", 3), ("resolution", 0.25)):                  # parameters that differ from the grids'
            keep = getattr(cm.params, f)
            setattr(cm.params, f, v)
            with pytest.raises(capi.GlocError):
                cm.match(q, [d])
            with pytest.raises(capi.GlocError):
                cm.match_pairs([d], [q])
            setattr(cm.params, f, keep)
            usable()
        gone = cm.add_image(case["img"], case["ox"], case["oy"], case["res"])
        cm.release(gone)
        for call in (lambda: cm.match(gone, [d]), lambda: cm.match(q, [d, gone]), lambda: cm.cells(gone), lambda: cm.release(gone)):
            with pytest.raises(capi.GlocError):                              # a released grid id
                call()
        usable()
        for call in (lambda: cm.match(q, []), lambda: cm.match_pairs([], [])):
            with pytest.raises(capi.GlocError):                              # zero pairs
                call()
        usable()
        rig.check("random:2", "lshape:2", cc.DEFAULTS)
    finally:
        cm.close()
