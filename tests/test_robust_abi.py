"""CPU: the C ABI of the robust weighting -- symbols, struct size and offsets, defaults, refusals before the handle."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_robust_default_params", "gloc_robust_scale", "gloc_robust_weight", "gloc_reg_p2l_batch_ids_robust",
       "gloc_reg_gicp_batch_ids_robust", "gloc_reg_vgicp_batch_ids_robust", "gloc_reg_p2l_system_robust", "gloc_reg_gicp_system_robust",
       "gloc_reg_vgicp_system_robust")
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)
NAN, INF = float("nan"), float("inf")
TINY = float(np.nextafter(np.float32(0), np.float32(1)))                 # the smallest float32 above 0
BELOW_1 = float(np.nextafter(np.float32(1), np.float32(0)))              # the largest below 1
# (field the message names, the block): every kind but NONE refuses them
BAD = [("scale", dict(scale=0.0)), ("scale", dict(scale=-1.0)), ("scale", dict(scale=NAN)), ("scale", dict(scale=INF)),
       ("scale_start", dict(scale=1.0, scale_start=-1.0, anneal=0.5)), ("scale_start", dict(scale=1.0, scale_start=NAN, anneal=0.5)),
       ("scale_start", dict(scale=1.0, scale_start=INF, anneal=0.5)), ("scale_start", dict(scale=1.0, scale_start=0.5, anneal=0.5)),
       ("scale_start", dict(scale=1.0, scale_start=BELOW_1, anneal=0.5)),
       ("anneal", dict(scale=1.0, scale_start=2.0, anneal=0.0)), ("anneal", dict(scale=1.0, scale_start=2.0, anneal=1.0)),
       ("anneal", dict(scale=1.0, scale_start=2.0, anneal=-0.5)), ("anneal", dict(scale=1.0, scale_start=2.0, anneal=1.5)),
       ("anneal", dict(scale=1.0, scale_start=2.0, anneal=NAN))]


def _err(L):
    L.gloc_last_error.restype = C.c_char_p
    return L.gloc_last_error()


def _entries(capi, rb, p2l=None, gicp=None, vgicp=None, pass_=0):
    """The six entries with a null handle: [(name, return code, message)].  rb: a RobustParams or None (a null block)."""
    L = capi.lib()
    T, ids = np.empty(16, np.float32), np.zeros(1, np.uint32)
    tp, ip = T.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)
    H, g = np.empty(36), np.empty(6)
    hp, gp = H.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p)
    s, c, w = C.c_double(), C.c_uint64(), C.c_double()
    r = None if rb is None else C.byref(rb)
    out = []
    for m, prm in (("p2l", p2l or capi.default_p2l_params()), ("gicp", gicp or capi.default_gicp_params()),
                   ("vgicp", vgicp or capi.default_vgicp_params())):
        rc = getattr(L, "gloc_reg_%s_batch_ids_robust" % m)(None, 0, ip, 1, None, C.byref(prm), r, tp, None, None, None, None)
        out.append((m + "_batch", rc, _err(L)))
        rc = getattr(L, "gloc_reg_%s_system_robust" % m)(None, 0, 0, None, C.byref(prm), r, pass_, hp, gp, C.byref(s), C.byref(c), C.byref(w))
        out.append((m + "_system", rc, _err(L)))
    return out


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_defaults_size_and_offsets(capi):
    p = capi.default_robust_params()
    assert (p.kind, p.scale, p.scale_start, p.anneal) == (0, 0.0, 0.0, 0.0)
    R = capi.RobustParams
    assert C.sizeof(R) == 16 and (R.kind.offset, R.scale.offset, R.scale_start.offset, R.anneal.offset) == (0, 4, 8, 12)
    assert (capi.ROBUST_NONE, capi.ROBUST_HUBER, capi.ROBUST_CAUCHY, capi.ROBUST_TUKEY, capi.ROBUST_GEMAN_MCCLURE) == (0, 1, 2, 3, 4)
    assert capi.default_robust_params(kind=2, scale=0.5).scale == 0.5
    capi.lib().gloc_robust_default_params(None)               # a null block is ignored


def test_a_null_block_and_an_unknown_kind_are_refused(capi):
    for name, rc, msg in _entries(capi, None):
        assert rc == INV and b"robust params" in msg, name
    for kind in (5, 0xFFFFFFFF):
        for name, rc, msg in _entries(capi, capi.default_robust_params(kind=kind, scale=1.0)):
            assert rc == INV and b"kind" in msg, (name, kind)
    L = capi.lib()
    c = C.c_double()
    assert L.gloc_robust_scale(None, 0, C.byref(c)) == INV and b"robust params" in _err(L)
    assert L.gloc_robust_weight(None, 0, 1.0, C.byref(c)) == INV and b"robust params" in _err(L)
    ok = capi.default_robust_params(kind=1, scale=1.0)
    assert L.gloc_robust_scale(C.byref(ok), 0, None) == INV and L.gloc_robust_weight(C.byref(ok), 0, 1.0, None) == INV
    bad = capi.default_robust_params(kind=7, scale=1.0)
    assert L.gloc_robust_scale(C.byref(bad), 0, C.byref(c)) == INV and b"kind" in _err(L)


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
@pytest.mark.parametrize("field,over", BAD)
def test_bad_parameters_are_refused_before_the_handle(capi, kind, field, over):
    rb = capi.default_robust_params(kind=kind, **over)
    for name, rc, msg in _entries(capi, rb, pass_=3):
        assert rc == INV and field.encode() in msg and b"null argument" not in msg, (name, msg)
    L = capi.lib()
    c = C.c_double()
    assert L.gloc_robust_scale(C.byref(rb), 0, C.byref(c)) == INV and field.encode() in _err(L)
    assert L.gloc_robust_weight(C.byref(rb), 0, 1.0, C.byref(c)) == INV and field.encode() in _err(L)


@pytest.mark.parametrize("field,over", BAD)
def test_kind_none_ignores_the_other_fields(capi, field, over):
    """NONE: the other three fields are ignored -- the refusal is the null handle's."""
    for name, rc, msg in _entries(capi, capi.default_robust_params(kind=0, **over)):
        assert rc == INV and b"null argument" in msg, (name, msg)


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_the_edges_of_the_ranges_are_inside(capi, kind):
    """scale_start == scale, anneal just inside both ends, the smallest and the largest scale, a schedule-less block
    whose anneal is anything: they pass the parameter check, and the refusal is then the null handle's."""
    fmax = float(np.finfo(np.float32).max)
    for over in (dict(scale=1.0, scale_start=1.0, anneal=0.5), dict(scale=1.0, scale_start=2.0, anneal=TINY),
                 dict(scale=1.0, scale_start=2.0, anneal=BELOW_1), dict(scale=TINY), dict(scale=fmax), dict(scale=1.0, scale_start=fmax, anneal=0.5),
                 dict(scale=1.0, anneal=7.0), dict(scale=1.0, anneal=NAN)):
        for name, rc, msg in _entries(capi, capi.default_robust_params(kind=kind, **over)):
            assert rc == INV and b"null argument" in msg, (name, over, msg)


def test_the_other_blocks_are_still_checked(capi):
    rb = capi.default_robust_params(kind=2, scale=1.0)
    got = dict((n, m) for n, _, m in _entries(capi, rb, p2l=capi.default_p2l_params(normal_k=2), gicp=capi.default_gicp_params(plane_eps=0.0),
                                              vgicp=capi.default_vgicp_params(neighbors=5)))
    for n in ("p2l_batch", "p2l_system"):
        assert b"normal_k" in got[n]
    for n in ("gicp_batch", "gicp_system"):
        assert b"plane_eps" in got[n]
    for n in ("vgicp_batch", "vgicp_system"):
        assert b"neighbors" in got[n]
    # ... and before the robust block: both bad, the method's own is named
    bad = capi.default_robust_params(kind=9)
    for n, rc, m in _entries(capi, bad, p2l=capi.default_p2l_params(max_iters=0), gicp=capi.default_gicp_params(max_iters=0),
                             vgicp=capi.default_vgicp_params(max_iters=0)):
        assert rc == INV and b"max_iters" in m, n


def test_null_outputs_of_the_system_form(capi):
    """out_weight may be null (it is above); the system form's outputs may not."""
    L = capi.lib()
    rb, prm = capi.default_robust_params(kind=1, scale=1.0), capi.default_p2l_params()
    assert L.gloc_reg_p2l_system_robust(None, 0, 0, None, C.byref(prm), C.byref(rb), 0, None, None, None, None, None) == INV
    assert b"null argument" in _err(L)
