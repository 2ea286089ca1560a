"""CPU: the C ABI of the evaluation of registered pairs (gloc_reg_evaluate_pairs, gloc_eval_default_params) and of the
pair lists' system form (gloc_reg_{p2l,gicp,vgicp}_pairs_system) -- symbols, the default, the struct's size, and the
refusals before the handle in their order: the parameter block, the arrays, n, and only then the null handle."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_eval_default_params", "gloc_reg_evaluate_pairs", "gloc_reg_p2l_pairs_system", "gloc_reg_gicp_pairs_system",
       "gloc_reg_vgicp_pairs_system")
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)
METHODS = ("p2l", "gicp", "vgicp")


def _err(L):
    L.gloc_last_error.restype = C.c_char_p
    return L.gloc_last_error()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _evaluate(capi, prm="default", src=True, tgt=True, outs=(0, 1, 2, 3, 4), n=1):
    """gloc_reg_evaluate_pairs with a null handle: (return code, message).  outs: which of the five outputs are given."""
    L = capi.lib()
    ids = np.zeros(1, np.uint32)
    bufs = [np.full(1, 7.0, np.float32), np.full(1, 7.0, np.float32), np.full(1, 77, np.uint32), np.full(36, 7.0), np.full(6, 7.0)]
    if isinstance(prm, str):
        prm = capi.default_eval_params()
    rc = L.gloc_reg_evaluate_pairs(None, _ptr(ids) if src else None, _ptr(ids) if tgt else None, n, None, None if prm is None else C.byref(prm),
                                   *[_ptr(b) if k in outs else None for k, b in enumerate(bufs)])
    assert all((b == (77 if b.dtype == np.uint32 else 7.0)).all() for b in bufs)        # a refused call leaves the outputs alone
    return rc, _err(L)


def _system(capi, method, prm=None, rb=None, src=True, tgt=True, out=True, n=1):
    """gloc_reg_<m>_pairs_system with a null handle: (return code, message)."""
    L = capi.lib()
    ids = np.zeros(1, np.uint32)
    H, g, s, c, w = np.full(36, 7.0), np.full(6, 7.0), np.full(1, 7.0), np.full(1, 77, np.uint64), np.full(1, 7.0)
    prm = prm or getattr(capi, "default_%s_params" % method)()
    rc = getattr(L, "gloc_reg_%s_pairs_system" % method)(None, _ptr(ids) if src else None, _ptr(ids) if tgt else None, n, None, C.byref(prm),
                                                         None if rb is None else C.byref(rb), 0, _ptr(H) if out else None, _ptr(g), _ptr(s),
                                                         _ptr(c), _ptr(w))
    assert (H == 7.0).all() and (g == 7.0).all() and (s == 7.0).all() and (c == 77).all() and (w == 7.0).all()
    return rc, _err(L)


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_default_and_size(capi):
    p = capi.default_eval_params()
    assert p.max_corr_dist == np.float32(0.6) and p.reserved_ == 0
    assert C.sizeof(capi.EvalParams) == 8 and capi.EvalParams.reserved_.offset == 4
    assert capi.default_eval_params(max_corr_dist=2.0).max_corr_dist == 2.0
    capi.lib().gloc_eval_default_params(None)                    # a null block is ignored


@pytest.mark.parametrize("value", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_max_corr_dist_is_refused_before_the_handle(capi, value):
    """... with everything behind it wrong as well: null arrays, no output, n = 0."""
    rc, msg = _evaluate(capi, prm=capi.default_eval_params(max_corr_dist=value), src=False, tgt=False, outs=(), n=0)
    assert rc == INV and b"max_corr_dist" in msg, msg


def test_refused_arguments_in_their_order(capi):
    rc, msg = _evaluate(capi, prm=None, src=False, outs=(), n=0)
    assert rc == INV and b"params is null" in msg, msg
    for kw in (dict(src=False), dict(tgt=False), dict(src=False, tgt=False)):
        rc, msg = _evaluate(capi, outs=(), n=0, **kw)
        assert rc == INV and b"scan ids" in msg, msg
    rc, msg = _evaluate(capi, outs=(), n=0)
    assert rc == INV and b"every output is null" in msg, msg
    for n in (0, 4097):
        rc, msg = _evaluate(capi, n=n)
        assert rc == INV and b"outside [1, 4096]" in msg and b"null argument" not in msg, msg
    for outs in ((0, 1, 2, 3, 4), (0,), (1,), (2,), (3,), (4,)):         # one output is enough; the edge of n is inside
        rc, msg = _evaluate(capi, outs=outs, n=4096)
        assert rc == INV and b"null argument" in msg, msg                # the handle's refusal, the last


@pytest.mark.parametrize("method", METHODS)
def test_list_systems_refuse_bad_blocks_before_the_handle(capi, method):
    """As gloc_reg_<m>_pairs: the method's block, the robust block, the arrays and n, then the null handle."""
    wrong = dict(src=False, tgt=False, out=False, n=0)
    rc, msg = _system(capi, method, prm=getattr(capi, "default_%s_params" % method)(max_iters=0), rb=capi.default_robust_params(kind=9), **wrong)
    assert rc == INV and b"max_iters" in msg, msg
    bad, field = {"p2l": (capi.default_p2l_params(normal_k=2), b"normal_k"), "gicp": (capi.default_gicp_params(plane_eps=0.0), b"plane_eps"),
                  "vgicp": (capi.default_vgicp_params(neighbors=5), b"neighbors")}[method]
    rc, msg = _system(capi, method, prm=bad, **wrong)
    assert rc == INV and field in msg, msg
    rc, msg = _system(capi, method, rb=capi.default_robust_params(kind=9), **wrong)
    assert rc == INV and b"kind" in msg, msg
    rc, msg = _system(capi, method, rb=capi.default_robust_params(kind=2, scale=0.0), **wrong)
    assert rc == INV and b"scale" in msg, msg
    for rb in (None, capi.default_robust_params(kind=2, scale=1.0)):
        rc, msg = _system(capi, method, rb=rb, src=False)
        assert rc == INV and b"scan ids" in msg, msg
        rc, msg = _system(capi, method, rb=rb, out=False)
        assert rc == INV and b"null argument" in msg, msg
        for n in (0, 4097):
            rc, msg = _system(capi, method, rb=rb, n=n)
            assert rc == INV and b"outside [1, 4096]" in msg, msg
        rc, msg = _system(capi, method, rb=rb, n=4096)
        assert rc == INV and b"null argument" in msg, msg
