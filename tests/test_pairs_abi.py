"""CPU: the C ABI of the pair-list entries (gloc_reg_{p2l,gicp,vgicp}_pairs) -- the symbols, and the order of the refusals
before the handle: the method's own block, the robust block, the arrays, n, and only then the null handle."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_reg_p2l_pairs", "gloc_reg_gicp_pairs", "gloc_reg_vgicp_pairs")
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)
METHODS = ("p2l", "gicp", "vgicp")


def _err(L):
    L.gloc_last_error.restype = C.c_char_p
    return L.gloc_last_error()


def _call(capi, method, prm=None, rb=None, src=True, tgt=True, out=True, n=1):
    """The entry with a null handle: (return code, message).  rb: a RobustParams or None (the plain step)."""
    L = capi.lib()
    T, ids = np.full(16, 7.0, np.float32), np.zeros(1, np.uint32)
    ip = ids.ctypes.data_as(C.c_void_p)
    prm = prm or getattr(capi, "default_%s_params" % method)()
    rc = getattr(L, "gloc_reg_%s_pairs" % method)(None, ip if src else None, ip if tgt else None, n, None, C.byref(prm),
                                                  None if rb is None else C.byref(rb), T.ctypes.data_as(C.c_void_p) if out else None,
                                                  None, None, None, None)
    assert (T == 7.0).all()                                 # a refused call leaves the outputs alone
    return rc, _err(L)


def _bad_block(capi, method):
    """(a bad block of the method, the field its refusal names)"""
    return {"p2l": (capi.default_p2l_params(normal_k=2), b"normal_k"), "gicp": (capi.default_gicp_params(plane_eps=0.0), b"plane_eps"),
            "vgicp": (capi.default_vgicp_params(neighbors=5), b"neighbors")}[method]


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


@pytest.mark.parametrize("method", METHODS)
def test_the_null_handle_is_refused_last(capi, method):
    """A good call but for the handle -- with the plain step, with kind NONE and with a kind: the null handle's refusal."""
    for rb in (None, capi.default_robust_params(kind=0, scale=-1.0), capi.default_robust_params(kind=2, scale=1.0, scale_start=4.0, anneal=0.5)):
        rc, msg = _call(capi, method, rb=rb)
        assert rc == INV and b"null argument" in msg, msg


@pytest.mark.parametrize("method", METHODS)
def test_the_methods_block_is_named_first(capi, method):
    """... with everything behind it wrong as well: a bad robust block, null arrays, n = 0."""
    wrong = dict(rb=capi.default_robust_params(kind=9), src=False, tgt=False, out=False, n=0)
    rc, msg = _call(capi, method, prm=getattr(capi, "default_%s_params" % method)(max_iters=0), **wrong)
    assert rc == INV and b"max_iters" in msg, msg
    prm, field = _bad_block(capi, method)
    rc, msg = _call(capi, method, prm=prm, **wrong)
    assert rc == INV and field in msg, msg


@pytest.mark.parametrize("method", METHODS)
def test_then_the_robust_block(capi, method):
    """... before the arrays and n."""
    wrong = dict(src=False, tgt=False, out=False, n=0)
    rc, msg = _call(capi, method, rb=capi.default_robust_params(kind=9), **wrong)
    assert rc == INV and b"kind" in msg, msg
    for kind in (1, 2, 3, 4):
        rc, msg = _call(capi, method, rb=capi.default_robust_params(kind=kind, scale=0.0), **wrong)
        assert rc == INV and b"scale" in msg and b"null" not in msg, msg


@pytest.mark.parametrize("method", METHODS)
def test_then_the_arrays_and_n(capi, method):
    for rb in (None, capi.default_robust_params(kind=2, scale=1.0)):
        for kw in (dict(src=False), dict(tgt=False), dict(src=False, tgt=False)):
            rc, msg = _call(capi, method, rb=rb, **kw)
            assert rc == INV and b"scan ids" in msg, msg
        rc, msg = _call(capi, method, rb=rb, out=False)
        assert rc == INV and b"out_T" in msg, msg
        for n in (0, 4097):
            rc, msg = _call(capi, method, rb=rb, n=n)
            assert rc == INV and b"outside [1, 4096]" in msg and b"null argument" not in msg, msg
        rc, msg = _call(capi, method, rb=rb, n=4096)            # the edge is inside: the handle's refusal
        assert rc == INV and b"null argument" in msg, msg
