"""CPU: the C ABI of the pose-graph optimisation -- symbols, struct sizes and offsets, defaults, and every refusal, in the
order the header states, with the outputs untouched.  The handle is checked last, so a null one stands in for it: what the
checks let through ends with "null handle"."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_pgo_default_params", "gloc_pgo_create", "gloc_pgo_destroy", "gloc_pgo_set_stream", "gloc_pgo_synchronize", "gloc_pgo_set_profile",
       "gloc_pgo_profile", "gloc_pgo_profile_reset", "gloc_pgo_linearize", "gloc_pgo_optimize")
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)
NAN, INF = float("nan"), float("inf")


def _err(L):
    L.gloc_last_error.restype = C.c_char_p
    return L.gloc_last_error()


def _graph(n=3, m=2):
    P = np.tile(np.eye(4), (n, 1, 1))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    src, tgt = (np.arange(m, dtype=np.uint32) % (n - 1)) + 1, np.zeros(m, np.uint32)
    Z = np.tile(np.eye(4, dtype=np.float32), (m, 1, 1))
    info = np.tile(np.eye(6), (m, 1, 1))
    return dict(P=P, fixed=fixed, src=src, tgt=tgt, Z=Z, info=info, mask=None)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(capi, g, prm, rob=None, entry="optimize", n=None, m=None):
    """(return code, True iff no output was written)."""
    L = capi.lib()
    n = len(g["P"]) if n is None else n
    m = len(g["src"]) if m is None else m
    head = (None, _p(g["P"]), _p(g["fixed"]), n, _p(g["src"]), _p(g["tgt"]), _p(g["Z"]), _p(g["info"]), _p(g["mask"]), m,
            None if prm is None else C.byref(prm), None if rob is None else C.byref(rob))
    if entry == "optimize":
        out, s2, w, res = np.full((4, 16), 7.0), np.full(4, 7.0), np.full(4, 7.0), capi.PgoResult(7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0)
        rc = L.gloc_pgo_optimize(*head, _p(out), _p(s2), _p(w), C.byref(res))
        same = all((a == 7).all() for a in (out, s2, w)) and (res.iters, res.status, res.cost_final) == (7, 7, 7.0)
    else:
        r, s2, w, g6, H, cost = np.full((4, 6), 7.0), np.full(4, 7.0), np.full(4, 7.0), np.full((4, 6), 7.0), np.full((4, 36), 7.0), C.c_double(7.0)
        rc = L.gloc_pgo_linearize(*head, _p(r), _p(s2), _p(w), _p(g6), _p(H), C.byref(cost))
        same = all((a == 7).all() for a in (r, s2, w, g6, H)) and cost.value == 7.0
    return rc, same


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_struct_sizes_and_offsets(capi):
    p, r = capi.PgoParams, capi.PgoResult
    assert C.sizeof(p) == 56
    assert [getattr(p, f).offset for f in ("max_iters", "pcg_max_iters", "lambda_init", "pcg_tol", "rot_eps", "trans_eps", "grad_eps", "reserved_")] == \
        [0, 4, 8, 16, 24, 32, 40, 48]
    assert C.sizeof(r) == 48
    assert [getattr(r, f).offset for f in ("iters", "accepted", "pcg_iters", "status", "cost_initial", "cost_final", "lam", "grad_inf")] == \
        [0, 4, 8, 12, 16, 24, 32, 40]


def test_defaults(capi):
    p = capi.default_pgo_params()
    assert (p.max_iters, p.pcg_max_iters, p.lambda_init, p.pcg_tol) == (50, 200, 1e-4, 1e-8)
    assert (p.rot_eps, p.trans_eps, p.grad_eps, list(p.reserved_)) == (1e-6, 1e-6, 1e-6, [0, 0])
    assert capi.default_pgo_params(max_iters=7).max_iters == 7
    capi.lib().gloc_pgo_default_params(None)               # a null block is ignored


def _res(a, b):
    return (C.c_uint32 * 2)(a, b)


# in the order the entries check them: (parameter fields, word of the message)
PARAM_BAD = [(None, b"null"), (dict(max_iters=0), b"max_iters"), (dict(pcg_max_iters=0), b"pcg_max_iters"),
             (dict(lambda_init=0.0), b"lambda_init"), (dict(lambda_init=-1.0), b"lambda_init"), (dict(lambda_init=NAN), b"lambda_init"),
             (dict(lambda_init=INF), b"lambda_init"), (dict(pcg_tol=0.0), b"pcg_tol"), (dict(pcg_tol=NAN), b"pcg_tol"), (dict(pcg_tol=INF), b"pcg_tol"),
             (dict(rot_eps=-1e-9), b"rot_eps"), (dict(rot_eps=NAN), b"rot_eps"), (dict(trans_eps=-1.0), b"trans_eps"), (dict(trans_eps=INF), b"trans_eps"),
             (dict(grad_eps=-1.0), b"grad_eps"), (dict(grad_eps=NAN), b"grad_eps"), (dict(reserved_=_res(1, 0)), b"reserved_"),
             (dict(reserved_=_res(0, 1)), b"reserved_")]


@pytest.mark.parametrize("entry", ["optimize", "linearize"])
@pytest.mark.parametrize("over,word", PARAM_BAD)
def test_parameter_refusals(capi, over, word, entry):
    rc, same = _call(capi, _graph(), None if over is None else capi.default_pgo_params(**over), entry=entry)
    assert rc == INV and word in _err(capi.lib()) and same


ROBUST_BAD = [(dict(kind=9), b"kind"), (dict(kind=2, scale=0.0), b"scale"), (dict(kind=2, scale=NAN), b"scale"),
              (dict(kind=2, scale=1.0, scale_start=0.5, anneal=0.5), b"scale_start"), (dict(kind=2, scale=1.0, scale_start=4.0, anneal=0.5), b"schedule")]


@pytest.mark.parametrize("over,word", ROBUST_BAD)
def test_robust_refusals(capi, over, word):
    rc, same = _call(capi, _graph(), capi.default_pgo_params(), capi.default_robust_params(**over))
    assert rc == INV and word in _err(capi.lib()) and same


def _bad_graphs():
    def g(**kw):
        d = _graph(4, 3)
        for k, v in kw.items():
            if callable(v):
                v(d)
            else:
                d[k] = v
        return d

    def put(name, idx, val):
        def f(d):
            d[name][idx] = val
        return f
    out = [(g(**{k: None}), dict(n=4, m=3), b"null") for k in ("P", "fixed", "src", "tgt", "Z", "info")]
    out += [(g(), dict(n=1), b"nodes"), (g(), dict(n=(1 << 20) + 1), b"nodes"), (g(), dict(m=0), b"edges"), (g(), dict(m=(1 << 22) + 1), b"edges")]
    out += [(g(a=put("src", 1, 4)), {}, b"beyond"), (g(a=put("tgt", 2, 0xFFFFFFFF)), {}, b"beyond"), (g(a=put("src", 2, 0)), {}, b"itself"),
            (g(a=put("fixed", 0, 0)), {}, b"fixed")]
    out += [(g(a=put("P", (3, 1, 2), NAN)), {}, b"pose"), (g(a=put("P", (0, 0, 3), INF)), {}, b"pose"), (g(a=put("Z", (2, 0, 3), NAN)), {}, b"Z of"),
            (g(a=put("info", (1, 5, 5), -INF)), {}, b"info of")]
    return out


@pytest.mark.parametrize("entry", ["optimize", "linearize"])
@pytest.mark.parametrize("case", range(len(_bad_graphs())))
def test_argument_refusals(capi, case, entry):
    g, kw, word = _bad_graphs()[case]
    rc, same = _call(capi, g, capi.default_pgo_params(), entry=entry, **kw)
    assert rc == INV and word in _err(capi.lib()) and same, word


def test_null_outputs_are_refused(capi):
    L, g, prm = capi.lib(), _graph(), capi.default_pgo_params()
    head = (None, _p(g["P"]), _p(g["fixed"]), 3, _p(g["src"]), _p(g["tgt"]), _p(g["Z"]), _p(g["info"]), None, 2, C.byref(prm), None)
    res, out = capi.PgoResult(), np.zeros((3, 16))
    assert L.gloc_pgo_optimize(*head, None, None, None, C.byref(res)) == INV and b"null argument" in _err(L)
    assert L.gloc_pgo_optimize(*head, _p(out), None, None, None) == INV and b"null argument" in _err(L)
    assert L.gloc_pgo_linearize(*head, None, None, None, None, None, None) == INV and b"null argument" in _err(L)
    s2 = np.zeros(2)                                       # any one output is enough: then the handle is looked at
    assert L.gloc_pgo_linearize(*head, None, _p(s2), None, None, None, None) == INV and b"null handle" in _err(L)


def test_the_first_fault_in_the_stated_order_is_the_one_reported(capi):
    L = capi.lib()
    g = _graph(4, 3)
    g["src"][1] = 9                                        # an end beyond the nodes
    g["src"][2] = 0                                        # a self edge
    g["fixed"][0] = 0                                      # no fixed node
    g["P"][2, 0, 0] = NAN
    every = dict(max_iters=0, lambda_init=-1.0, grad_eps=NAN, reserved_=_res(1, 1))
    rob = capi.default_robust_params(kind=2, scale=1.0, scale_start=4.0, anneal=0.5)
    for key, word, mended in (("max_iters", b"max_iters", 5), ("lambda_init", b"lambda_init", 1.0), ("grad_eps", b"grad_eps", 0.0),
                              ("reserved_", b"reserved_", _res(0, 0))):
        rc, same = _call(capi, g, capi.default_pgo_params(**every), rob, n=1, m=0)
        assert rc == INV and word in _err(L) and same, word
        every[key] = mended
    prm = capi.default_pgo_params(**every)
    steps = [(b"schedule", lambda: setattr(rob, "scale_start", 0.0)), (b"nodes", None), (b"edges", None),
             (b"beyond", lambda: g["src"].__setitem__(1, 2)), (b"itself", lambda: g["src"].__setitem__(2, 3)),
             (b"fixed", lambda: g["fixed"].__setitem__(0, 1)), (b"pose", lambda: g["P"].__setitem__((2, 0, 0), 1.0))]
    kw = dict(n=1, m=0)
    for word, mend in steps:
        rc, same = _call(capi, g, prm, rob, **kw)
        assert rc == INV and word in _err(L) and same, word
        if word == b"nodes":
            kw.pop("n")
        elif word == b"edges":
            kw.pop("m")
        else:
            mend()
    rc, same = _call(capi, g, prm, rob)
    assert rc == INV and b"null handle" in _err(L) and same


def test_the_edges_of_the_ranges_are_inside(capi):
    """What the checks let through is refused for the null handle."""
    L = capi.lib()
    for over in (dict(max_iters=1, pcg_max_iters=1), dict(rot_eps=0.0, trans_eps=0.0, grad_eps=0.0), dict(lambda_init=1e-300, pcg_tol=1e300),
                 dict(max_iters=0xFFFFFFFF)):
        rc, same = _call(capi, _graph(), capi.default_pgo_params(**over))
        assert rc == INV and b"null handle" in _err(L) and same
    for rob in (capi.default_robust_params(), capi.default_robust_params(kind=4, scale=1e-30), capi.default_robust_params(kind=0, scale_start=5.0)):
        rc, same = _call(capi, _graph(), capi.default_pgo_params(), rob)
        assert rc == INV and b"null handle" in _err(L) and same
    rc, same = _call(capi, _graph(2, 1), capi.default_pgo_params())                      # the smallest graph
    assert rc == INV and b"null handle" in _err(L) and same
    g = _graph(3, 2)                                                                     # duplicate and opposite edges are legal
    g["src"], g["tgt"] = np.array([1, 1, 0], np.uint32), np.array([0, 0, 1], np.uint32)
    g["Z"], g["info"] = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1)), np.tile(np.eye(6), (3, 1, 1))
    rc, same = _call(capi, g, capi.default_pgo_params())
    assert rc == INV and b"null handle" in _err(L) and same


def test_the_largest_graph_is_inside(capi):
    """n = 2^20 nodes and m = 2^22 edges pass the checks (zero-filled arrays: untouched pages, and zeros are finite)."""
    n, m = 1 << 20, 1 << 22
    g = dict(P=np.zeros((n, 4, 4)), fixed=np.zeros(n, np.uint8), src=np.ones(m, np.uint32), tgt=np.zeros(m, np.uint32),
             Z=np.zeros((m, 4, 4), np.float32), info=np.zeros((m, 6, 6)), mask=None)
    g["fixed"][n - 1] = 1
    g["src"][m - 1], g["tgt"][m - 1] = n - 1, n - 2
    rc, same = _call(capi, g, capi.default_pgo_params())
    assert rc == INV and b"null handle" in _err(capi.lib()) and same
