"""CPU: the C ABI of the pose graph's closure selection (gloc_pgo_consistency) -- symbols, struct size and offsets, defaults,
and every refusal in the order the header states, with the outputs untouched.  The handle is checked last, so a null one
stands in for it: what the checks let through ends with "null handle"."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_pgo_consistency_default_params", "gloc_pgo_consistency")
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)
NAN, INF = float("nan"), float("inf")
OUTS = ("mask", "size", "rank", "ok", "status", "degree", "score", "seeds", "sizes", "s2")


def _err(L):
    L.gloc_last_error.restype = C.c_char_p
    return L.gloc_last_error()


def _case(n=4, L=3):
    P = np.tile(np.eye(4), (n, 1, 1))
    src, tgt = (np.arange(L, dtype=np.uint32) % (n - 1)) + 1, np.zeros(L, np.uint32)
    return dict(P=P, src=src, tgt=tgt, Z=np.tile(np.eye(4, dtype=np.float32), (L, 1, 1)), info=np.tile(np.eye(6), (L, 1, 1)), path=np.arange(n, dtype=np.float64))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(capi, c, prm, n=None, L=None, only=None, handle=None):
    """(return code, True iff no output was written).  only: the outputs that are passed (the others NULL)."""
    lib = capi.lib()
    n = len(c["P"]) if n is None else n
    L = len(c["src"]) if L is None else L
    o = dict(mask=np.full(8, 7, np.uint8), status=np.full(8, 7, np.uint8), degree=np.full(8, 7, np.uint32), score=np.full(8, 7, np.uint64),
             seeds=np.full(1024, 7, np.uint32), sizes=np.full(1024, 7, np.uint32), s2=np.full(64, 7.0))
    sc = dict(size=C.c_uint32(7), rank=C.c_uint32(7), ok=C.c_uint32(7))
    args = []
    for k in OUTS:
        if only is not None and k not in only:
            args.append(None)
        else:
            args.append(C.byref(sc[k]) if k in sc else _p(o[k]))
    rc = lib.gloc_pgo_consistency(handle, _p(c["P"]), n, _p(c["src"]), _p(c["tgt"]), _p(c["Z"]), _p(c["info"]), _p(c["path"]), L,
                                  None if prm is None else C.byref(prm), *args)
    same = all((a == 7).all() for a in o.values()) and all(v.value == 7 for v in sc.values())
    return rc, same


def test_symbols_exported(capi):
    lib = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.gloc_abi_version() == 6


def test_struct_size_and_offsets(capi):
    p = capi.PgoConsistencyParams
    assert C.sizeof(p) == 40
    assert [getattr(p, f).offset for f in ("chi2", "drift_rot", "drift_trans", "n_seeds", "min_clique", "reserved_")] == [0, 8, 16, 24, 28, 32]


def test_defaults(capi):
    p = capi.default_pgo_consistency_params()
    assert (p.chi2, p.drift_rot, p.drift_trans, p.n_seeds, p.min_clique, list(p.reserved_)) == (16.8119, 0.0, 0.0, 64, 2, [0, 0])
    assert capi.default_pgo_consistency_params(n_seeds=7).n_seeds == 7
    capi.lib().gloc_pgo_consistency_default_params(None)               # a null block is ignored


def _res(a, b):
    return (C.c_uint32 * 2)(a, b)


# in the order the entry checks them: (parameter fields, word of the message)
PARAM_BAD = [(None, b"null"), (dict(chi2=0.0), b"chi2"), (dict(chi2=-1.0), b"chi2"), (dict(chi2=NAN), b"chi2"), (dict(chi2=INF), b"chi2"),
             (dict(drift_rot=-1e-9), b"drift_rot"), (dict(drift_rot=NAN), b"drift_rot"), (dict(drift_trans=-1.0), b"drift_trans"),
             (dict(drift_trans=INF), b"drift_trans"), (dict(n_seeds=0), b"n_seeds"), (dict(n_seeds=1025), b"n_seeds"),
             (dict(reserved_=_res(1, 0)), b"reserved_"), (dict(reserved_=_res(0, 1)), b"reserved_")]


@pytest.mark.parametrize("over,word", PARAM_BAD)
def test_parameter_refusals(capi, over, word):
    rc, same = _call(capi, _case(), None if over is None else capi.default_pgo_consistency_params(**over))
    assert rc == INV and word in _err(capi.lib()) and same


def _bad_cases():
    def g(**kw):
        d = _case()
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
    out = [(g(**{k: None}), dict(n=4, L=3), b"null argument") for k in ("P", "src", "tgt", "Z", "info")]
    out += [(g(), dict(only=()), b"null argument")]
    out += [(g(), dict(n=1), b"nodes"), (g(), dict(n=(1 << 20) + 1), b"nodes"), (g(), dict(L=0), b"closures"), (g(), dict(L=16385), b"closures"),
            (g(), dict(L=4097), b"out_s2")]
    out += [(g(a=put("src", 1, 4)), {}, b"beyond"), (g(a=put("tgt", 2, 0xFFFFFFFF)), {}, b"beyond"), (g(a=put("src", 2, 0)), {}, b"itself")]
    out += [(g(a=put("P", (3, 1, 2), NAN)), {}, b"pose"), (g(a=put("P", (0, 0, 3), INF)), {}, b"pose"), (g(a=put("Z", (2, 0, 3), NAN)), {}, b"Z of"),
            (g(a=put("info", (1, 5, 5), -INF)), {}, b"info of"), (g(a=put("path", 3, NAN)), {}, b"path of")]
    return out


@pytest.mark.parametrize("case", range(len(_bad_cases())))
def test_argument_refusals(capi, case):
    c, kw, word = _bad_cases()[case]
    rc, same = _call(capi, c, capi.default_pgo_consistency_params(), **kw)
    assert rc == INV and word in _err(capi.lib()) and same, word


def test_the_first_fault_in_the_stated_order_is_the_one_reported(capi):
    lib = capi.lib()
    c = _case()
    c["src"][1] = 9                                        # an end beyond the nodes
    c["src"][2] = 0                                        # a self edge
    c["P"][2, 0, 0] = NAN
    c["Z"][0, 1, 1] = NAN
    c["info"][0, 1, 1] = NAN
    c["path"][0] = INF
    every = dict(chi2=0.0, drift_rot=-1.0, drift_trans=NAN, n_seeds=0, reserved_=_res(1, 1))
    for key, word, mended in (("chi2", b"chi2", 1.0), ("drift_rot", b"drift_rot", 0.0), ("drift_trans", b"drift_trans", 0.5), ("n_seeds", b"n_seeds", 1024),
                              ("reserved_", b"reserved_", _res(0, 0))):
        rc, same = _call(capi, c, capi.default_pgo_consistency_params(**every), n=1, L=0)
        assert rc == INV and word in _err(lib) and same, word
        every[key] = mended
    prm = capi.default_pgo_consistency_params(**every)
    steps = [(b"nodes", None), (b"closures", None), (b"beyond", lambda: c["src"].__setitem__(1, 2)), (b"itself", lambda: c["src"].__setitem__(2, 3)),
             (b"pose", lambda: c["P"].__setitem__((2, 0, 0), 1.0)), (b"Z of", lambda: c["Z"].__setitem__((0, 1, 1), 1.0)),
             (b"info of", lambda: c["info"].__setitem__((0, 1, 1), 1.0)), (b"path of", lambda: c["path"].__setitem__(0, 0.0))]
    kw = dict(n=1, L=0)
    for word, mend in steps:
        rc, same = _call(capi, c, prm, **kw)
        assert rc == INV and word in _err(lib) and same, word
        if word == b"nodes":
            kw.pop("n")
        elif word == b"closures":
            kw.pop("L")
        else:
            mend()
    rc, same = _call(capi, c, prm)
    assert rc == INV and b"null handle" in _err(lib) and same


def test_the_edges_of_the_ranges_are_inside(capi):
    """What the checks let through is refused for the null handle."""
    lib = capi.lib()
    for over in (dict(chi2=1e-300), dict(chi2=1e300), dict(drift_rot=0.0, drift_trans=0.0), dict(drift_rot=1e300), dict(n_seeds=1), dict(n_seeds=1024),
                 dict(min_clique=0), dict(min_clique=0xFFFFFFFF)):
        rc, same = _call(capi, _case(), capi.default_pgo_consistency_params(**over))
        assert rc == INV and b"null handle" in _err(lib) and same
    for only in OUTS:                                     # any one output is enough
        rc, same = _call(capi, _case(), capi.default_pgo_consistency_params(), only=(only,))
        assert rc == INV and b"null handle" in _err(lib) and same, only
    c = _case(2, 1)                                       # the smallest case; a null path is all zeros
    c["path"] = None
    rc, same = _call(capi, c, capi.default_pgo_consistency_params())
    assert rc == INV and b"null handle" in _err(lib) and same
    c = _case()                                           # duplicate and opposite closures are legal
    c["src"], c["tgt"] = np.array([1, 1, 0], np.uint32), np.array([0, 0, 1], np.uint32)
    rc, same = _call(capi, c, capi.default_pgo_consistency_params())
    assert rc == INV and b"null handle" in _err(lib) and same


def test_the_largest_case_is_inside(capi):
    """n = 2^20 nodes and L = 16384 closures pass the checks without out_s2, L = 4096 with it (zero-filled arrays)."""
    n, L = 1 << 20, 16384
    c = dict(P=np.zeros((n, 4, 4)), src=np.ones(L, np.uint32), tgt=np.zeros(L, np.uint32), Z=np.zeros((L, 4, 4), np.float32), info=np.zeros((L, 6, 6)),
             path=np.zeros(n))
    c["src"][L - 1], c["tgt"][L - 1] = n - 1, n - 2
    rc, same = _call(capi, c, capi.default_pgo_consistency_params(), only=("mask",))
    assert rc == INV and b"null handle" in _err(capi.lib()) and same
    rc, same = _call(capi, c, capi.default_pgo_consistency_params(), L=4096)
    assert rc == INV and b"null handle" in _err(capi.lib()) and same
