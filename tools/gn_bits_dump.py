"""The outputs of the entries of the three Gauss-Newton refinements (gloc_reg_{p2l,gicp,vgicp}_batch_ids, _system, their
_robust forms and _pairs) as raw bits: one file, to be compared byte for byte between two builds of the library on one
machine -- the check that a change under those entries moved nothing.

    GLOC3D_LIB_PATH=<a build's libgloc3d.so> python tools/gn_bits_dump.py --out FILE

What is run: every case of tests/gn_cases.py CASES (its own method, plain and with a robust block; the generalized ICP cases'
scans and guesses through the voxelized refinement as well), the batches of gn_cases.MIXED as ONE call each (plain and
robust), every case of tests/robust_cases.py CASES, and the system form of each case at its guess.  Through the pair-list
entries: the list of tests/pairs_cases.py under both of its blocks, and a short list of two sources, a repeated target and
a row without a target, each method plain and robust.  The file is a line per call: a label, then the hex of every output
array.  The last line printed is the file's SHA-256."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import gn_cases as GC
    import pairs_cases as PC
    import robust_cases as RC
    import robust_ref as RR
    from gloc3d_amd import capi

    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    ids = {}

    def sid(name):
        if name not in ids:
            xyz = RC.cloud(name)
            ids[name] = store.add(np.ascontiguousarray(xyz, np.float32))
            if len(xyz):
                store.build_normals(ids[name], GC.NORMAL_K)
        return ids[name]

    def prm(method, p):
        p = dict(p)
        if method == "p2l":
            p.pop("plane_eps", None)
        if method == "vgicp":
            p = dict(RC.VGICP, **p)
        return getattr(capi, "default_%s_params" % method)(**p)

    lines = []

    def put(label, out):
        lines.append(label + " " + " ".join(np.ascontiguousarray(o).tobytes().hex() for o in out))

    def both(label, method, src, tgts, init, p):
        for rb in (None, RC.robust(method, RR.CAUCHY, 4.0, 0.5), RC.robust(method, RR.TUKEY)):
            r = None if rb is None else capi.default_robust_params(**rb)
            out = getattr(reg, method + "_batch")(sid(src), [sid(t) for t in tgts], init_T=np.ascontiguousarray(init, np.float32),
                                                  params=prm(method, p), robust=r)
            put("%s %s batch %s" % (label, method, "plain" if rb is None else RR.NAMES[rb["kind"]]), out)
            H, g, s, c = getattr(reg, method + "_system")(sid(src), sid(tgts[0]), np.ascontiguousarray(init[0], np.float32), prm(method, p),
                                                          robust=r, robust_pass=1)[:4]
            put("%s %s system %s" % (label, method, "plain" if rb is None else RR.NAMES[rb["kind"]]), (H, g, np.float64(s), np.uint64(c)))

    for case in GC.CASES:
        both(case["name"], case["method"], case["src"], [case["tgt"]], GC.guess(case)[None], GC.params(case))
        if case["method"] == "gicp":
            both(case["name"], "vgicp", case["src"], [case["tgt"]], GC.guess(case)[None], GC.params(case))
    for method, batches in GC.MIXED.items():
        for names in batches:
            cs = [GC.by_name(n) for n in names]
            init = np.stack([GC.guess(c) for c in cs])
            for m in ((method, "vgicp") if method == "gicp" else (method,)):
                both("mixed_" + names[0], m, cs[0]["src"], [c["tgt"] for c in cs], init, GC.params(cs[0]))
    for case in RC.CASES:
        out = getattr(reg, case["method"] + "_batch")(sid(case["src"]), [sid(case["tgt"])], init_T=RC.guess(case)[None],
                                                      params=prm(case["method"], RC.params(case)),
                                                      robust=capi.default_robust_params(**case["robust"]))
        put("robust_" + case["name"], out)
    # the pair-list entries: the ragged list of pairs_cases, then two sources, a repeated target and a row without one
    short = [("a2", "a0"), ("a3", "a0"), ("a2", None), ("a3", "a1")]
    short_init = np.stack([(GC.truth(s, t or "a0") @ GC._se3(0.5 + 0.25 * j, (0.05, -0.02 * j, 0.01))).astype(np.float32)
                           for j, (s, t) in enumerate(short)])
    lists = [(b, [(q["src"], q["tgt"]) for q in PC.pairs(b)], PC.guesses(PC.pairs(b)), b) for b in PC.BLOCKS] + [("short", short, short_init, "P1")]
    for method in PC.METHODS:
        for label, names, init, block in lists:
            for rb in (None, PC.robust(method)):
                out = getattr(reg, method + "_pairs")([sid(s) for s, _ in names], [None if t is None else sid(t) for _, t in names],
                                                      init_T=np.ascontiguousarray(init, np.float32),
                                                      params=getattr(capi, "default_%s_params" % method)(**PC.params(method, block)),
                                                      robust=None if rb is None else capi.default_robust_params(**rb))
                put("pairs_%s %s %s" % (label, method, "plain" if rb is None else RR.NAMES[rb["kind"]]), out)
    reg.close()
    store.close()
    blob = ("\n".join(lines) + "\n").encode()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "wb") as f:
        f.write(blob)
    print("%d calls, %d bytes" % (len(lines), len(blob)))
    print("sha256 " + hashlib.sha256(blob).hexdigest())


if __name__ == "__main__":
    main()
