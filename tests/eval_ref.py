"""Float64 restatement of the point-to-point evaluation of registered pairs (gloc_reg_evaluate_pairs): the executable
contract of gloc3d_amd/csrc/eval_kernels.hpp, V1 - V6 of include/gloc3d.h.  numpy plus a 1-NN search handed in (the
project's oracle `nn3` behind gn_cases.finite_nn: exact, fp32 un-fused distance, smallest index among equals, no pair for
a non-finite point).

One row at pose T (source -> target):
  V1  p = R s + t in fp32 with the pose rounded to fp32, ((r0 x + r1 y) + r2 z) + t un-fused (p2l_ref.move);
  V2  j = 1-NN of p, d2 the search's fp32 squared distance;
  V3  the pair counts iff d2 is finite and d2 <= max_corr_dist x max_corr_dist, the product in fp32;
  V4  in fp64 from the fp32 values: e = p - q_j, J = [-[p]x , I] (xi = (w, v), rotation first);
      info += J^T J, g += J^T e, sum += (ex ex + ey ey) + ez ez, count += 1;
  V5  fitness = (float)(count / n_src) over ALL source rows, rmse = (float)sqrt(sum / count) or 0, info symmetric.

The sums are kept as the device keeps them: 29 values S_k -- the upper triangle of info row-major (21), g (6), the squared
residual, the count -- each the sum over the pairs of a per-pair value written out below with the device's operations.
Beside every S_k stands A_k, the sum of the absolute values of the products that went into it: what a bound on the
rounding error of any summation order is stated in.
"""
import numpy as np

from p2l_ref import move

NSUM = 29
TRI = [(a, b) for a in range(6) for b in range(a, 6)]      # slot -> (row, column) of the upper triangle


def pairs(src, tgt, T, nn, max_corr_dist):
    """(p, q) float64 [m, 3] of the pairs that count, the mask [n_src] of the source rows they belong to and j [m]."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    p = move(np.eye(4) if T is None else T, src)
    if len(tgt) == 0 or len(src) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(len(src), bool), np.zeros(0, np.int64)
    idx, d2 = nn(p, tgt)
    idx = idx.astype(np.int64)
    g2 = np.float32(max_corr_dist) * np.float32(max_corr_dist)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d2) & (idx < len(tgt)) & (d2 <= g2)
    j = idx[ok]
    return p[ok].astype(np.float64), tgt[j].astype(np.float64), ok, j


def terms(p, q):
    """The pairs' 29 values v [m, 29] and the absolute values a [m, 29] of the products in them, fp64."""
    m = len(p)
    v, a = np.zeros((m, NSUM)), np.zeros((m, NSUM))
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    ex, ey, ez = (p - q).T if m else (np.zeros(0),) * 3

    def put(k, *prods, sign=1.0):
        """v = sign (prods[0] + prods[1] ...): one to three products, added left to right."""
        s = prods[0].copy()
        for t in prods[1:]:
            s = s + t
        v[:, k] = sign * s
        a[:, k] = sum(np.abs(t) for t in prods)

    one = np.ones(m)
    # J^T J with J = [-[p]x , I]: the columns of -[p]x are (0, -pz, py), (pz, 0, -px), (-py, px, 0)
    put(0, py * py, pz * pz)
    put(1, px * py, sign=-1.0)
    put(2, px * pz, sign=-1.0)
    put(4, pz, sign=-1.0)
    put(5, py)
    put(6, px * px, pz * pz)
    put(7, py * pz, sign=-1.0)
    put(8, pz)
    put(10, px, sign=-1.0)
    put(11, px * px, py * py)
    put(12, py, sign=-1.0)
    put(13, px)
    for k in (15, 18, 20, 28):
        put(k, one)
    # J^T e = (p x e, e)
    put(21, py * ez, -(pz * ey))
    put(22, pz * ex, -(px * ez))
    put(23, px * ey, -(py * ex))
    put(24, ex)
    put(25, ey)
    put(26, ez)
    v[:, 27] = (ex * ex + ey * ey) + ez * ez
    a[:, 27] = v[:, 27]
    return v, a


def evaluate(src, tgt, T, nn, max_corr_dist=0.6):
    """One row: dict(count, fitness float32, rmse float32, info [6, 6], g [6], sum, S [29], A [29], mask [n_src], j [count])."""
    n_src = len(np.asarray(src).reshape(-1, 3))
    p, q, ok, j = pairs(src, tgt, T, nn, max_corr_dist)
    v, a = terms(p, q)
    S, A = v.sum(0) + 0.0, a.sum(0)
    count = int(len(p))
    info = np.zeros((6, 6))
    for k, (r, c) in enumerate(TRI):
        info[r, c] = info[c, r] = S[k]
    fitness = np.float32(count / n_src) if count else np.float32(0)
    rmse = np.float32(np.sqrt(S[27] / count)) if count else np.float32(0)
    return dict(count=count, fitness=fitness, rmse=rmse, info=info, g=S[21:27].copy(), sum=float(S[27]), S=S, A=A, mask=ok, j=j)


def sums_of(info, g, s, count):
    """The 29 sums from a row's outputs (info's upper triangle, g, the squared residual, the count)."""
    return np.concatenate([[info[r, c] for r, c in TRI], np.asarray(g, np.float64), [float(s), float(count)]])


def bound(ref):
    """What a row's 29 sums may differ by from `ref`'s: 2 (count + 4) 2^-53 A_k.  The entries of J are fp32 values widened,
    so every product in info is exact in fp64 and a pair's value carries the rounding of one addition at most; a term of g
    or of the squared residual carries at most three roundings (e, the product, the addition).  A sum of n such values in
    any order is off by at most (n - 1) 2^-53 A_k to first order, and this restatement's own sum by no more."""
    return 2.0 * (ref["count"] + 4) * 2.0 ** -53 * ref["A"]
