"""Developer model (CPU only: numpy + scipy) of what a WARM culled 1-NN pass could still gain from a better starting bound.

A full 20-pass point-to-point ICP of a bench-like pair (synthetic lidar casts of one world, the source 0.9 m resp. 4 m from the
target's pose, started 0.3 m / 1 degree off as the coarse stage hands it over), with the kernel's structure as
tools/sim_culling.py models it: the target in the store's kd order cut into 128-point chunks, 16-point sub-blocks and 4-point
quarters with bounding boxes; the source in Hilbert order, a wave = 128 consecutive sources; per wave the CANDIDATE chunks
(chunk box within the largest bound of the wave's box), swept in chunk order with every source's bound tightening chunk by
chunk; a chunk is PROCESSED when some source's distance to its box is within that source's bound, a (source, sub-block) ITEM
evaluated likewise.  Cost of a wave: the regression of the warm kernel's cycle counter on those counts,

    cycles = 261 candidate + 2796 processed + 33.9 item + 19621.

Per warm pass (2 .. 20) and per starting bound of a source
    previous match   distance to the target point matched in the pass before (what the kernel does)
    its quarter      the nearest of the 4 points of that point's quarter
    its sub-block    the nearest of the 16 points of that point's sub-block
    ideal            the true nearest distance, for free
the mean counts per wave and the modelled cycles; then the sums over the 19 warm passes and what each bound saves against
the previous match, GROSS -- the instructions a tighter bound costs (about +48 VALU per wave for the quarter, +240 for the
sub-block) are not taken off.  Every eighth wave is modelled.

    python tools/sim_warm_bounds.py > profiles/warm_bounds_model.txt      (a few minutes)
"""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gloc3d_amd import synth

PASSES = 20
WAVE_STEP = 8
FAR = 1e18


def hilbert_keys(ix, bits):
    """Skilling's transpose, 3-D; ix [n, 3] uint64 in [0, 2^bits)."""
    X = [ix[:, i].astype(np.uint64).copy() for i in range(3)]
    M = np.uint64(1) << np.uint64(bits - 1)
    Q = M
    while Q > 1:
        P = Q - np.uint64(1)
        for i in range(3):
            m = (X[i] & Q) != 0
            X[0] = np.where(m, X[0] ^ P, X[0])
            t = np.where(m, np.uint64(0), (X[0] ^ X[i]) & P)
            X[0] ^= t
            X[i] ^= t
        Q >>= np.uint64(1)
    X[1] ^= X[0]
    X[2] ^= X[1]
    t = np.zeros_like(X[0])
    Q = M
    while Q > 1:
        t = np.where((X[2] & Q) != 0, t ^ (Q - np.uint64(1)), t)
        Q >>= np.uint64(1)
    for i in range(3):
        X[i] ^= t
    key = np.zeros_like(X[0])
    for b in range(bits):
        for i in range(3):
            key |= ((X[i] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + (2 - i))
    return key


def hilbert_order(P, cell=0.25, bits=10):
    ix = np.clip(np.floor((P - P.min(0)) / cell), 0, (1 << bits) - 1).astype(np.uint64)
    return np.argsort(hilbert_keys(ix, bits), kind="stable")


def store_kd_order(P):
    """The store's kd re-sort: 16 * 2^L positions, every node cut at its middle position along the widest axis of its points."""
    n, L = len(P), 0
    while (16 << L) < n:
        L += 1
    order = np.arange(n)
    for l in range(L):
        size = (16 << L) >> l
        for nd in range(1 << l):
            a = nd * size
            if a >= n:
                break
            b = min(a + size, n)
            pts = P[order[a:b]]
            ax = int(np.argmax(pts.max(0) - pts.min(0)))
            order[a:b] = order[a:b][np.argsort(pts[:, ax], kind="stable")]
    return order


def boxes(P, m):
    return P.reshape(-1, m, 3).min(1), np.where(P.reshape(-1, m, 3) >= FAR, -FAR, P.reshape(-1, m, 3)).max(1)


def lb2(p, lo, hi):
    e = np.maximum(np.maximum(lo[None] - p[:, None], p[:, None] - hi[None]), 0)
    return (e * e).sum(-1)


def kabsch(p, q):
    pc, qc = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((p - pc).T @ (q - qc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, qc - R @ pc


def cycles(cand, proc, items):
    return 261.0 * cand + 2796.0 * proc + 33.9 * items + 19621.0


def model_pair(tag, A, B, T_true):
    n = len(A)
    o = store_kd_order(A)
    inv = np.empty(n, np.int64)
    inv[o] = np.arange(n)
    npad = (n + 127) // 128 * 128
    Tp = np.concatenate([A[o], np.full((npad - n, 3), FAR)])
    clo, chi = boxes(Tp, 128)
    slo, shi = boxes(Tp, 16)
    tree = cKDTree(A)
    S0 = B[hilbert_order(B)]  # the source in its own frame: the waves are the same in every pass
    E = synth.se3(1.0, (0.3, -0.2, 0.02))
    R, t = (E @ T_true)[:3, :3], (E @ T_true)[:3, 3]
    waves = range(0, len(S0) // 128, WAVE_STEP)
    names = ("previous match", "its quarter", "its sub-block", "ideal")
    total = {k: 0.0 for k in names}
    print(f"== {tag}: source {len(S0)} points ({len(S0) // 128} waves, every {WAVE_STEP}th modelled), target {n} points in {npad // 128} chunks")
    print(f"   {'pass':>4} {'moved':>7} | " + " | ".join(f"{k:>14}: cand  proc  items  kcyc" for k in names))
    jprev = None
    for p in range(1, PASSES + 1):
        S = S0 @ R.T + t
        d_true, j = tree.query(S)
        if jprev is not None:
            pos = inv[jprev]
            bounds = {
                "previous match": np.linalg.norm(Tp[pos] - S, axis=1),
                "its quarter": np.linalg.norm(Tp[(pos // 4 * 4)[:, None] + np.arange(4)[None]] - S[:, None], axis=2).min(1),
                "its sub-block": np.linalg.norm(Tp[(pos // 16 * 16)[:, None] + np.arange(16)[None]] - S[:, None], axis=2).min(1),
                "ideal": d_true,
            }
            row = []
            for k in names:
                cand = proc = items = 0
                for wv in waves:
                    s = S[wv * 128:(wv + 1) * 128]
                    b = bounds[k][wv * 128:(wv + 1) * 128] * (1 + 1e-9) + 1e-12
                    wl, wh = s.min(0), s.max(0)
                    e = np.maximum(np.maximum(clo - wh, wl - chi), 0)
                    cs = np.nonzero((e * e).sum(-1) <= b.max() ** 2)[0]
                    cand += len(cs)
                    for c in cs:
                        if not (lb2(s, clo[c:c + 1], chi[c:c + 1])[:, 0] <= b * b).any():
                            continue
                        proc += 1
                        items += int((lb2(s, slo[c * 8:c * 8 + 8], shi[c * 8:c * 8 + 8]) <= (b * b)[:, None]).sum())
                        dd = np.sqrt(((Tp[c * 128:(c + 1) * 128][None] - s[:, None]) ** 2).sum(-1)).min(1)
                        np.minimum(b, dd * (1 + 1e-9) + 1e-12, out=b)
                nw = len(waves)
                cyc = cycles(cand / nw, proc / nw, items / nw)
                total[k] += cyc
                row.append(f"{'':>14}  {cand / nw:5.1f} {proc / nw:5.2f} {items / nw:6.0f} {cyc / 1e3:5.1f}")
            moved = np.linalg.norm(S - Sprev, axis=1).mean()
            print(f"   {p:4d} {moved:7.4f} | " + " | ".join(row))
        # the pass's update: Kabsch on its correspondences
        dR, dt = kabsch(S, A[j])
        R, t = dR @ R, dR @ t + dt
        jprev, Sprev = j, S
    base = total["previous match"]
    print("   warm passes 2..%d, modelled kcycles per wave summed: " % PASSES +
          "; ".join(f"{k} {total[k] / 1e3:.1f} ({100.0 * (base - total[k]) / base:+.1f} % saved)" for k in names))
    err = np.linalg.norm((S0 @ R.T + t) - (S0 @ T_true[:3, :3].T + T_true[:3, 3]), axis=1).mean()
    print(f"   after {PASSES} passes the source lies {err:.4f} m (mean) from where its true pose puts it")


def main():
    w = synth.make_world(1001)
    A = synth.lidar_scan(w, None, seed=1001)[:, :3].astype(np.float64)
    for tag, T, seed in (("0.9 m apart", synth.se3(5.0, (0.8, -0.4, 0.1)), 1002), ("4 m apart", synth.se3(2.0, (4.0, 0.8, 0.0)), 1003)):
        B = synth.lidar_scan(w, T, seed=seed)[:, :3].astype(np.float64)
        model_pair(tag, A, B, T)


if __name__ == "__main__":
    main()
