"""Seeded pose graphs for the tests of gloc_pgo_*: chains and loops whose relative poses are cut from a ground-truth
trajectory, noise drawn through Omega^(-1/2), a share of gross-outlier closures."""
import numpy as np

import pgo_ref as R


def se3(w, t):
    T = np.eye(4)
    T[:3, :3] = R.exp_so3(np.asarray(w, np.float64))
    T[:3, 3] = t
    return T


def left(xi, T):
    """The library's retraction: (exp(w) R, exp(w) t + v)."""
    Q = T.copy()
    E = R.exp_so3(np.asarray(xi[:3], np.float64))
    Q[:3, :3] = E @ T[:3, :3]
    Q[:3, 3] = E @ T[:3, 3] + xi[3:]
    return Q


def trajectory(n, rng, radius=None, wobble=0.05):
    """n poses round a circle of about 2 m per node (one lap), with a little roll, pitch and height."""
    radius = radius or max(3.0, n * 2.0 / (2 * np.pi))
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        w = np.array([wobble * np.sin(3 * a), wobble * np.cos(2 * a), a + np.pi / 2])
        yaw = se3([0, 0, w[2]], [0, 0, 0])
        tilt = se3([w[0], w[1], 0], [0, 0, 0])
        T = yaw @ tilt
        T[:3, 3] = [radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(2 * a)]
        out.append(T)
    return np.array(out)


def random_info(rng, m, rot=4e4, trans=2e3):
    """SPD information matrices of the size evaluate_pairs gives for a few thousand pairs (rotation block larger)."""
    out = np.empty((m, 6, 6))
    for e in range(m):
        B = rng.normal(size=(6, 6)) * 0.15 + np.eye(6)
        D = np.diag(np.sqrt([rot, rot, rot, trans, trans, trans]))
        out[e] = D @ (B @ B.T) @ D
    return out


def measure(Ti, Tj, info=None, rng=None, sigma=1.0):
    """Z = T_j^-1 T_i, float32; with rng: perturbed on the left by xi ~ N(0, sigma^2 info^-1)."""
    Z = np.linalg.inv(Tj) @ Ti
    if rng is not None:
        Lc = np.linalg.cholesky(info)
        xi = sigma * np.linalg.solve(Lc.T, rng.normal(size=6))
        Z = left(xi, Z)
    return Z.astype(np.float32)


def graph(n, closures, seed, noise=0.0, outliers=0.0, drift=(0.002, 0.02), loop=True, radius=None):
    """A loop of n nodes: n - 1 odometry edges (k + 1 -> k), `closures` closure edges between random distant nodes (and,
    with loop, one from the last node to the first).  Returns dict(truth, init, fixed, src, tgt, Z, info, odo, outlier).
    init: the truth with a random-walk drift (rot, trans per step) applied on the left of every relative step."""
    rng = np.random.default_rng(seed)
    truth = trajectory(n, rng, radius)
    src, tgt = [k + 1 for k in range(n - 1)], [k for k in range(n - 1)]
    if loop and n > 2:
        src.append(n - 1), tgt.append(0)
    while len(src) < (n - 1) + closures + (1 if loop and n > 2 else 0):
        i, j = rng.integers(0, n, 2)
        if abs(int(i) - int(j)) >= 2:
            src.append(int(i)), tgt.append(int(j))
    src, tgt = np.array(src, np.uint32), np.array(tgt, np.uint32)
    m = len(src)
    info = random_info(rng, m)
    odo = np.arange(m) < n - 1
    outlier = (~odo) & (rng.random(m) < outliers)
    Z = np.empty((m, 4, 4), np.float32)
    for e in range(m):
        Z[e] = measure(truth[src[e]], truth[tgt[e]], info[e], rng if noise else None, noise)
        if outlier[e]:
            Z[e] = left(np.concatenate([rng.normal(size=3) * 0.3, rng.normal(size=3) * 4.0]), Z[e].astype(np.float64)).astype(np.float32)
    init = [truth[0].copy()]
    for k in range(1, n):
        step = np.linalg.inv(truth[k - 1]) @ truth[k]
        step = left(np.concatenate([rng.normal(size=3) * drift[0], rng.normal(size=3) * drift[1]]), step)
        init.append(init[-1] @ step)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return dict(truth=truth, init=np.array(init), fixed=fixed, src=src, tgt=tgt, Z=Z, info=info, odo=odo, outlier=outlier)


def hub(degree, seed):
    """Node 0 fixed, node 1 the hub with `degree` edges to leaves 2 .. degree + 1 (alternating directions), noisy."""
    rng = np.random.default_rng(seed)
    n = degree + 2
    truth = np.array([se3(rng.normal(size=3) * 0.5, rng.normal(size=3) * 10.0) for _ in range(n)])
    src, tgt = [0], [1]
    for k in range(degree - 1):
        a, b = (1, 2 + k) if k % 2 else (2 + k, 1)
        src.append(a), tgt.append(b)
    src, tgt = np.array(src, np.uint32), np.array(tgt, np.uint32)
    info = random_info(rng, len(src))
    Z = np.array([measure(truth[i], truth[j], info[e], rng, 1.0) for e, (i, j) in enumerate(zip(src, tgt))])
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    init = np.array([left(rng.normal(size=6) * 0.01, T) for T in truth])
    return dict(truth=truth, init=init, fixed=fixed, src=src, tgt=tgt, Z=Z, info=info)


def loop5():
    """A 5-node loop with edge 1 reversed and edge 2 given twice."""
    g = graph(5, 0, seed=2, noise=1.0)
    s, t = g["src"].copy(), g["tgt"].copy()
    s[1], t[1] = t[1], s[1]
    g["Z"][1] = np.linalg.inv(g["Z"][1].astype(np.float64)).astype(np.float32)
    for k in ("Z", "info"):
        g[k] = np.concatenate([g[k], g[k][2:3]])
    g["src"], g["tgt"] = np.append(s, s[2]).astype(np.uint32), np.append(t, t[2]).astype(np.uint32)
    return g


def n257():
    """257 nodes and 1025 edges (work-group boundaries): node 128 fixed as well as node 0, node 256 without an edge."""
    g = graph(256, 1025 - 256, seed=4, noise=1.0)                                  # 255 odometry + 1 + 769 closures
    g["init"] = np.concatenate([g["init"], [se3([0.3, 0.1, -0.2], [5.0, 6.0, 7.0])]])
    g["fixed"] = np.append(g["fixed"], 0).astype(np.uint8)
    g["fixed"][128] = 1
    assert len(g["init"]) == 257 and len(g["src"]) == 1025
    return g


def robust_case():
    g = graph(12, 8, seed=6, noise=1.0, outliers=0.4)
    return g, (~g["odo"]).astype(np.uint8)


def moved(T, G):
    """Every pose moved by one rigid motion G on the left."""
    return np.array([G @ P for P in T])


def rel_error(A, B):
    """max over nodes of |log(A_k^-1 B_k)| (rotation, translation) after aligning node 0."""
    Ga, Gb = np.linalg.inv(A[0]), np.linalg.inv(B[0])
    er = et = 0.0
    for a, b in zip(A, B):
        D = np.linalg.inv(Ga @ a) @ (Gb @ b)
        er = max(er, np.linalg.norm(R.log_so3(D[:3, :3])))
        et = max(et, np.linalg.norm(D[:3, 3]))
    return er, et
