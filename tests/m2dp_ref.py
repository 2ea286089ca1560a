"""The contract of gloc_m2dp_* (include/gloc3d.h) restated in numpy, float64 throughout: points -> frame -> counts ->
descriptor, and the seed of two frames.  fp32 only where the contract says fp32: the range test of M1 and the final cast.
Nothing here looks at the library."""
import numpy as np

DEFAULTS = dict(n_azimuth=4, n_elevation=16, n_rings=8, n_sectors=16, max_range=80.0, min_points=16)


def _prm(prm):
    out = dict(DEFAULTS)
    out.update({k: v for k, v in prm.items() if k in DEFAULTS})
    return out


def dim(**prm):
    p = _prm(prm)
    return p["n_azimuth"] * p["n_elevation"] + p["n_rings"] * p["n_sectors"]


def used_points(pts, **prm):
    """M1: [n] bool -- the three coordinates finite and (x x + y y) + z z < max_range^2 in un-fused fp32."""
    p = np.asarray(pts, np.float32)[:, :3]
    mr = np.float32(_prm(prm)["max_range"])
    with np.errstate(all="ignore"):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        d2 = (x * x + y * y) + z * z
        return np.isfinite(p).all(axis=1) & (d2 < mr * mr)


def jacobi_eig3(A):
    """The project's cyclic Jacobi (csrc/math3.hpp jacobi_eig3) on a symmetric 3 x 3: (diagonal left, V with the
    eigenvectors as columns)."""
    A = np.array(A, np.float64)
    V = np.eye(3)
    for _ in range(16):
        off = A[0, 1] * A[0, 1] + A[0, 2] * A[0, 2] + A[1, 2] * A[1, 2]
        diag = A[0, 0] * A[0, 0] + A[1, 1] * A[1, 1] + A[2, 2] * A[2, 2]
        if off <= 1e-32 * diag or off == 0.0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p, q]
            if apq == 0.0:
                continue
            theta = (A[q, q] - A[p, p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + np.sqrt(theta * theta + 1.0))
            if theta < 0:
                t = -t
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            for M in (A, None, V):
                if M is None:
                    rp, rq = A[p, :].copy(), A[q, :].copy()
                    A[p, :], A[q, :] = c * rp - s * rq, s * rp + c * rq
                else:
                    cp, cq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * cp - s * cq, s * cp + c * cq
    return np.diag(A).copy(), V


def frame(pts, **prm):
    """M2: dict(n, c [3], R [3, 3] with e1 e2 e3 as columns, lam [3] descending, m3 [2] the normalised third moments on e1
    and e2 before the sign rule, r = max |p - c|, frame [12] = R row-major then c).  n = 0: no descriptor."""
    P = _prm(prm)
    p = np.asarray(pts, np.float32)[:, :3]
    p = p[used_points(pts, **prm)].astype(np.float64)
    n = p.shape[0]
    if n < P["min_points"]:
        return dict(n=0, c=np.zeros(3), R=np.eye(3), lam=np.zeros(3), m3=np.zeros(2), r=0.0,
                    frame=np.concatenate([np.eye(3).ravel(), np.zeros(3)]), d=np.zeros((0, 3)))
    c = p.sum(axis=0) / n
    d = p - c
    C = d.T @ d / n
    lam, V = jacobi_eig3(C)
    order = np.argsort(-lam, kind="stable")                       # ties: the lower column first
    lam, V = lam[order], V[:, order]
    m3 = np.array([((d @ V[:, a]) ** 3).sum() for a in range(2)])
    e1 = -V[:, 0] if m3[0] < 0 else V[:, 0]
    e2 = -V[:, 1] if m3[1] < 0 else V[:, 1]
    R = np.stack([e1, e2, np.cross(e1, e2)], axis=1)
    with np.errstate(all="ignore"):
        m3n = m3 / (n * np.maximum(lam[:2], 0) ** 1.5)
    r = float(np.sqrt((d * d).sum(axis=1).max()))
    return dict(n=n, c=c, R=R, lam=lam, m3=m3n, r=r, frame=np.concatenate([R.ravel(), c]), d=d)


def plane_basis(**prm):
    """M3: (u [p q, 3], v [p q, 3]) -- the in-plane unit pair of plane a q + b."""
    P = _prm(prm)
    p_, q_ = P["n_azimuth"], P["n_elevation"]
    a, b = np.divmod(np.arange(p_ * q_), q_)
    th = -np.pi / 2 + a * np.pi / p_
    ph = b * (np.pi / 2) / q_
    u = np.stack([-np.sin(th), np.cos(th), np.zeros_like(th)], axis=1)
    v = np.stack([-np.sin(ph) * np.cos(th), -np.sin(ph) * np.sin(th), np.cos(ph)], axis=1)
    return u, v


def bin_coordinates(pts, **prm):
    """(fractional ring coordinate [n_used, p q], fractional sector coordinate [n_used, p q], the frame): the ring of a
    (point, plane) is the floor of the first, its sector the floor of the second, each clamped to the last bin."""
    f = frame(pts, **prm)
    fr, fs = coordinates_in_frame(f["d"], f, **prm)
    return fr, fs, f


def coordinates_in_frame(d, f, **prm):
    """The fractional (ring, sector) coordinates [m, p q] of the centred points d = p - c [m, 3] in a given frame."""
    P = _prm(prm)
    y = np.asarray(d, np.float64) @ f["R"]
    u, v = plane_basis(**prm)
    al, be = y @ u.T, y @ v.T
    rho = np.hypot(al, be)
    with np.errstate(all="ignore"):
        fr = np.where(rho > 0, np.sqrt(rho / f["r"]) * P["n_rings"], 0.0) if f["r"] > 0 else np.zeros_like(rho)
    ang = np.mod(np.arctan2(be, al), 2 * np.pi)
    fs = np.where(rho > 0, ang / (2 * np.pi) * P["n_sectors"], 0.0)
    return fr, fs


def counts(pts, **prm):
    """M3: (counts [p q, l t] uint32, the frame)."""
    P = _prm(prm)
    l, t = P["n_rings"], P["n_sectors"]
    fr, fs, f = bin_coordinates(pts, **prm)
    nP = P["n_azimuth"] * P["n_elevation"]
    out = np.zeros((nP, l * t), np.uint32)
    if f["n"]:
        ring = np.minimum(np.floor(fr).astype(np.int64), l - 1)
        sec = np.minimum(np.floor(fs).astype(np.int64), t - 1)
        np.add.at(out, (np.broadcast_to(np.arange(nP), ring.shape), ring * t + sec), 1)
    return out, f


def signature_svd(cnt, n_points):
    """M4 on given counts: (descriptor [p q + l t] float32, sigma1, sigma2) of A = counts / n_points; the zero matrix (or
    n_points = 0) gives the zero row."""
    cnt = np.asarray(cnt, np.float64)
    if n_points == 0 or not cnt.any():
        return np.zeros(cnt.shape[0] + cnt.shape[1], np.float32), 0.0, 0.0
    U, S, Vt = np.linalg.svd(cnt / n_points, full_matrices=False)
    u1, v1 = U[:, 0], Vt[0]
    if u1.sum() < 0:
        u1, v1 = -u1, -v1
    return np.concatenate([u1, v1]).astype(np.float32), float(S[0]), float(S[1]) if len(S) > 1 else 0.0


def describe(pts, **prm):
    """(descriptor float32 [dim], frame [12] float64, counts [p q, l t] uint32)."""
    cnt, f = counts(pts, **prm)
    return signature_svd(cnt, f["n"])[0], f["frame"], cnt


def frame_to_seed(frame_q, frame_db):
    """M5: the fp32 4 x 4 query -> place: R_db R_q^T and c_db - R_db R_q^T c_q."""
    fq, fd = np.asarray(frame_q, np.float64), np.asarray(frame_db, np.float64)
    R = fd[:9].reshape(3, 3) @ fq[:9].reshape(3, 3).T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, fd[9:] - R @ fq[9:]
    return T.astype(np.float32)
