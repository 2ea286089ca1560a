"""Restatement of the ISS keypoints and the keypoint-restricted FPFH matching (include/gloc3d.h: gloc_iss_params, I1 - I4) --
the contract of gloc_scan_store_iss_saliency / _build_keypoints / _keypoints and of the _keypoints batch entries.  numpy only;
the lists are tests/fpfh_radius_ref.py's float32 brute force (R1), the eigenvalues the checker's cyclic Jacobi
(oracle.oracle_jacobi_eig3), and the matcher is tests/fpfh_ref.py's on tables whose non-keypoint rows are zeroed: no second
matcher is written here.

Parameters are a dict with the keys of DEFAULTS."""
import numpy as np

import fpfh_radius_ref as R
import fpfh_ref as F

NONE = F.NONE
DEFAULTS = dict(salient_radius=3.0, max_nn=128, min_nn=5, non_max_radius=2.0, gamma_21=0.975, gamma_32=0.975)


def params(**over):
    return dict(DEFAULTS, **over)


def saliency(xyz, prm, oracle):
    """I1: (saliency [n] float32, eig [n, 3] float64 sorted l1 >= l2 >= l3 -- zeros where the list is too short --, idx, count
    of the lists).  float64 from the float32 inputs, every sum taken in list order."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n, W = len(xyz), int(prm["max_nn"])
    sal, eig = np.zeros(n, np.float32), np.zeros((n, 3), np.float64)
    idx, _, count = R.radius_lists(xyz, prm["salient_radius"], W)
    if n == 0:
        return sal, eig, idx, count
    P = xyz.astype(np.float64)
    valid = idx != NONE
    q = P[np.where(valid, idx, 0)]                                    # [n, W, 3]
    cnt = valid.sum(1)
    mean = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for s in range(W):                                            # the sum in list order, slot by slot
            mean = mean + np.where(valid[:, s, None], q[:, s], 0.0)
        mean = mean / np.maximum(cnt, 1)[:, None].astype(np.float64)
        C = np.zeros((n, 6))                                          # xx xy xz yy yz zz
        for s in range(W):
            d = q[:, s] - mean
            t = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
            C = C + np.where(valid[:, s, None], t, 0.0)
    L = oracle.lib()
    g21, g32 = float(np.float32(prm["gamma_21"])), float(np.float32(prm["gamma_32"]))
    A, V = np.empty(9), np.empty(9)
    for i in np.flatnonzero(cnt >= int(prm["min_nn"])):
        c = C[i]
        A[:] = (c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5])
        L.oracle_jacobi_eig3(A, V)
        l1, l2, l3 = sorted((A[0], A[4], A[8]), reverse=True)
        eig[i] = (l1, l2, l3)
        if l3 > 0.0 and l2 < g21 * l1 and l3 < g32 * l2:
            sal[i] = np.float32(l3)
    return sal, eig, idx, count


def nms(xyz, sal, non_max_radius, chunk=512):
    """I2: bool [n].  i is a keypoint iff sal_i > 0 and no j != i with d2(i, j) <= r2 (float32, as R1 forms them) has
    sal_j > sal_i, or sal_j == sal_i and j < i."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    sal = np.asarray(sal, np.float32)
    n = len(xyz)
    r2 = np.float32(non_max_radius) * np.float32(non_max_radius)
    keep = np.zeros(n, bool)
    j = np.arange(n)
    for s in range(0, n, chunk):
        p, ps, pi = xyz[s:s + chunk], sal[s:s + chunk], j[s:s + chunk]
        with np.errstate(all="ignore"):
            dx, dy, dz = (p[:, None, a] - xyz[None, :, a] for a in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            inside = d <= r2
        beats = (sal[None, :] > ps[:, None]) | ((sal[None, :] == ps[:, None]) & (j[None, :] < pi[:, None]))
        beaten = (inside & beats & (j[None, :] != pi[:, None])).any(1)
        keep[s:s + chunk] = (ps > 0) & ~beaten
    return keep


def keypoints(xyz, prm, oracle):
    """I1 - I3: the keypoints' indices, ascending, uint32 [K]."""
    sal = saliency(xyz, prm, oracle)[0]
    return np.flatnonzero(nms(xyz, sal, prm["non_max_radius"])).astype(np.uint32)


def restrict(feat, kp):
    """I4's tables: the feature rows with every non-keypoint row "no feature"."""
    feat = np.asarray(feat, np.float32).reshape(-1, F.DIM)
    out = np.zeros_like(feat)
    kp = np.asarray(kp, np.int64)
    out[kp] = feat[kp]
    return out


def register(src, tgt, src_feat, tgt_feat, kp_src, kp_tgt, oracle, graph=False, stream_id=0, **params_):
    """F3 on the restricted tables, then F4 (fpfh_ref.register) or G1 - G4 (pairgraph_ref.register), both unchanged."""
    fs, ft = restrict(src_feat, kp_src), restrict(tgt_feat, kp_tgt)
    if graph:
        import pairgraph_ref as G
        return G.register(src, tgt, oracle, src_feat=fs, tgt_feat=ft, **params_)
    return F.register(src, tgt, oracle, stream_id=stream_id, src_feat=fs, tgt_feat=ft, **params_)
