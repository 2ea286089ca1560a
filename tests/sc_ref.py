"""The contract of gloc_sc_* restated in numpy: float64 for every decision and every distance, fp32 only where the
contract itself says fp32 (the height's one addition, the ring key's sum).  Nothing here looks at the library."""
import numpy as np

DEFAULTS = dict(n_rings=20, n_sectors=60, max_radius=80.0, sensor_height=2.0, min_common_columns=1)


def bin_coordinates(pts, n_rings=20, n_sectors=60, max_radius=80.0, **_):
    """(finite & in range [n] bool, fractional ring coordinate [n], fractional sector coordinate [n]) in float64; the
    ring of a point is the floor of the first, its sector the floor of the second (each clamped to the last bin)."""
    p = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(p).all(axis=1)
        r = np.hypot(p[:, 0], p[:, 1])
        keep = fin & (r < np.float64(np.float32(max_radius)))
        fr = r / np.float64(np.float32(max_radius)) * n_rings
        th = np.arctan2(p[:, 1], p[:, 0])
        th = np.where(th < 0, th + 2 * np.pi, th)
        fs = th / (2 * np.pi) * n_sectors
    return keep, fr, fs


def describe(pts, n_rings=20, n_sectors=60, max_radius=80.0, sensor_height=2.0, **_):
    """[n_rings, n_sectors] float32: the maximum of max(fp32(z) + fp32(sensor_height), 0) per polar bin, 0 when empty."""
    keep, fr, fs = bin_coordinates(pts, n_rings, n_sectors, max_radius)
    z = np.asarray(pts, np.float32)[keep, 2]
    ring = np.minimum(np.floor(fr[keep]).astype(np.int64), n_rings - 1)
    sec = np.minimum(np.floor(fs[keep]).astype(np.int64), n_sectors - 1)
    with np.errstate(over="ignore"):
        v = np.maximum(z + np.float32(sensor_height), np.float32(0))
    D = np.zeros((n_rings, n_sectors), np.float32)
    np.maximum.at(D, (ring, sec), v)
    return D


def ring_keys(desc):
    """The fp32 mean of every ring, summed in sector order: (((d[r][0] + d[r][1]) + ...) + d[r][S-1]) / fp32(S)."""
    d = np.asarray(desc, np.float32)
    s = np.zeros(d.shape[:-1], np.float32)
    for j in range(d.shape[-1]):
        s = s + d[..., j]
    return s / np.float32(d.shape[-1])


def by_shift(q, c, min_common_columns=1):
    """float64 [n_sectors]: at shift s, 1 - the mean cosine of np.roll(q, s, axis=1)'s and c's columns over the sectors
    where both are non-empty; 1.0 where fewer than max(min_common_columns, 1) sectors qualify."""
    q, c = np.asarray(q, np.float64), np.asarray(c, np.float64)
    S = q.shape[1]
    qn, cn = np.sqrt((q * q).sum(0)), np.sqrt((c * c).sum(0))
    qne, cne = (q > 0).any(0), (c > 0).any(0)
    out = np.ones(S)
    for s in range(S):
        both = np.roll(qne, s) & cne
        if both.sum() >= max(int(min_common_columns), 1):
            qs = np.roll(q, s, axis=1)[:, both]
            cos = (qs * c[:, both]).sum(0) / (np.roll(qn, s)[both] * cn[both])
            out[s] = 1.0 - cos.mean()
    return out


def by_shift_many(q, rows, min_common_columns=1):
    """by_shift of one query against many rows at once, float64 [n, n_sectors]: the same sums, read off the diagonals of
    the matrix of column cosines (tests/test_sc_ref_cpu.py holds the two together)."""
    q, C = np.asarray(q, np.float64), np.asarray(rows, np.float64)
    S = q.shape[1]
    qn, cn = np.sqrt((q * q).sum(0)), np.sqrt((C * C).sum(1))                    # [S], [n, S]
    qne, cne = (q > 0).any(0), (C > 0).any(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.tensordot(q.T, C, axes=([1], [1])).transpose(1, 0, 2) / (qn[None, :, None] * cn[:, None, :])
        # (cos[n, i, j]: column i of q against column j of row n)
    out = np.ones((C.shape[0], S))
    j = np.arange(S)
    for s in range(S):
        i = (j - s) % S
        both = qne[i][None, :] & cne
        cnt = both.sum(1)
        tot = np.where(both, cos[:, i, j], 0.0).sum(1)
        ok = cnt >= max(int(min_common_columns), 1)
        out[ok, s] = 1.0 - tot[ok] / cnt[ok]
    return out


def distance(q, c, min_common_columns=1):
    """(distance, shift): the minimum over the shifts, the lowest shift among equals."""
    d = by_shift(q, c, min_common_columns)
    s = int(np.argmin(d))
    return float(d[s]), s


def shift_to_yaw(shift, n_sectors=60):
    a = 2 * np.pi * shift / n_sectors
    return a - 2 * np.pi if a > np.pi else a
