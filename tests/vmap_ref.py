"""Float64 restatement of the resident voxel maps (gloc_reg_vmap_*, gloc_reg_vgicp_vmap*; include/gloc3d.h M1 - M8): the
executable contract of gloc3d_amd/csrc/vmap_kernels.hpp.  numpy only, built on tests/vgicp_ref.py: the voxel rule is its
cell_of, a map's voxels come out in the dict its voxels() makes, and the refinement against a map is its align(vox=...).

An insert of a cloud (with its normals, a zero normal meaning "no normal") under T, scan -> map:
  T None: point and normal as they are.  Else p = R s + t in fp32 with the pose rounded to fp32 (p2l_ref.move) and
  m = R n in float64 from the fp32 values, as ((R0 n0 + R1 n1) + R2 n2);
  per voxel (vgicp_ref.cell_of) n, s1 = sum (p - corner), s2 = sum m m^T, corner = k * resolution, in upload order;
  a new voxel takes them, an old one gets N += n, S1 += s1, S2 += s2; mean = corner + S1 / N, Nbar = S2 / N; the stamp of
  every voxel touched is the number of inserts so far, this one included.  An insert that would take the map above its
  capacity changes nothing and returns False.
Prune: a voxel goes if center is given and |mean - c|^2 > max_dist^2 (float64 of the fp32 values) or if max_age > 0 and
n_inserts - stamp > max_age.

`order`: "reversed" takes the sums of every contribution backwards -- the restatement's own noise floor, as in vgicp_ref.
"""
import numpy as np

import vgicp_ref as V
from p2l_ref import move

KEY_LIMIT = V.KEY_LIMIT


def contribution(cloud, nrm, resolution, T=None, order="forward"):
    """(packed int64 [m] ascending, n int64 [m], s1 [m, 3], s2 [m, 6]) of one insert."""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    n64 = np.zeros((len(cloud), 3)) if nrm is None else np.asarray(nrm, np.float32).reshape(-1, 3).astype(np.float64)
    if T is None:
        p, m = cloud, n64
    else:
        Tf = np.asarray(T, np.float64).astype(np.float32)
        p = move(Tf, cloud)
        R = Tf[:3, :3].astype(np.float64)
        m = np.stack([(R[r, 0] * n64[:, 0] + R[r, 1] * n64[:, 1]) + R[r, 2] * n64[:, 2] for r in range(3)], 1)
    k, ok = V.cell_of(p, resolution)
    idx = np.flatnonzero(ok)
    uniq, inverse, count = np.unique(V._pack(k[idx]), return_inverse=True, return_counts=True)
    corner = corners(uniq, resolution)
    if order == "reversed":
        idx, inverse = idx[::-1], inverse[::-1]
    rel = p[idx].astype(np.float64) - corner[inverse]
    u = m[idx]
    outer = np.stack([u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2], u[:, 2] * u[:, 2]], 1)
    s1, s2 = np.zeros((len(uniq), 3)), np.zeros((len(uniq), 6))
    np.add.at(s1, inverse, rel)                                      # one after the other, in index order
    np.add.at(s2, inverse, outer)
    return uniq.astype(np.int64), count.astype(np.int64), s1, s2


def key3_of(packed):
    packed = np.asarray(packed, np.int64)
    if not len(packed):
        return np.zeros((0, 3), np.int64)
    return np.stack([(packed >> 42) & 0x1FFFFF, (packed >> 21) & 0x1FFFFF, packed & 0x1FFFFF], 1).astype(np.int64) - KEY_LIMIT


def corners(packed, resolution):
    return key3_of(packed).astype(np.float64) * float(np.float32(resolution))


class Map:
    """A resident map: the voxels in the order they entered it (the device's array order), found by a dict."""

    def __init__(self, resolution=1.0, capacity=1 << 18, order="forward"):
        self.resolution, self.capacity, self.order = float(np.float32(resolution)), int(capacity), order
        self.packed = np.zeros(0, np.int64)
        self.N = np.zeros(0, np.int64)
        self.S1, self.S2 = np.zeros((0, 3)), np.zeros((0, 6))
        self.stamp = np.zeros(0, np.int64)
        self.at = {}
        self.n_inserts = 0

    def __len__(self):
        return len(self.packed)

    @property
    def n_points(self):
        return int(self.N.sum())

    def insert(self, cloud, nrm, T=None):
        """False, and nothing changed, if the voxels new to the map do not fit."""
        packed, n, s1, s2 = contribution(cloud, nrm, self.resolution, T, self.order)
        where = np.array([self.at.get(int(k), -1) for k in packed], np.int64)
        old, new = where >= 0, where < 0
        if len(self) + int(new.sum()) > self.capacity:
            return False
        self.n_inserts += 1
        self.N[where[old]] += n[old]                                 # (a contribution's keys are distinct: no index twice)
        self.S1[where[old]] += s1[old]
        self.S2[where[old]] += s2[old]
        self.stamp[where[old]] = self.n_inserts
        for i, k in enumerate(packed[new]):
            self.at[int(k)] = len(self.packed) + i
        self.packed = np.concatenate([self.packed, packed[new]])
        self.N = np.concatenate([self.N, n[new]])
        self.S1, self.S2 = np.concatenate([self.S1, s1[new]]), np.concatenate([self.S2, s2[new]])
        self.stamp = np.concatenate([self.stamp, np.full(int(new.sum()), self.n_inserts, np.int64)])
        return True

    def mean(self):
        return corners(self.packed, self.resolution) + self.S1 / self.N[:, None].astype(np.float64)

    def prune(self, center=None, max_dist=0.0, max_age=0):
        """How many voxels went."""
        gone = np.zeros(len(self), bool)
        if center is not None:
            d = self.mean() - np.asarray(center, np.float32).astype(np.float64)
            gone |= (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] > float(np.float32(max_dist)) ** 2
        if max_age > 0:
            gone |= self.n_inserts - self.stamp > int(max_age)
        keep = ~gone
        self.packed, self.N, self.S1, self.S2, self.stamp = self.packed[keep], self.N[keep], self.S1[keep], self.S2[keep], self.stamp[keep]
        self.at = {int(k): i for i, k in enumerate(self.packed)}
        return int(gone.sum())

    def voxels(self):
        """vgicp_ref.voxels' dict, sorted by key, and stamp int64 [m]."""
        o = np.argsort(self.packed, kind="stable")
        cnt = self.N[o].astype(np.float64)[:, None]
        return dict(key3=key3_of(self.packed[o]), count=self.N[o].copy(), mean=self.mean()[o], nn6=self.S2[o] / cnt, packed=self.packed[o].copy(),
                    stamp=self.stamp[o].copy())


def align(src, src_nrm, vmap, init_T=None, how="inv", order="forward", **params):
    """vgicp_ref.align against a map's voxels (resolution: the map's; min_points does not apply)."""
    params = {k: v for k, v in params.items() if k not in ("resolution", "min_points")}
    return V.align(src, src_nrm, None, None, init_T=init_T, resolution=vmap.resolution, how=how, order=order, vox=vmap.voxels(), **params)
