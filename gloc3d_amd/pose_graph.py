"""A pose graph over the library's registration results: nodes with float64 poses (node -> map), edges (source, target, Z,
information) as gloc_reg_<m>_pairs and gloc_reg_evaluate_pairs produce them, optimised on the device by
capi.PoseGraphOptimizer (gloc_pgo_* of include/gloc3d.h)."""
import numpy as np

from . import capi


class PoseGraph:
    def __init__(self, device=0):
        self.poses, self.fixed = [], []
        self.src, self.tgt, self.Z, self.info, self.robust = [], [], [], [], []
        self._device, self._opt = device, None
        self.last_s2 = self.last_weight = self.last_consistency = None

    def __len__(self):
        return len(self.poses)

    @property
    def n_edges(self):
        return len(self.src)

    def add_node(self, pose, fixed=False):
        """pose [4, 4], node -> map.  Returns the node's index."""
        self.poses.append(np.array(pose, np.float64).reshape(4, 4))
        self.fixed.append(bool(fixed))
        return len(self.poses) - 1

    def add_edge(self, i, j, Z, info, robust=True):
        """Z [4, 4] maps node i (source) -> node j (target), Z ~ T_j^-1 T_i; info [6, 6] weights its left perturbation,
        rotation first.  robust: the robust kernel of optimize() applies to this edge (odometry usually says False)."""
        if i == j or not (0 <= i < len(self.poses) and 0 <= j < len(self.poses)):
            raise ValueError(f"edge ({i}, {j}) of {len(self.poses)} nodes")
        self.src.append(int(i)), self.tgt.append(int(j))
        self.Z.append(np.array(Z, np.float32).reshape(4, 4))
        self.info.append(np.array(info, np.float64).reshape(6, 6))
        self.robust.append(bool(robust))
        return len(self.src) - 1

    def add_registered(self, registrar, node_of_scan, src_ids, tgt_ids, T, eval_params=None, min_fitness=0.0, robust=True):
        """The rows of a pairs call as edges: evaluate_pairs gives each its information matrix, and a row becomes an edge
        iff its fitness is at least min_fitness and it counted a pair.  node_of_scan maps a scan id to its node.  Returns the
        indices of the rows that were added."""
        ev = registrar.evaluate_pairs(src_ids, tgt_ids, T, eval_params)
        T = np.asarray(T, np.float32).reshape(-1, 4, 4)
        kept = []
        for c, (s, t) in enumerate(zip(src_ids, tgt_ids)):
            if ev["count"][c] > 0 and ev["fitness"][c] >= min_fitness:
                self.add_edge(node_of_scan[int(s)], node_of_scan[int(t)], T[c], ev["info"][c], robust)
                kept.append(c)
        return kept

    def optimize(self, params=None, robust=None):
        """Levenberg-Marquardt on the device.  Returns (poses [n, 4, 4], (s2 [m], weight [m]), PgoResult) and keeps the poses;
        robust: a capi.RobustParams applied to the edges added with robust=True."""
        if self._opt is None:
            self._opt = capi.PoseGraphOptimizer(self._device)
        out, s2, w, res = self._opt.optimize(np.array(self.poses), np.array(self.fixed, np.uint8), self.src, self.tgt, np.array(self.Z),
                                             np.array(self.info), np.array(self.robust, np.uint8), params, robust)
        self.poses = [p for p in out]
        self.last_s2, self.last_weight = s2, w
        return out, (s2, w), res

    def prune(self, min_weight):
        """Drop the edges whose weight in the last optimize() was below min_weight: the ones the robust kernel switched off.
        Returns how many went."""
        if self.last_weight is None:
            raise RuntimeError("prune() follows optimize()")
        keep = [e for e in range(len(self.src)) if self.last_weight[e] >= min_weight]
        gone = len(self.src) - len(keep)
        for name in ("src", "tgt", "Z", "info", "robust"):
            setattr(self, name, [getattr(self, name)[e] for e in keep])
        self.last_s2, self.last_weight = self.last_s2[keep], self.last_weight[keep]
        return gone

    def select_consistent(self, params=None, path=None, apply=True):
        """The largest mutually consistent set of the closures -- the edges added with robust=True -- at the graph's current
        poses (gloc_pgo_consistency; params: a capi.PgoConsistencyParams).  path [n]: a coordinate along the trajectory,
        the node index by default.  Returns the indices of the kept closures in the graph as the call leaves it; with apply
        the others are dropped as prune() drops edges (none is when no set reaches min_clique: then the returned list is
        empty and the graph stays).
        Use: select_consistent(), optimize(), and select_consistent() again with a smaller drift on the corrected poses to
        re-admit closures the drifted start hid."""
        if self._opt is None:
            self._opt = capi.PoseGraphOptimizer(self._device)
        cand = [e for e in range(len(self.src)) if self.robust[e]]
        if not cand:
            return []
        pth = np.arange(len(self.poses), dtype=np.float64) if path is None else np.asarray(path, np.float64)
        out = self._opt.consistency(np.array(self.poses), [self.src[e] for e in cand], [self.tgt[e] for e in cand],
                                    np.array([self.Z[e] for e in cand]), np.array([self.info[e] for e in cand]), pth, params)
        self.last_consistency = out
        if not out["ok"]:
            return []
        kept = [e for e, m in zip(cand, out["mask"]) if m]
        if apply:
            gone = set(cand) - set(kept)
            keep = [e for e in range(len(self.src)) if e not in gone]
            new_index = {e: k for k, e in enumerate(keep)}
            for name in ("src", "tgt", "Z", "info", "robust"):
                setattr(self, name, [getattr(self, name)[e] for e in keep])
            if self.last_weight is not None:
                self.last_s2, self.last_weight = self.last_s2[keep], self.last_weight[keep]
            kept = [new_index[e] for e in kept]
        return kept

    def close(self):
        if self._opt is not None:
            self._opt.close()
            self._opt = None
