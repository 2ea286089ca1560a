"""Scan-to-map tracking on a resident voxel map (include/gloc3d.h: M1 - M8): what follows the sensor once a global fix has
said where it is.  Orchestration only: every number comes from Registrar.vgicp_vmap, vmap_insert and vmap_prune, and a
hand-written sequence of those calls gives the same bits."""
import numpy as np

from . import capi


class ScanToMapTracker:
    """Holds a resident map of `registrar` and the sensor's pose in the map's frame (float32 [4, 4], scan -> map).

    track(scan_id, guess=None) registers the scan against the map from the guess -- or, without one, from the
    constant-velocity prediction of the last two poses (the last pose before there are two) --, inserts it under the refined
    pose when that has moved more than keyframe_dist metres or keyframe_angle radians since the last insert (or the map is
    empty: the first scan makes the map, at the guess or the identity), and then prunes the voxels beyond max_dist of the
    sensor (None: never).  Returns what vgicp_vmap returned for the scan, (T [1, 4, 4], rmse, iters, status[, weight]);
    None for the scan that made the map.  A refinement that ends degenerate (status 2) leaves pose and map as they were."""

    def __init__(self, registrar, map_params=None, vgicp_params=None, robust=None, keyframe_dist=1.0, keyframe_angle=0.2, max_dist=None,
                 pose=None):
        self.reg = registrar
        self.map_params = map_params or capi.default_vmap_params()
        self.params = vgicp_params or capi.default_vgicp_params(resolution=self.map_params.resolution)
        self.robust = robust
        self.keyframe_dist, self.keyframe_angle, self.max_dist = float(keyframe_dist), float(keyframe_angle), max_dist
        self.map_id = registrar.vmap_create(self.map_params)
        self.pose = np.eye(4, dtype=np.float32) if pose is None else np.array(pose, np.float32).reshape(4, 4)
        self.prev_pose = None           # the pose before this one: what the prediction extrapolates from
        self.key_pose = None            # the pose of the last insert
        self.inserted = []              # (scan id, pose) of every insert, in order

    @staticmethod
    def predict(prev_pose, pose):
        """Constant velocity: the last step applied once more, pose (prev^-1 pose), in float64, rounded to float32."""
        if prev_pose is None:
            return np.array(pose, np.float32)
        p, q = np.asarray(pose, np.float64), np.asarray(prev_pose, np.float64)
        return (p @ (np.linalg.inv(q) @ p)).astype(np.float32)

    @staticmethod
    def moved(a, b):
        """(metres, radians) between two poses."""
        d = np.linalg.inv(np.asarray(a, np.float64)) @ np.asarray(b, np.float64)
        return float(np.linalg.norm(d[:3, 3])), float(np.arccos(np.clip((np.trace(d[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))

    def _insert(self, scan_id):
        self.reg.vmap_insert(self.map_id, [scan_id], self.pose[None])
        self.key_pose = self.pose.copy()
        self.inserted.append((int(scan_id), self.pose.copy()))
        if self.max_dist is not None:
            self.reg.vmap_prune(self.map_id, center=self.pose[:3, 3], max_dist=self.max_dist)

    def track(self, scan_id, guess=None):
        start = self.predict(self.prev_pose, self.pose) if guess is None else np.array(guess, np.float32).reshape(4, 4)
        if self.key_pose is None:       # nothing to register against yet: the scan makes the map where the guess says it is
            self.pose = start
            self._insert(scan_id)
            return None
        out = self.reg.vgicp_vmap([scan_id], [self.map_id], init_T=start[None], params=self.params, robust=self.robust)
        if int(out[3][0]) == 2:
            return out
        self.prev_pose, self.pose = self.pose, out[0][0].copy()
        dist, angle = self.moved(self.key_pose, self.pose)
        if dist > self.keyframe_dist or angle > self.keyframe_angle:
            self._insert(scan_id)
        return out

    def info(self):
        return self.reg.vmap_info(self.map_id)

    def close(self):
        if self.map_id is not None:
            self.reg.vmap_destroy(self.map_id)
            self.map_id = None
