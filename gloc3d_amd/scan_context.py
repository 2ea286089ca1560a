"""Loop detection on Scan Context descriptors (gloc_sc_*): the surface of RpyPCLoopDetector (loop_detector.py) with a
descriptor that needs no trained weights -- add_keyframe(scan), detect(scan), detect_slam(), match(...) -- so that
scan -> descriptor -> retrieval -> registration runs on what the repository holds.  The retrieval also returns the column
shift of every candidate, i.e. the query's yaw in the candidate's frame, and match() starts the 3-D registration there:
a reverse-direction revisit begins 180 degrees turned instead of at the identity.
"""
import numpy as np

from . import capi
from .loop_detector import RpyPCLoopDetector


class ScanContextLoopDetector:
    def __init__(self, loop_dist_th, device=0, top_k=20, params=None, store=None):
        """loop_dist_th: detect_slam() accepts a loop iff the best Scan Context distance (in [0, 1]) is below it.  It has
        no default: a value has to come from the data the detector is used on.  store: a capi.ScanStore to keep the
        places' scans in (add_store_keyframes takes scans that are already resident there); its own otherwise."""
        self.top_k_ = top_k
        self.num_exclude_recent_ = 30   # the reference's window constants (loop_detector.h:99-100)
        self.tree_making_period_ = 30
        self.tree_making_period_counter_ = 0
        self.loop_dist_th_ = float(loop_dist_th)
        self._searchable_end = 0
        self._sc = capi.ScanContext(device, params)
        self._store = store
        self._reg = capi.Registrar(device, store)
        self._db_scan_ids = []
        self._last_descriptor = None
        self.reg_params = capi.default_reg_params()

    def close(self):
        self._sc.close()
        self._reg.close()

    def __len__(self):
        return len(self._db_scan_ids)

    def add_keyframe(self, scan):
        """Append one place: its descriptor (built on the device from the scan [n, 3|4]) and the scan as a registration
        target."""
        scan = np.ascontiguousarray(scan, np.float32)
        row = self._sc.add_scan(scan)
        self._db_scan_ids.append(self._reg.scan_build_target_index(self._reg.scan_upload(scan)))
        self._last_descriptor = self._sc.rows(row, 1)

    def add_store_keyframes(self, scan_ids):
        """Append scans resident in the detector's store as places, in order: descriptors in one launch sequence, the
        points never leave the device."""
        if self._store is None:
            raise ValueError("the detector was made without a store")
        ids = [int(i) for i in scan_ids]
        first = self._sc.add_store_scans(self._store, ids)
        self._store.build_target_index_batch(ids)
        self._db_scan_ids.extend(ids)
        self._last_descriptor = self._sc.rows(first + len(ids) - 1, 1)

    def detect(self, scan):
        """Global localization: (row indices, distances, shifts) of the top_k nearest places, or three empty arrays while
        the database is too small (the reference's guard, loop_detector.cpp:27-30)."""
        if len(self) <= self.num_exclude_recent_ + self.top_k_:
            print("Not enough keyframes in database.")
            return np.zeros(0, np.uint64), np.zeros(0, np.float32), np.zeros(0, np.uint32)
        idx, dist, shift = self._sc.search(self._sc.describe(scan), self.top_k_)
        return idx[0], dist[0], shift[0]

    def detect_slam(self):
        """SLAM mode (loop_detector.cpp:48-81): the newest keyframe is the query; every 30th call the searchable window is
        refreshed to db[0 : end - 30]; a loop iff the best distance is below loop_dist_th.
        Returns (found, q_idx, loop_idx, shift)."""
        n = len(self)
        if n <= self.num_exclude_recent_ + self.top_k_:
            return False, None, None, None
        if self.tree_making_period_counter_ % self.tree_making_period_ == 0:
            self._searchable_end = n - self.num_exclude_recent_
        self.tree_making_period_counter_ += 1
        idx, dist, shift = self._sc.search(self._last_descriptor, self.top_k_, 0, self._searchable_end)
        if dist[0, 0] < self.loop_dist_th_:
            return True, n - 1, int(idx[0, 0]), int(shift[0, 0])
        return False, None, None, None

    def yaw_from_shift(self, shift):
        return self._sc.shift_to_yaw(shift)

    def match(self, q_scan, db_indices, shifts=None, init_T=None):
        """Register the query scan against the retrieved places in one batch; returns (rank of the first successful
        candidate or -1, its 4x4 pose query -> db, full result).  Unless the caller gives initial poses, candidate c starts
        from the rotation about z by the yaw its shift stands for."""
        ids = [self._db_scan_ids[int(i)] for i in db_indices]
        q = np.ascontiguousarray(q_scan, np.float32)
        if init_T is None and shifts is not None and len(ids):
            init_T = np.stack([RpyPCLoopDetector.embed_3d((0.0, 0.0, self.yaw_from_shift(int(s)))) for s in shifts])
        qid = self._reg.scan_upload(q)
        try:
            res = self._reg.batch_ids(qid, ids, params=self.reg_params, init_T=init_T)
        finally:
            self._reg.scan_release(qid)
        r = capi.reg_select_first_ok(res["ok"].astype(np.int32))
        return r, (res["T"][r] if r >= 0 else np.eye(4, dtype=np.float32)), res
