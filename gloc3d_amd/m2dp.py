"""Loop detection on M2DP descriptors (gloc_m2dp_*): the surface of ScanContextLoopDetector (scan_context.py) with a
descriptor that is a plain L2 vector -- add_keyframe(scan), detect(scan), detect_slam(), match(...) -- so that the places
go into the exact top-k search of gloc_knn_* like any trained descriptor, at any database size it handles.  Every row
keeps the PCA frame its descriptor was built in; the frames of a query and of a retrieved place give the rotation
between the two scans at any yaw (gloc_m2dp_frame_to_seed), and match() starts the 3-D registration there.
"""
import numpy as np

from . import capi


class M2DPLoopDetector:
    def __init__(self, loop_dist_th, device=0, top_k=20, params=None, store=None):
        """loop_dist_th: detect_slam() accepts a loop iff the best squared descriptor distance is below it.  It has no
        default: a value has to come from the data the detector is used on.  store: a capi.ScanStore to keep the places'
        scans in (add_store_keyframes takes scans that are already resident there); its own otherwise."""
        self.top_k_ = top_k
        self.num_exclude_recent_ = 30   # the reference's window constants (loop_detector.h:99-100)
        self.tree_making_period_ = 30
        self.tree_making_period_counter_ = 0
        self.loop_dist_th_ = float(loop_dist_th)
        self._searchable_end = 0
        self._m2dp = capi.M2dp(device, params)
        self._index = capi.KnnIndex(self._m2dp.dim, device)
        self._store = store
        self._reg = capi.Registrar(device, store)
        self._db_scan_ids = []
        self._db_frames = []
        self._last_descriptor = None
        self._last_frame = None
        self.reg_params = capi.default_reg_params()

    def close(self):
        self._index.close()
        self._m2dp.close()
        self._reg.close()

    def __len__(self):
        return len(self._db_scan_ids)

    def describe(self, scan):
        """(descriptor [dim], frame [12]) of a host scan [n, 3|4]."""
        return self._m2dp.describe(np.ascontiguousarray(scan, np.float32))

    def _append(self, desc, frames, scan_ids):
        self._index.add(desc)
        self._db_frames.extend(np.asarray(frames, np.float64).reshape(-1, 12))
        self._db_scan_ids.extend(scan_ids)
        self._last_descriptor, self._last_frame = desc[-1:].copy(), self._db_frames[-1]

    def add_keyframe(self, scan):
        """Append one place: its descriptor and frame (built on the device from the scan [n, 3|4]) and the scan as a
        registration target."""
        scan = np.ascontiguousarray(scan, np.float32)
        d, f = self._m2dp.describe(scan)
        self._append(d[None], f[None], [self._reg.scan_build_target_index(self._reg.scan_upload(scan))])

    def add_store_keyframes(self, scan_ids):
        """Append scans resident in the detector's store as places, in order: descriptors in one launch sequence, the
        points never leave the device."""
        if self._store is None:
            raise ValueError("the detector was made without a store")
        ids = [int(i) for i in scan_ids]
        d, f = self._m2dp.describe_store_scans(self._store, ids)
        self._store.build_target_index_batch(ids)
        self._append(d, f, ids)

    def frame(self, row):
        return self._db_frames[int(row)]

    def seeds(self, q_frame, db_indices):
        """[n, 4, 4] float32: the rotation query -> place of every candidate from the two frames, translation zero (the
        centroid of a ring scan sits at the sensor: the frames' translation carries little)."""
        T = np.stack([capi.m2dp_frame_to_seed(q_frame, self._db_frames[int(i)]) for i in db_indices]) if len(db_indices) else np.zeros((0, 4, 4), np.float32)
        T[:, :3, 3] = 0
        return T

    def detect(self, scan):
        """Global localization: (row indices, squared distances, the query's frame) of the top_k nearest places, or
        empty arrays while the database is too small (the reference's guard, loop_detector.cpp:27-30)."""
        if len(self) <= self.num_exclude_recent_ + self.top_k_:
            print("Not enough keyframes in database.")
            return np.zeros(0, np.uint64), np.zeros(0, np.float32), None
        d, f = self.describe(scan)
        idx, d2 = self._index.search(d[None], self.top_k_)
        return idx[0], d2[0], f

    def detect_slam(self):
        """SLAM mode (loop_detector.cpp:48-81): the newest keyframe is the query; every 30th call the searchable window is
        refreshed to db[0 : end - 30]; a loop iff the best squared distance is below loop_dist_th.
        Returns (found, q_idx, loop_idx, seed 4x4 newest -> loop place)."""
        n = len(self)
        if n <= self.num_exclude_recent_ + self.top_k_:
            return False, None, None, None
        if self.tree_making_period_counter_ % self.tree_making_period_ == 0:
            self._searchable_end = n - self.num_exclude_recent_
        self.tree_making_period_counter_ += 1
        idx, d2 = self._index.search(self._last_descriptor, self.top_k_, 0, self._searchable_end)
        if d2[0, 0] < self.loop_dist_th_:
            return True, n - 1, int(idx[0, 0]), self.seeds(self._last_frame, idx[0, :1])[0]
        return False, None, None, None

    def match(self, q_scan, db_indices, q_frame=None, init_T=None):
        """Register the query scan against the retrieved places in one batch; returns (rank of the first successful
        candidate or -1, its 4x4 pose query -> db, full result).  Unless the caller gives initial poses, candidate c starts
        from the rotation between the query's frame and the place's, with the translation set to zero."""
        ids = [self._db_scan_ids[int(i)] for i in db_indices]
        q = np.ascontiguousarray(q_scan, np.float32)
        if init_T is None and q_frame is not None and len(ids):
            init_T = self.seeds(q_frame, db_indices)
        qid = self._reg.scan_upload(q)
        try:
            res = self._reg.batch_ids(qid, ids, params=self.reg_params, init_T=init_T)
        finally:
            self._reg.scan_release(qid)
        r = capi.reg_select_first_ok(res["ok"].astype(np.int32))
        return r, (res["T"][r] if r >= 0 else np.eye(4, dtype=np.float32)), res
