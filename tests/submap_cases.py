"""The small trajectory the submap tests share: five places 0.8 m apart, four queries around the middle one.

32 beams x 600 azimuths (about 18 400 points a cast) of synth.make_world(7); the anchor is place 2.  Everything is made
once per process and must not be modified by a test.
"""
import functools

import numpy as np

from gloc3d_amd import synth

ANCHOR = 2
QUERY_POSES = [(3.0, (1.9, 0.4, 0.0)), (-4.0, (1.3, -0.5, 0.0)), (8.0, (2.6, 0.3, 0.0)), (1.0, (0.4, 1.5, 0.0))]


@functools.lru_cache(maxsize=None)
def trajectory():
    """(place scans [5] of [n, 3] float32, place poses [5, 4, 4] float64 world <- place, query scans [4], query poses [4, 4, 4])."""
    world = synth.make_world(7)
    P = np.stack([synth.se3(yaw_deg=2.0 * i, t=(0.8 * i, 0.05 * i, 0.0)) for i in range(5)])
    places = [np.ascontiguousarray(synth.lidar_scan(world, P[i], seed=10 + i, n_beams=32, n_az=600)[:, :3]) for i in range(5)]
    Q = np.stack([synth.se3(yaw_deg=y, t=t) for y, t in QUERY_POSES])
    queries = [np.ascontiguousarray(synth.lidar_scan(world, Q[i], seed=90 + i, n_beams=32, n_az=600)[:, :3]) for i in range(4)]
    return places, P, queries, Q


def member_poses(P, i, js):
    """T [len(js), 4, 4] float32, place j -> place i: inv(P_i) P_j in float64, then rounded."""
    inv_i = np.linalg.inv(np.asarray(P[i], np.float64))
    return np.stack([inv_i @ np.asarray(P[j], np.float64) for j in js]).astype(np.float32)


def truth(P, Q, qi, place=ANCHOR):
    """The pose query qi -> place frame."""
    return np.linalg.inv(P[place]) @ Q[qi]


def position_error(T_est, T_true):
    return float(np.linalg.norm(np.asarray(T_est, np.float64)[:3, 3] - np.asarray(T_true, np.float64)[:3, 3]))


def rotation_error_rad(T_est, T_true):
    """Angle of R_true^T R_est, well conditioned near zero (atan2 of the skew part, not acos of the trace)."""
    E = np.asarray(T_true, np.float64)[:3, :3].T @ np.asarray(T_est, np.float64)[:3, :3]
    v = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), (np.trace(E) - 1.0) / 2.0))


def rotation_error_deg(T_est, T_true):
    return float(np.degrees(rotation_error_rad(T_est, T_true)))
