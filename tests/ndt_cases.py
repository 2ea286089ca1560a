"""Inputs shared by tests/test_ndt_sweep_cpu.py and tests/test_ndt_sweep_gpu.py: a few synthetic worlds, the scans taken
in them (CPU synth.lidar_scan, whose device twin tests/test_raycast_gpu.py pins), and the list of whole-alignment cases
with the float64 restatement's verdict on each (tests/ndt_ref.py::align, run twice in two summation orders).

Nothing here looks at a device: whether a case is "stable" is decided by the restatement alone."""
import functools

import numpy as np

import ndt_ref as R

N_AZ = 200          # azimuth steps of a scan: ~12 k points, so one ndt_ref.align takes a second or two on a CPU
STABLE_TOL = 1e-6   # m and rad: two summation orders of the restatement agree this well on a stable case

# name -> (seed, n_boxes, extent) of synth.make_world
WORLDS = {"a": (1001, 400, 50.0), "b": (2002, 300, 40.0), "c": (3003, 500, 60.0)}


def _se3(*a, **k):
    from gloc3d_amd import synth
    return synth.se3(*a, **k)


def scan_poses():
    """world <- sensor poses of the scans taken in every world: 0 and 1 serve as targets, 2 and 3 as sources."""
    return [np.eye(4), _se3(-3.0, (0.4, -0.3, 0.0)), _se3(2.0, (0.2, 0.0, 0.0)),
            _se3(-1.5, (0.1, 0.15, 0.02), roll_deg=-0.5)]


def tiny_scene(seed):
    """A hand-built scene of a few dozen cells: clusters of 14 points with random anisotropic spread as the target, and
    as the source every second target point with 1 cm of noise (source frame = target frame).  Small enough that a
    search over many of them for the line search's rare branches takes seconds."""
    rng = np.random.default_rng(seed)
    n_cl = 24
    centre = rng.uniform(-2.5, 2.5, (n_cl, 3)) * np.array([1.0, 1.0, 0.4])
    sigma = rng.uniform(0.02, 0.15, (n_cl, 1, 3))
    tgt = (centre[:, None, :] + rng.normal(size=(n_cl, 14, 3)) * sigma).reshape(-1, 3)
    src = tgt[::2] + rng.normal(size=tgt[::2].shape) * 0.01
    return np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32)


@functools.lru_cache(maxsize=None)
def scan(world, k):
    """Scan k of a world, float32 [n, 3], in its sensor's frame.  World "t<seed>": tiny_scene(seed), 0 its target and
    2 its source."""
    if world[0] == "t":
        return tiny_scene(int(world[1:]))[0 if k == 0 else 1]
    from gloc3d_amd import synth
    seed, n_boxes, extent = WORLDS[world]
    w = synth.make_world(seed, n_boxes=n_boxes, extent=extent)
    return np.ascontiguousarray(synth.lidar_scan(w, scan_poses()[k], seed=seed + 10 + k, n_az=N_AZ)[:, :3])


def truth(world, src, tgt):
    """source frame -> target frame of two scans of one world."""
    if world[0] == "t":
        return np.eye(4)
    P = scan_poses()
    return np.linalg.inv(P[tgt]) @ P[src]


def ref_params(over=None):
    """The parameter dict the restatement runs with: ndt_ref.DEFAULTS, then `over`, every float rounded to the float32
    a gloc_ndt_params holds (so 0.1 is the device's 0.1f)."""
    p = dict(R.DEFAULTS, **(over or {}))
    return {k: (int(v) if k in ("max_iters", "min_points_per_cell") else float(np.float32(v))) for k, v in p.items()}


def _case(name, world, src, tgt, yaw=0.0, t=(0.0, 0.0, 0.0), pitch=0.0, roll=0.0, **params):
    return dict(name=name, world=world, src=src, tgt=tgt, off=(yaw, t, pitch, roll), params=params)


# Guess = truth x offset.  Offsets run from 0.05 m / 0.5 deg to 1.5 m / 12 deg, some with roll / pitch, some with the
# yaw wrong by 180 deg (an indefinite Hessian); the parameter variants are the issue's.  "reach_*": no cell in reach.
CASES = [
    _case("b_00", "b", 3, 0, yaw=1.6, t=(-0.197, 0.018, -0.027), step_size=0.1, trans_eps=0.01, max_iters=35, resolution=0.5),
    _case("a_01", "a", 3, 1, yaw=4.0, t=(-0.442, -0.233, -0.005), step_size=1.0, trans_eps=0.001, resolution=2.0, outlier_ratio=0.2),
    _case("a_02", "a", 2, 1, yaw=172.0, t=(0.822, 0.243, 0.516), trans_eps=0.01, outlier_ratio=0.2),
    _case("c_03", "c", 2, 1, yaw=-1.6, t=(0.138, -0.145, 0.005), pitch=-0.42, roll=1.42, step_size=1.0, trans_eps=0.001, resolution=1.0),
    _case("b_04", "b", 2, 0, yaw=-1.6, t=(-0.043, -0.195, -0.007), pitch=-1.73, roll=1.56, step_size=1.0, trans_eps=0.01, outlier_ratio=0.2),
    _case("b_05", "b", 2, 1, yaw=179.6, t=(0.033, -0.033, -0.017), pitch=-0.84, roll=-2.44, step_size=1.0, trans_eps=0.01, max_iters=1, resolution=2.0),
    _case("c_06", "c", 3, 1, yaw=0.4, t=(0.044, 0.022, 0.005), step_size=0.1, trans_eps=0.001, max_iters=3, resolution=2.0, outlier_ratio=0.55),
    _case("a_07", "a", 3, 0, yaw=-8.0, t=(-0.39, 0.92, -0.026), pitch=2.88, roll=-1.19, step_size=0.02, trans_eps=0.01, max_iters=3, resolution=0.5),
    _case("a_08", "a", 3, 0, yaw=178.4, t=(-0.051, -0.193, -0.009), pitch=2.7, roll=0.41, step_size=0.1, trans_eps=0.001, max_iters=1),
    _case("c_09", "c", 2, 0, yaw=0.4, t=(-0.016, -0.047, 0.001), step_size=0.1, max_iters=35, resolution=1.0),
    _case("c_10", "c", 3, 1, yaw=-12.0, t=(0.563, 1.389, 0.047), step_size=0.02, trans_eps=0.2, max_iters=3, resolution=1.0, outlier_ratio=0.2),
    _case("a_11", "a", 2, 0, yaw=184.0, t=(-0.499, 0.021, -0.014), pitch=-0.73, roll=-2.62, step_size=1.0, max_iters=3, outlier_ratio=0.2),
    _case("b_12", "b", 2, 0, yaw=-12.0, t=(0.461, -1.427, -0.007), step_size=0.02, trans_eps=0.01, max_iters=1, resolution=1.0, outlier_ratio=0.55),
    _case("c_13", "c", 2, 0, yaw=-12.0, t=(-0.083, 1.45, 0.376), pitch=-2.98, roll=-1.91, step_size=0.1, trans_eps=0.2, resolution=0.5, outlier_ratio=0.55),
    _case("b_14", "b", 2, 1, yaw=-8.0, t=(-0.276, -0.954, -0.115), trans_eps=0.2, max_iters=3, resolution=1.0),
    _case("a_15", "a", 3, 0, yaw=168.0, t=(1.307, -0.696, -0.238), trans_eps=0.2, resolution=2.0, outlier_ratio=0.55),
    _case("c_16", "c", 2, 0, yaw=-1.6, t=(0.134, -0.148, -0.01), pitch=2.69, roll=-2.89, step_size=0.02, trans_eps=0.2, max_iters=35, outlier_ratio=0.2),
    _case("c_17", "c", 2, 0, yaw=8.0, t=(0.994, -0.079, -0.075), max_iters=1, resolution=2.0, outlier_ratio=0.55),
    _case("b_18", "b", 3, 0, yaw=-0.4, t=(-0.042, -0.026, 0.007), step_size=0.02, max_iters=35),
    _case("b_19", "b", 3, 0, yaw=4.0, t=(-0.062, 0.495, -0.033), max_iters=35, resolution=0.5),
    _case("c_20", "c", 2, 1, yaw=-0.4, t=(0.001, -0.047, -0.017), pitch=-0.48, roll=2.58, trans_eps=0.2, max_iters=1, resolution=0.5),
    _case("c_21", "c", 2, 0, yaw=-4.0, t=(0.307, -0.394, -0.012), trans_eps=0.001),
    _case("b_22", "b", 3, 1, yaw=-12.0, t=(0.256, 1.457, -0.25), step_size=1.0, trans_eps=0.2, outlier_ratio=0.55),
    _case("c_23", "c", 3, 0, yaw=-4.0, t=(-0.112, -0.487, 0.018), pitch=-1.57, roll=-1.82, step_size=0.1, trans_eps=0.2, resolution=0.5),
    _case("c_24", "c", 2, 1, yaw=-8.0, t=(-0.358, 0.928, -0.1), pitch=-0.75, roll=-1.33, step_size=0.1, trans_eps=0.2),
    _case("c_25", "c", 3, 1, yaw=1.6, t=(-0.193, -0.052, -0.009), step_size=0.02, trans_eps=0.2, outlier_ratio=0.2),
    _case("b_26", "b", 3, 1, yaw=188.0, t=(-0.965, 0.241, 0.1), pitch=-1.3, roll=-1.12, step_size=1.0),
    _case("a_27", "a", 3, 1, yaw=8.0, t=(0.303, 0.949, -0.081), step_size=1.0),
    _case("a_28", "a", 3, 0, yaw=-1.6, t=(-0.062, 0.19, 0.006), trans_eps=0.2, max_iters=35),
    _case("c_29", "c", 2, 0, yaw=178.4, t=(-0.197, 0.034, 0.008), pitch=1.68, roll=-2.88, step_size=0.02, trans_eps=0.2, outlier_ratio=0.55),
    _case("b_30", "b", 3, 0, yaw=168.0, t=(0.03, -1.481, 0.235), step_size=0.02, trans_eps=0.2),
    _case("a_31", "a", 2, 1, yaw=4.0, t=(0.474, -0.159, 0.001), trans_eps=0.001),
    _case("a_32", "a", 2, 1, yaw=-0.4, t=(0.041, -0.029, 0.0), step_size=0.1, trans_eps=0.2, max_iters=3),
    _case("b_33", "b", 2, 1, yaw=-0.4, t=(0.049, 0.011, 0.001), trans_eps=0.001, max_iters=35),
    _case("b_34", "b", 2, 0, yaw=0.4, t=(-0.023, 0.044, 0.002), step_size=1.0),
    _case("t114_35", "t114", 2, 0, yaw=6.03, t=(0.029, 0.017, 0.037), pitch=-0.59, roll=-0.3, source_leaf=0.0, step_size=0.02, trans_eps=0.2, resolution=1.0),
    _case("t118_36", "t118", 2, 0, yaw=5.41, t=(-0.082, -0.49, -0.059), pitch=-2.35, roll=2.68, source_leaf=0.0, step_size=1.0, trans_eps=0.01, resolution=2.0),
    _case("t109_37", "t109", 2, 0, yaw=2.4, t=(-0.018, -0.025, -0.04), pitch=-1.22, roll=2.07, source_leaf=0.0, step_size=1.0, trans_eps=0.2, resolution=2.0),
    _case("a_out_of_reach", "a", 2, 0, yaw=1.0, t=(1000.0, 0.0, 0.0)),
]


def guess(case):
    yaw, t, pitch, roll = case["off"]
    return (truth(case["world"], case["src"], case["tgt"]) @ _se3(yaw, t, pitch_deg=pitch, roll_deg=roll)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def filtered(world, src, leaf):
    return R.approx_voxel(scan(world, src), leaf)


@functools.lru_cache(maxsize=None)
def cells(world, tgt, resolution, min_points, eig_mult):
    return R.build_cells(scan(world, tgt), resolution, min_points, eig_mult)


def pose_gap(A, B):
    """Translation [m] and rotation angle [rad] between two 4x4 poses."""
    E = np.linalg.inv(np.asarray(A, np.float64)) @ np.asarray(B, np.float64)
    return float(np.linalg.norm(E[:3, 3])), float(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))


def reference(case):
    """The restatement's run of a case, and the same with the filtered source's rows reversed (another summation
    order, the same mathematics).  Returns dict(ref, events, stable): stable when both runs record the same events,
    iters and converged and end within STABLE_TOL of each other."""
    prm = ref_params(case["params"])
    x = filtered(case["world"], case["src"], prm["source_leaf"])
    c = cells(case["world"], case["tgt"], prm["resolution"], prm["min_points_per_cell"], prm["min_covar_eigvalue_mult"])
    g = guess(case)
    ev, ev2 = [], []
    r = R.align(x, c, init_T=g, params=prm, events=ev)
    r2 = R.align(x[::-1], c, init_T=g, params=prm, events=ev2)
    dt, da = pose_gap(r["T"], r2["T"])
    stable = bool(ev == ev2 and r["iters"] == r2["iters"] and r["converged"] == r2["converged"]
                  and np.isfinite(r["T"]).all() and dt <= STABLE_TOL and da <= STABLE_TOL)
    return dict(ref=r, events=ev, stable=stable)


@functools.lru_cache(maxsize=None)
def references():
    """name -> reference(case) for every case (computed once per process)."""
    return {c["name"]: reference(c) for c in CASES}
