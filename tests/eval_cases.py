"""Inputs shared by tests/test_eval_cases_cpu.py, tests/test_eval_gpu.py and tests/test_pairs_system_gpu.py: the clouds
and the table of rows the point-to-point evaluation (gloc_reg_evaluate_pairs) is run on, with the float64 restatement's
answer to every row (tests/eval_ref.py through the CPU oracle's 1-NN search, computed once per process).

  (a) a shuffled 9^3 integer lattice as the target, its first 1 .. 513 points as sources, at the identity: every term and
      every partial sum is an integer far below 2^53, so no summation order can change a bit;
  (b) the lattice's points with x < 8 moved by (0.5, 0, 0): every moved point lies midway between two target points, the
      tie rule (smallest original index) decides e and g but not info; d2 = 0.25 exactly, so the gate 0.5 takes every
      pair and nextafter(0.5, 0) none; every term is a multiple of 1/4;
  (c) a ray-cast target of about 6 400 points (synth.lidar_scan, the CPU twin of ScanStore.add_raycast that
      tests/test_raycast_gpu.py pins, 100 azimuth steps) and three sources at truth x a small offset, under the gates 0.3,
      0.6 and 2.0;
  (d) a source with 1 % NaN / +-inf rows, the first and the last row among them;
  (e) a scan cast in another world;
  (f) a mixed list: sources of 1, 257 and about 6 400 points, a row without a target, an empty target, a scan against
      itself and one row twice.

Nothing here looks at a device."""
import functools

import numpy as np

import eval_ref as E
import gn_cases as GC

N_AZ = 100                                         # 64 beams x 100 azimuth steps: about 6 400 returns
WORLD, OTHER = (1001, 400, 50.0), (2002, 300, 40.0)
SIZES = (1, 5, 63, 64, 65, 255, 256, 257, 513)      # around a wave (64) and a work-group (256), and three work-groups
HALF_SIZES = (1, 64, 257, 648)
TIE_GATE = 0.5
BELOW_TIE_GATE = float(np.nextafter(np.float32(0.5), np.float32(0)))
GATES = (0.3, 0.6, 2.0)


def _se3(*a, **k):
    from gloc3d_amd import synth
    return synth.se3(*a, **k)


def scan_poses():
    """world <- sensor: 0 is the target's, 1 - 3 the sources'."""
    return [np.eye(4), _se3(2.0, (0.2, 0.0, 0.0)), _se3(-1.5, (0.1, 0.15, 0.02), roll_deg=-0.5), _se3(1.0, (-0.15, 0.1, 0.0), pitch_deg=0.3)]


OFFSETS = [(1.0, (0.10, -0.05, 0.02), 0.0), (-2.0, (-0.15, 0.10, -0.03), 0.4), (0.5, (0.25, 0.20, 0.05), 0.0)]


def _odd(xyz):
    """1 % of the rows NaN or +-inf in one coordinate or all, the first and the last row among them."""
    odd = xyz.copy()
    rows = np.unique(np.concatenate([[0, len(odd) - 1], np.arange(37, len(odd), 100)]))
    for k, r in enumerate(rows):
        if k % 4 == 0:
            odd[r] = np.nan
        elif k % 4 == 1:
            odd[r, 0] = np.inf
        elif k % 4 == 2:
            odd[r, 2] = -np.inf
        else:
            odd[r, 1] = np.nan
    return odd


@functools.lru_cache(maxsize=None)
def cloud(name):
    """float32 [n, 3].
      "lat"            the 9^3 integer lattice, shuffled
      "lat_n<k>"       its first k points
      "lat_h<k>"       k of its points with x < 8, shuffled again
      "t", "s1" - "s3" the target scan and the three source scans of the world
      "s1_odd"         s1 with non-finite rows
      "s1_n<k>"        k points of s1, evenly spread
      "far"            a scan cast in another world
      "empty"          no points"""
    from gloc3d_amd import synth
    if name == "empty":
        return np.zeros((0, 3), np.float32)
    if name == "lat":
        g = np.arange(9, dtype=np.float32)
        pts = np.stack([m.ravel() for m in np.meshgrid(g, g, g, indexing="ij")], 1)
        return np.ascontiguousarray(pts[np.random.default_rng(9).permutation(len(pts))])
    if name.startswith("lat_n"):
        return np.ascontiguousarray(cloud("lat")[:int(name[5:])])
    if name.startswith("lat_h"):
        half = cloud("lat")[cloud("lat")[:, 0] < 8]           # (in an order of its own: a point's index and its neighbour's are unrelated)
        return np.ascontiguousarray(half[np.random.default_rng(10).permutation(len(half))][:int(name[5:])])
    if name == "s1_odd":
        return np.ascontiguousarray(_odd(cloud("s1")))
    if name.startswith("s1_n"):
        xyz = cloud("s1")
        return np.ascontiguousarray(xyz[np.linspace(0, len(xyz) - 1, int(name[4:])).astype(np.int64)])
    if name == "far":
        w = synth.make_world(OTHER[0], n_boxes=OTHER[1], extent=OTHER[2])
        return np.ascontiguousarray(synth.lidar_scan(w, np.eye(4), seed=OTHER[0] + 10, n_az=N_AZ)[:, :3])
    k = 0 if name == "t" else int(name[1])
    w = synth.make_world(WORLD[0], n_boxes=WORLD[1], extent=WORLD[2])
    return np.ascontiguousarray(synth.lidar_scan(w, scan_poses()[k], seed=WORLD[0] + 10 + k, n_az=N_AZ)[:, :3])


def truth(src):
    """source frame -> the target's frame for the scans of the world; the identity for everything else."""
    if src[0] == "s" and src[1] in "123":
        return np.linalg.inv(scan_poses()[0]) @ scan_poses()[int(src[1])]
    return np.eye(4)


def _row(group, src, tgt, T=None, gate=0.6):
    return dict(group=group, src=src, tgt=tgt, T=None if T is None else np.ascontiguousarray(T, np.float32), gate=float(np.float32(gate)))


def _guess(src, k):
    yaw, t, roll = OFFSETS[k]
    return (truth(src) @ _se3(yaw, t, roll_deg=roll)).astype(np.float32)


def _shift(dx):
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = dx
    return T


ROWS = [_row("a", "lat_n%d" % n, "lat") for n in SIZES]
ROWS += [_row("b", "lat_h%d" % n, "lat", _shift(0.5), TIE_GATE) for n in HALF_SIZES]
ROWS += [_row("b0", "lat_h%d" % n, "lat", _shift(0.5), BELOW_TIE_GATE) for n in HALF_SIZES]
ROWS += [_row("c", "s%d" % (k + 1), "t", _guess("s%d" % (k + 1), k), gate) for gate in GATES for k in range(3)]
ROWS += [_row("d", "s1_odd", "t", _guess("s1", 0), gate) for gate in (0.6, 2.0)]
ROWS += [_row("e", "s1", "far", truth("s1")), _row("e", "far", "t")]
# (f): one list under the default gate; None: no target
MIXED = [_row("f", "s1_n1", "t", _guess("s1", 0)), _row("f", "s1_n257", "t", _guess("s1", 1)), _row("f", "s2", "t", _guess("s2", 1)),
         _row("f", "s1", None, _guess("s1", 0)), _row("f", "s3", "empty", _guess("s3", 2)), _row("f", "t", "t", _shift(0.05)),
         _row("f", "s1_odd", "t", _guess("s1", 0)), _row("f", "s2", "t", _guess("s2", 1)), _row("f", "lat_n65", "lat", _shift(0.25))]
TWICE = (2, 7)                                     # the row that stands at two positions of MIXED


def rows(group):
    return [r for r in ROWS if r["group"] == group]


def by_gate(rws):
    """gate -> the rows under it, in table order: a call takes ONE gate."""
    out = {}
    for r in rws:
        out.setdefault(r["gate"], []).append(r)
    return out


_REFS = {}


def reference(row, oracle):
    """The restatement's answer to a row (eval_ref.evaluate); computed once per process, never changed."""
    key = (row["src"], row["tgt"], None if row["T"] is None else row["T"].tobytes(), row["gate"])
    if key not in _REFS:
        tgt = cloud("empty") if row["tgt"] is None else cloud(row["tgt"])
        r = E.evaluate(cloud(row["src"]), tgt, row["T"], GC.finite_nn(oracle), row["gate"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]
