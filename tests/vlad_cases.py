"""The case table of the NetVLAD-FC head sweep (test_vlad_cases_cpu.py proves on the CPU that it can fail,
test_vlad_sweep_gpu.py runs it on the device) -- numpy only.

A case is (name, n, K, C, H, W, out, flags, branch): one dimension sits on an edge of a kernel's tiling, the others
are small.  `branch` names the code path the case is there for.  Flags: "nonorm" normalize_input = 0; "x30" features
scaled by 30; "pos" strictly positive features; "zero_img" image 1 all zero; "zero_cent" zero centroids; "gate" a
GatingContext behind the FC.  Cases at odd positions of the table have a 1x1-conv bias, even ones none.  Every case
is evaluated with a random dense FC and with a selection FC (vlad_ref.selection_fc) over vlad_ref.rows_of_interest;
a gated case selects as many rows as it has outputs, so that both runs share the gate.
"""
import collections
import functools

import numpy as np

import vlad_ref as R

Case = collections.namedtuple("Case", "name n K C H W out flags branch seed bias")

_TABLE = [
    # clusters: 1..4 MFMA tiles of 16 (one wave each), padded clusters, idle waves
    ("K1", 2, 1, 8, 3, 5, 4, "", "1 cluster tile with 15 padded clusters, 3 idle waves"),
    ("K15", 2, 15, 8, 3, 5, 4, "", "1 cluster tile, 1 padded cluster"),
    ("K16", 2, 16, 8, 3, 5, 4, "", "1 exact cluster tile"),
    ("K17", 2, 17, 8, 3, 5, 4, "", "2 cluster tiles, 15 padded clusters"),
    ("K33", 2, 33, 8, 3, 5, 4, "", "3 cluster tiles, padded, 1 idle wave"),
    ("K48", 2, 48, 8, 3, 5, 4, "", "3 exact cluster tiles, 1 idle wave"),
    ("K49", 2, 49, 8, 3, 5, 4, "", "4 cluster tiles, 15 padded clusters"),
    ("K63", 2, 63, 8, 3, 5, 4, "", "4 cluster tiles, 1 padded cluster"),
    ("K64", 2, 64, 8, 3, 5, 4, "", "4 exact cluster tiles"),
    # channels: steps of 16 with 4-wide MFMA operands, accumulator groups of 128
    ("C3", 2, 5, 3, 3, 5, 4, "", "channels: 4-wide MFMA operand tail"),
    ("C1_HW1", 1, 3, 1, 1, 1, 2, "pos", "channels: a single channel; positions: a lone padded tile of 1"),
    ("C15", 2, 5, 15, 3, 5, 4, "", "channels: 16-step tail, one short"),
    ("C16", 2, 5, 16, 3, 5, 4, "", "channels: one exact 16-step"),
    ("C17_nonorm", 2, 5, 17, 3, 5, 4, "nonorm", "channels: one into the next 16-step; normalize_input = 0"),
    ("C127", 2, 5, 127, 3, 5, 4, "", "channels: one short of the 128-channel accumulator group"),
    ("C128", 2, 5, 128, 3, 5, 4, "", "channels: one exact accumulator group"),
    ("C129", 2, 5, 129, 3, 5, 4, "", "channels: one into the second accumulator group"),
    ("C130", 2, 5, 130, 3, 5, 4, "", "channels: second group with a 2-wide operand tail"),
    ("C257", 2, 5, 257, 3, 5, 4, "", "channels: one into the third accumulator group"),
    ("C512", 2, 5, 512, 3, 5, 4, "", "channels: four exact accumulator groups"),
    ("C557_K64", 1, 64, 557, 3, 5, 4, "", "largest LDS tile with 64 clusters (76 B under 160 KiB)"),
    ("C560_K48", 1, 48, 560, 3, 5, 4, "", "largest channel count, 48 clusters"),
    # positions (tiles of 64) with FC rows (slabs of 512)
    ("HW1_KC6", 2, 2, 3, 1, 1, 4, "", "positions: lone padded tile; FC rows: 6, far below one slab"),
    ("HW63_KC512", 2, 4, 128, 1, 63, 4, "", "positions: one short of a tile; FC rows: one exact slab"),
    ("HW64_KC513", 2, 27, 19, 1, 64, 4, "", "positions: one exact tile; FC rows: slab tail of 1"),
    ("HW65_KC1024", 2, 8, 128, 1, 65, 4, "", "positions: one into the second tile; FC rows: two exact slabs"),
    ("HW72_KC2400", 2, 24, 100, 1, 72, 4, "", "positions: 8 into the second tile; FC rows: 4 slabs and a tail of 352"),
    ("HW128", 2, 5, 8, 1, 128, 4, "", "positions: two exact tiles"),
    ("HW130_nonorm", 2, 17, 129, 1, 130, 4, "nonorm", "positions: 2 into the third tile; normalize_input = 0"),
    ("x30_nonorm", 2, 3, 8, 5, 13, 4, "nonorm x30", "max-subtraction in the softmax: logits of +-100"),
    # images (FC passes of 8) with outputs (blocks of 256)
    ("n7_out1", 7, 5, 8, 3, 5, 1, "", "images: one short of an FC pass; outputs: 1"),
    ("n8_out3", 8, 5, 8, 3, 5, 3, "", "images: one exact FC pass; outputs: 3"),
    ("n9_out255", 9, 5, 8, 3, 5, 255, "", "images: one into the second FC pass; outputs: one short of a block"),
    ("n16_out256", 16, 5, 8, 3, 5, 256, "", "images: two exact FC passes; outputs: one exact block"),
    ("n17_out257", 17, 5, 8, 3, 5, 257, "", "images: third FC pass of 1; outputs: one into the second block"),
    ("out300", 2, 5, 8, 3, 5, 300, "", "outputs: second block of 44"),
    # degenerate images
    ("zero_img", 3, 5, 8, 3, 5, 4, "zero_img", "an all-zero image inside a batch, no bias"),
    ("zero_img_bias", 3, 5, 8, 3, 5, 4, "zero_img", "an all-zero image inside a batch, with bias"),
    ("zero_cent", 3, 5, 8, 3, 5, 4, "zero_img zero_cent", "zero centroids: the all-zero image gives exactly 0.0"),
    # the sizes the descriptors ship with
    ("i2i", 1, 64, 512, 48, 48, 512, "", "the image descriptor's head: every tile exact; a single image"),
    ("pillar", 2, 64, 128, 8, 24, 128, "", "the PointPillar descriptor's widths"),
    # gating: one wave per 64 outputs
    ("gate_out1", 1, 5, 32, 3, 5, 1, "gate", "gate: a single output"),
    ("gate_out63", 9, 5, 32, 3, 5, 63, "gate", "gate: one short of a wave"),
    ("gate_out64", 1, 5, 32, 3, 5, 64, "gate", "gate: one exact wave"),
    ("gate_out65", 9, 5, 32, 3, 5, 65, "gate", "gate: one into the second wave"),
    ("gate_out130", 1, 5, 32, 3, 5, 130, "gate", "gate: third wave of 2"),
    ("gate_out512", 9, 8, 64, 3, 5, 512, "gate", "gate: 8 exact waves"),
]
# a draw that test_vlad_cases_cpu.py refuses (a mutant it cannot tell apart) is replaced by changing the case's seed here
CASES = [Case(*t, seed=7000 + i, bias=bool(i % 2)) for i, t in enumerate(_TABLE)]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PRODUCTION = "i2i"
KINDS = ("dense", "selection")

Inputs = collections.namedtuple("Inputs", "x conv_w conv_b centroids fc rows normalize_input gating")


@functools.lru_cache(maxsize=4)
def inputs(case):
    """The case's arrays (float32).  fc is {"dense": ..., "selection": ...}; treat everything as read-only."""
    n, K, C, H, W, out = case.n, case.K, case.C, case.H, case.W, case.out
    fl = case.flags.split()
    rng = np.random.default_rng(case.seed)
    x = np.maximum(rng.standard_normal((n, C, H, W)), 0)
    if "pos" in fl:
        x = x + 0.5
    if "x30" in fl:
        x = x * 30.0
    if "zero_img" in fl:
        x[1] = 0.0
    x = x.astype(np.float32)
    w = (rng.standard_normal((K, C)) * 4.0 / np.sqrt(C)).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32) if case.bias else None
    cen = np.zeros((K, C), np.float32) if "zero_cent" in fl else rng.random((K, C)).astype(np.float32)
    dense = (rng.standard_normal((K * C, out)) / np.sqrt(C)).astype(np.float32)
    rows = R.rows_of_interest(K, C)
    gating = None
    if "gate" in fl:
        assert out <= len(rows)
        rows = rows[np.round(np.linspace(0, len(rows) - 1, out)).astype(int)] if out > 1 else rows[-1:]
        gw = (rng.standard_normal((out, out)) / np.sqrt(out)).astype(np.float32)
        scale = (rng.standard_normal(out) * 3.0).astype(np.float32)   # mixed signs
        shift = rng.standard_normal(out).astype(np.float32)
        shift[0] = 90.0           # sigmoid saturated at 1: expf(-90) underflows
        if out > 1:
            shift[-1] = -90.0     # ... and at 0: expf(90) overflows to inf
        gating = (gw, scale, shift)
    for a in (x, w, cen, dense, rows):
        a.setflags(write=False)
    return Inputs(x, w, b, cen, {"dense": dense, "selection": R.selection_fc(K, C, rows)}, rows, "nonorm" not in fl,
                  gating)


def reference64(case, mutant=0):
    """{"dense": y, "selection": y} in float64, the first half of the head evaluated once."""
    a = inputs(case)
    v = R.vlad64(a.x, a.conv_w, a.conv_b, a.centroids, a.normalize_input, mutant)
    return {"dense": R.head64(v, a.fc["dense"], a.gating, mutant),
            "selection": R.head64(v, None, a.gating, mutant, rows=a.rows)}


Bound = collections.namedtuple("Bound", "ref tol d_oracle d_ordered ulp")


@functools.lru_cache(maxsize=None)
def bounds(case):
    """{"dense": Bound, "selection": Bound}: the float64 result and
    tol = 4 max(|oracle32 - forward64|, |forward32_ordered - forward64|, 2^-23 max|forward64|), measured on the two
    float32 evaluations of the reference only -- never on a kernel's output."""
    from oracle import vlad_oracle
    a = inputs(case)
    ref = reference64(case)
    v32, inv = R.vlad32_ordered(a.x, a.conv_w, a.conv_b, a.centroids, a.normalize_input)
    res = {}
    for kind in KINDS:
        o32 = vlad_oracle.netvlad_fc_forward(a.x, a.conv_w, a.conv_b, a.centroids, a.fc[kind], a.normalize_input)
        if a.gating is not None:
            with np.errstate(over="ignore"):
                o32 = vlad_oracle.gating_forward(o32, *a.gating)
        s32 = R.fc32_ordered(v32, inv, a.fc[kind], a.gating)
        d_o = float(np.abs(o32 - ref[kind]).max())
        d_s = float(np.abs(s32 - ref[kind]).max())
        ulp = float(2.0 ** -23 * np.abs(ref[kind]).max())
        ref[kind].setflags(write=False)
        res[kind] = Bound(ref[kind], 4.0 * max(d_o, d_s, ulp), d_o, d_s, ulp)
    return res


def applies(case, mutant):
    """Whether the mutant is a different computation on this case at all."""
    fl = case.flags.split()
    return {R.M_LAST_CLUSTER: case.K >= 2, R.M_NO_BIAS: case.bias, R.M_LAST_IMAGE: case.n >= 2,
            R.M_PADDED_WEIGHT: (case.H * case.W) % R.TILE != 0 and "zero_cent" not in fl,
            R.M_GATE_SHIFT: "gate" in fl}.get(mutant, True)
