"""CPU: the planner of the coarse descriptor kNN search (gloc3d_amd/csrc/knn_plan.hpp).  Every decision of a search --
coarse kernel and tile, K split, grid, selection form, redo form -- is made by plan_search() before anything is launched;
tests/knn_plan_probe.cpp prints its plans, and what the kernels assume of a plan is asserted here over a sweep of shapes,
plain and with the probe built under the address and undefined-behaviour sanitizers (windows up to 2^31 - 1 rows)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = (1, 2, 3, 8, 9, 16, 17, 32, 33, 64, 65, 130, 1024)
N_RANGE = (64, 100, 4541, 10000, 16384, 16385, 40001, 98304, 125000, 524288, 524320, 6000000, 2**31 - 1)
FIRST = (0, 13, 63)        # the window's first row: the split-bf16 form's grid starts at the head of its mirror tile
DIM = (4, 8, 24, 64, 100, 256, 2048, 4096, 4104)
K = (1, 20, 21, 52)
CANDIDATES = (1, 32)
COLUMNS = ("nq n_range first dim k cand fp32 b3 t32 WQ NT KS BQ BN kps gx gy gz ld qpad strideP KC qraw use_bmin n_blocks "
           "large fused sel sel_S sel_L redo redo_sel redo_S redo_L eps_d eps_n").split()
WINDOW, BLOCK_MINIMA, SLICES, CHUNKS = range(4)             # knn_plan.hpp: enum class Selection
IN_LAUNCH, ONE_LAUNCH, FLAGGED_EXACT, HOST_READ_BACK = range(4)  # enum class Redo
FP32_TILES = ((4, 2), (4, 3), (4, 4), (4, 5), (4, 6), (4, 8), (2, 2), (2, 4), (1, 1), (1, 2))  # knn.hip: the MF() instances


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_plan_is_one_the_kernels_can_run(tmp_path, sanitize):
    exe = tmp_path / "knn_plan_probe"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + os.path.join(ROOT, "gloc3d_amd", "csrc"),
                           os.path.join(ROOT, "tests", "knn_plan_probe.cpp"), "-o", str(exe)])
    shapes = itertools.product(NQ, N_RANGE, FIRST, DIM, K, CANDIDATES, (0, 1))
    text = "".join("%d %d %d %d %d %d %d\n" % s for s in shapes)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout   # (a sanitizer report: exit != 0)
    consts, _, body = out.partition("\n")
    SELQ_MAX_ROWS, SRR_KC, SRR_G, MIR_ROWS = (int(t) for t in consts.split())
    assert SELQ_MAX_ROWS == 16384 and MIR_ROWS == 64
    plans = np.array(body.split(), dtype=np.int64).reshape(-1, len(COLUMNS))
    assert plans.shape[0] == len(NQ) * len(N_RANGE) * len(FIRST) * len(DIM) * len(K) * len(CANDIDATES) * 2
    c = {name: plans[:, i] for i, name in enumerate(COLUMNS)}
    (nq, n, first, dim, k, cand, fp32, b3, t32, WQ, NT, KS, BQ, BN, kps, gx, gy, gz, ld, qpad, strideP, KC, qraw, use_bmin,
     n_blocks, large, fused, sel, sel_S, sel_L, redo, redo_sel, redo_S, redo_L, eps_d, eps_n) = (c[x] for x in COLUMNS)

    def every(cond, what):
        bad = np.flatnonzero(~cond)
        assert bad.size == 0, f"{what}: {bad.size} plans, the first {dict(zip(COLUMNS, plans[bad[0]].tolist()))}"

    def implies(a, b, what):
        every(~a.astype(bool) | b, what)

    def ceil_div(a, b):
        return (a + b - 1) // b

    b3, t32, qraw, use_bmin, large, fused = (x.astype(bool) for x in (b3, t32, qraw, use_bmin, large, fused))
    # the coarse kernel has an instance
    tiles = ~b3 & ~t32
    every(~(b3 & t32), "two coarse kernels at once")
    every(b3 == ((dim % 8 == 0) & (fp32 == 0)), "the split-bf16 form exactly when dim % 8 == 0 and fp32_only is off")
    implies(b3, ((NT == 1) | (NT == 2)) & (BQ == 64) & (BN == 64 * NT), "split-bf16 tile")
    implies(t32, (WQ == 4) & (NT == 2) & (KS == 1) & (BQ == 64) & (BN == 128), "the one 32 x 32 plan")
    implies(tiles, np.isin(WQ * 100 + NT, [w * 100 + t for w, t in FP32_TILES]), "no dist_mfma_kernel<WQ, NT> instance")
    implies(tiles, (BQ == 16 * WQ) & (BN == 16 * NT * (4 // np.maximum(WQ, 1))), "fp32 tile size")
    # K splits: whole 64-float steps that cover dim
    every(np.isin(KS, [1, 2, 4, 8, 16]), "KS")
    implies(KS > 1, (dim % (128 * KS // 2) == 0) & (dim // KS >= 128), "a K split of partial or short steps")
    every((kps % 64 == 0) & (kps * KS >= dim) & (kps < ceil_div(dim, KS) + 64), "K per split")
    # the grid covers queries and rows (the split-bf16 form: from the head of the first mirror tile) and is launchable
    every((gy == ceil_div(nq, BQ)) & (gz == KS) & (gy <= 65535), "grid y / z")
    every(gx == ceil_div(np.where(b3, first % MIR_ROWS, 0) + n, BN), "grid x")
    every(gx < 2**31, "grid x")
    every((ld == ceil_div(n, 64) * 64) & (qpad == gy * BQ) & (strideP == qpad * ld), "partial-dot layout")
    every(KC == np.maximum(cand, np.minimum(64, k + 12)), "KC")
    every(qraw == (b3 & (ceil_div(n, BN) * gy * gz <= 768)), "queries split in-kernel up to 768 work-groups")
    every(large == (n > SELQ_MAX_ROWS), "large")

    def slices_ok(on, S, L, lists, what):   # what select_slices_kernel / flagged_redo_kernel and the kernel over their lists assume
        implies(on, (L % 64 == 0) & (L > 0) & (L <= SELQ_MAX_ROWS) & (S >= 1) & (S <= 65535), what + ": slice length / count")
        implies(on, ((S - 1) * L < n) & (n <= S * L), what + ": an empty slice or uncovered rows")
        implies(on, S * lists <= SELQ_MAX_ROWS, what + ": the lists do not fit one work-group")

    slices_ok(sel == SLICES, sel_S, sel_L, KC, "selection")
    slices_ok(redo == ONE_LAUNCH, redo_S, redo_L, k, "redo launch")
    slices_ok((redo == FLAGGED_EXACT) & (redo_sel == SLICES), redo_S, redo_L, k, "flagged exact pass")
    # block minima
    implies(use_bmin, b3 & (n > SELQ_MAX_ROWS) & (KS == 1) & (n_blocks <= SELQ_MAX_ROWS) & (KC <= SRR_KC) & (dim <= 4 * SRR_G),
            "block minima")
    implies(use_bmin, (n_blocks == gx * (BN // 32)) & fused, "block minima: blocks / fused")
    every(use_bmin == (sel == BLOCK_MINIMA), "block minima selected exactly when they are made")
    # the selection
    implies(fused, (KC <= SRR_KC) & (dim <= 4 * SRR_G), "fused beyond the kernel's candidate rows")
    implies(fused, np.where(large, (sel == BLOCK_MINIMA) | (sel == SLICES), sel == WINDOW), "fused selection form")
    implies(~fused, np.where(large, (sel == SLICES) | (sel == CHUNKS), sel == WINDOW), "separate selection form")
    # the redo: in the fused launch for small windows; else on the device wherever the lists of the fewest slices fit one
    # work-group (plan_slices adds slices only while they still fit), and only then by the host's read-back
    s0 = ceil_div(n, SELQ_MAX_ROWS)
    every((redo == IN_LAUNCH) == (fused & ~large), "redo inside the launch")
    every((redo == HOST_READ_BACK) == ((redo != IN_LAUNCH) & ((s0 * k > SELQ_MAX_ROWS) | (s0 > 65535))), "host read-back")
    implies(redo == HOST_READ_BACK, n > SELQ_MAX_ROWS, "host read-back of a small window")
    implies(redo == ONE_LAUNCH, fused & large, "redo launch")
    implies(redo == FLAGGED_EXACT, redo_sel != CHUNKS, "flagged exact pass that cannot replace a result written already")
    # rounding bounds: positive, the split-bf16 form's at least its 1160 u
    u = 2.0 ** -24
    every((eps_d.astype(np.uint32).view(np.float32) > 0) & (eps_n.astype(np.uint32).view(np.float32) > np.where(b3, 1160, 64) * u),
          "rounding bound")
    # the sweep reaches every form
    assert set(np.unique(sel)) == {WINDOW, BLOCK_MINIMA, SLICES, CHUNKS}
    assert set(np.unique(redo)) == {IN_LAUNCH, ONE_LAUNCH, FLAGGED_EXACT, HOST_READ_BACK}
    assert b3.any() and t32.any() and tiles.any() and set(np.unique(KS)) == {1, 2, 4, 8, 16}
