"""PointPillar front-end timing (not bench.py): the [P, 16] model input and the PointNet canvas of synthetic 64 x 2000-ray
scans at P = 122480 and B = 1, 8, 64 through the device entry points on torch's stream; the per-kernel profile; the
voxel-0 chain on its own; the torch backbone and the HIP NetVLAD-FC head; the numpy restatement on this host.

    python tools/pillar_timing.py [--reps 10] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("pillar_classify", "pillar_sort", "pillar_runs", "pillar_voxel", "pillar_gather", "pillar_partial",
           "pillar_canvas")
# bytes per row each kernel moves at least (4-byte words): classify reads a point, writes key, row, flag; two sort passes
# read and write (key, row) three times; runs reads the keys; voxel reads row, flag and xyz; gather reads the point and
# two voxel records, writes 64 B; partial + canvas read the row index, flag and 60 B of the input row once
ROW_BYTES = {"inputs": 16 + 12 + 2 * 3 * 16 + 4 + 20 + 16 + 20 + 64, "canvas_extra": 4 + 4 + 60}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pillar_ref as R
    from gloc3d_amd import capi, synth
    from gloc3d_amd.pillar import PillarBackbone
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    w = synth.make_world(7)
    base = [synth.lidar_scan(w, synth.se3(30.0 * k, (3.0 * k, -2.0 * k, 0)), 100 + k) for k in range(8)]
    p = capi.default_pillar_params()
    P = p.num_points
    grid = R.Grid()
    m = [R.voxelize(*R.pad_scan(s, P), grid) for s in base]
    v0 = [int((x["index"] == 0).sum() - (P - min(len(s), P))) for x, s in zip(m, base)]
    say(f"scans: 64 x 2000 rays to 80 m, {min(map(len, base))}..{max(map(len, base))} returns; P = {P}; "
        f"voxel-0 chain (rows summed in order) {min(v0)}..{max(v0)} rows per scan")
    dev = torch.device("cuda", 0)
    enc = capi.PillarEncoder()
    sd = R.seeded_state_dict({"encoder.pn.pointnet.0.weight": (64, 14, 1), "encoder.pn.pointnet.1.weight": (64,),
                              "encoder.pn.pointnet.1.bias": (64,), "encoder.pn.pointnet.1.running_mean": (64,),
                              "encoder.pn.pointnet.1.running_var": (64,)})
    enc.set_pointnet(*R.pn_params_from_state(sd))
    stream = torch.cuda.Stream(dev)       # not the default stream: its handle 0 means "the handle's own stream" to the C ABI
    torch.cuda.set_stream(stream)
    enc.set_stream(stream.cuda_stream)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        return float(np.median(t))

    def batch(scans):
        off = np.zeros(len(scans) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in scans])
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(scans))).to(dev), off

    for B in (1, 8, 64):
        scans = [base[k % 8] for k in range(B)]
        pts, off = batch(scans)
        oi = torch.empty((B, P, 16), device=dev)
        oc = torch.empty((B, 64, grid.nv), device=dev)
        ti = timed(lambda: enc.inputs_device(pts.data_ptr(), off, 4, oi.data_ptr(), p), a.reps)
        tc = timed(lambda: enc.canvas_device(pts.data_ptr(), off, 4, oc.data_ptr(), p), a.reps)
        gb_i = ROW_BYTES["inputs"] * P * B / 1e9
        gb_c = (ROW_BYTES["inputs"] + ROW_BYTES["canvas_extra"]) * P * B / 1e9 + 64 * grid.nv * 4 * B / 1e9
        say(f"B = {B:2d}: inputs {ti / B:7.3f} ms per scan ({ti:7.3f} per batch, >= {gb_i * 1e3 / B:.1f} MB per scan, "
            f"{gb_i / ti * 1e3:6.0f} GB/s);  canvas {tc / B:7.3f} ms per scan ({tc:7.3f} per batch, {gb_c / tc * 1e3:6.0f} GB/s)")
        enc.set_profile(True)
        enc.profile_reset()
        for _ in range(a.reps):
            enc.canvas_device(pts.data_ptr(), off, 4, oc.data_ptr(), p)
        prof = {k: enc.profile(k) for k in KERNELS}
        enc.set_profile(False)
        say("    kernel ms per batch (profiled canvas call): " +
            ", ".join(f"{k[7:]} {t / a.reps:.3f}" for k, (t, n) in prof.items()))
        # the voxel-0 chain on its own: the voxel kernel with and without the out-of-range rows
        inr = [s[~R.voxelize(*R.pad_scan(s, len(s)), grid)["pad"]] for s in scans]
        pts2, off2 = batch(inr)
        enc.set_profile(True)
        enc.profile_reset()
        for _ in range(a.reps):
            enc.inputs_device(pts2.data_ptr(), off2, 4, oi.data_ptr(), p)
        t_in = enc.profile("pillar_voxel")[0] / a.reps
        enc.set_profile(False)
        say(f"    voxel kernel {prof['pillar_voxel'][0] / a.reps:.3f} ms with the out-of-range rows, {t_in:.3f} ms with "
            f"only in-range rows: the voxel-0 chain costs {prof['pillar_voxel'][0] / a.reps - t_in:.3f} ms per batch")
        del oi, oc, pts, pts2

    # backbone (torch, plumbing) and the NetVLAD-FC head (HIP)
    bb = PillarBackbone(140, 80).to(dev).eval()
    pool = capi.NetVladFC(np.asarray(R.seeded_param("pool.conv.weight", (64, 128, 1, 1))).reshape(64, 128),
                          R.seeded_param("pool.centroids", (64, 128)), R.seeded_param("pool.hidden1_weights", (8192, 128)))
    capi.lib().gloc_vlad_set_stream(pool._h, capi.C.c_void_p(stream.cuda_stream))
    for B in (1, 8, 64):
        cv = torch.rand((B, 64, grid.nv), device=dev)
        with torch.no_grad():
            tb = timed(lambda: bb(cv), a.reps)
            feat = bb(cv).contiguous()
        out = torch.empty((B, 128), device=dev)
        tv = timed(lambda: pool.forward_device(feat.data_ptr(), B, 80 * 140, out.data_ptr()), a.reps)
        say(f"B = {B:2d}: backbone (torch fp32) {tb / B:7.3f} ms per scan; NetVLAD-FC {tv / B:7.3f} ms per scan")
    pool.close()
    enc.close()

    # the numpy restatement on this host, one scan
    t0 = time.perf_counter()
    pts_, mask_ = R.pad_scan(base[0], P)
    inp, v = R.inputs16(pts_, mask_, grid)
    t1 = time.perf_counter()
    R.canvas(inp, v["pad"], grid, R.pn_params_from_state(sd))
    t2 = time.perf_counter()
    say(f"numpy restatement on this host, one scan: inputs {1e3 * (t1 - t0):.1f} ms, canvas {1e3 * (t2 - t1):.1f} ms more")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
