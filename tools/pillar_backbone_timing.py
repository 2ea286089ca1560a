"""PointPillar backbone timing (not bench.py): the HIP backbone (gloc_pillar_backbone_device) against the torch
PillarBackbone (fp32 nn.Conv2d) on the same canvases of synthetic 64 x 2000-ray scans at B = 1, 8, 64; the per-layer
profile with TFLOP/s in fp32-equivalent units (2 x multiply-adds of the convolution, not the three bf16 products); the
whole descriptor from host scans to host descriptors (PillarVladDescriptor, backbone="hip" and "torch").

    python tools/pillar_backbone_timing.py [--reps 10] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GX, GY = 140, 80


def layer_flops(capi):
    """fp32-equivalent FLOP per scan of each layer (2 x multiply-adds) at the reference grid."""
    sides = {0: 1, 1: 1, 2: 2, 3: 2, 4: 2, 5: 4, 6: 4, 7: 4}   # output side divisor
    out = []
    for layer in range(13):
        ci, co, _, _ = capi.pillar_backbone_layer_shape(layer)
        d = sides.get(layer, 1)
        out.append(2.0 * (-(-GX // d)) * (-(-GY // d)) * co * ci * 9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from gloc3d_amd import capi, synth
    from gloc3d_amd.pillar import PillarBackbone, PillarVladDescriptor, backbone_layers
    from test_pillar_backbone_abi import seeded_pillar_vlad_sd
    import pillar_ref as R
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    dev = torch.device("cuda", 0)
    sd = seeded_pillar_vlad_sd()
    enc = capi.PillarEncoder()
    enc.set_pointnet(*R.pn_params_from_state(sd))
    for layer, args in enumerate(backbone_layers(sd)):
        enc.set_backbone_layer(layer, *args)
    stream = torch.cuda.Stream(dev)       # not the default stream: its handle 0 means "the handle's own stream" to the C ABI
    torch.cuda.set_stream(stream)
    enc.set_stream(stream.cuda_stream)
    tb = PillarBackbone(GX, GY)
    tb.load_state_dict({k[len("encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()
                        if k.startswith("encoder.") and not k.startswith(("encoder.pn.", "encoder.conv_out_pose."))})
    tb = tb.to(dev).eval()

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

    w = synth.make_world(7)
    base = [synth.lidar_scan(w, synth.se3(30.0 * k, (3.0 * k, -2.0 * k, 0)), 100 + k) for k in range(8)]
    cv8 = torch.from_numpy(enc.canvas(base)).to(dev)
    flops = layer_flops(capi)
    say(f"backbone: 13 convolutions at {GX} x {GY}, {sum(flops) / 1e9:.1f} GFLOP per scan fp32-equivalent "
        f"({3 * sum(flops) / 1e9:.0f} GFLOP of bf16 MFMA work); canvases of 8 synthetic scans, repeated; "
        f"median of {a.reps} after a warm-up")
    for B in (1, 8, 64):
        cv = cv8[torch.arange(B) % 8].contiguous()
        out = torch.empty((B, 128, GX * GY), device=dev)
        th = timed(lambda: enc.backbone_device(cv.data_ptr(), B, GX, GY, out.data_ptr()), a.reps)
        with torch.no_grad():
            tt = timed(lambda: tb(cv), a.reps)
            ref = tb(cv).contiguous().view(B, 128, -1)
        err = float((out - ref).abs().max() / ref.abs().max())
        say(f"B = {B:2d}: HIP {th / B:6.3f} ms per scan ({th:8.3f} per batch, {sum(flops) * B / th / 1e9:5.0f} TFLOP/s)"
            f";  torch {tt / B:6.3f} ms per scan ({tt:8.3f} per batch);  torch / HIP {tt / th:4.2f}x;  "
            f"max|HIP - torch| {err:.1e} max|torch|")
        enc.set_profile(True)
        enc.profile_reset()
        for _ in range(a.reps):
            enc.backbone_device(cv.data_ptr(), B, GX, GY, out.data_ptr())
        prof = {k: enc.profile(k)[0] / a.reps for k in
                [f"pillar_conv{i}" for i in range(13)] + ["pillar_upsample", "pillar_layout"]}
        enc.set_profile(False)
        say("    per layer, ms per batch (TFLOP/s): " + ", ".join(
            f"{i} {prof[f'pillar_conv{i}']:.3f} ({flops[i] * B / prof[f'pillar_conv{i}'] / 1e9:.0f})" for i in range(13)) +
            f"; upsample {prof['pillar_upsample']:.3f}, layout {prof['pillar_layout']:.3f}")
        del out, cv
    # the whole descriptor: host scans -> host descriptors
    for name in ("hip", "torch"):
        d = PillarVladDescriptor(sd, backbone=name)
        for B in (1, 8):
            scans = base[:B]
            d(scans)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                d(scans)                                  # ends with the descriptors copied to the host
                ts.append(1e3 * (time.perf_counter() - t0))
            t = float(np.median(ts))
            say(f"descriptor, backbone={name}: B = {B}: {t / B:6.3f} ms per scan from host scans to host descriptors")
        d.close()
    enc.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
