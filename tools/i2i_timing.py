"""i2i descriptor timing (not bench.py): the HIP VGG16 encoder at 768 x 768 for B = 1, 8, 32 through the device entry
point on a torch stream, its per-layer kernel time from gloc_vgg_profile and the TFLOP/s it reaches, the same stack as
torch nn.Conv2d (MIOpen, fp32) with the same weights and inputs, and the whole descriptor (HIP BEV + encoder + NetVLAD-FC)
per scan.  Warm-up first, then the median of --reps timed repetitions (HIP events); the clocks are not pinned, so read
the numbers as of this box at this time.

    python tools/i2i_timing.py [--reps 10] [--out profiles/i2i_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HW = 768


def layer_macs(H, W):
    """Multiply-adds of each of the 13 convolutions at input H x W (VGG16 features[:-2])."""
    from gloc3d_amd import i2i
    out, h, w = [], H, W
    for li in range(13):
        ci, co, _, pool = i2i._shape(li)
        out.append(h * w * co * 9 * ci)
        if pool:
            h, w = h // 2, w // 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,32")
    a = ap.parse_args()
    import torch
    import i2i_ref as R
    from gloc3d_amd import i2i, synth
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    dev = torch.device("cuda", 0)
    sd = R.make_state_dict(R.SEED)
    model = i2i.I2iVladDescriptor.from_state_dict(sd)
    enc = model.encoder
    stream = model.stream
    torch.cuda.set_stream(stream)
    macs = layer_macs(HW, HW)
    say(f"VGG16 features[:-2] at {HW} x {HW}: {sum(macs) / 1e9:.1f} G multiply-adds = {2 * sum(macs) / 1e9:.1f} GFLOP "
        f"per scan; split-bf16 form (three bf16 MFMA products per fp32 product); median of {a.reps} after warm-up")

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

    g = np.load(os.path.join(ROOT, "tests", "golden", "i2i_full.npz"))
    x = np.unpackbits(g["bits"])[:3 * HW * HW].reshape(1, 3, HW, HW).astype(np.float32)
    feat, desc = model.describe_images(torch.from_numpy(x).to(dev))
    ef = np.abs(feat.cpu().numpy().reshape(-1)[g["idx"]] - g["feat_sample"]).max() / g["feat_absmax"]
    ed = np.abs(desc.cpu().numpy() - g["desc"]).max() / np.abs(g["desc"]).max()
    say(f"accuracy at {HW} x {HW} against the fp32 CPU goldens: feature map {ef:.2e} x max|ref| (sample of 4096), "
        f"descriptor {ed:.2e} x max|ref|")
    rng = np.random.default_rng(3)
    tm = R.encoder(sd).to(dev).eval()
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.from_numpy(R.binary_image(rng, B, HW, HW, fill=0.08, inner=(600, 520))).to(dev)
        feat = torch.empty((B, 512, HW // 16, HW // 16), device=dev)
        t = timed(lambda: enc.forward_device(x.data_ptr(), B, HW, HW, feat.data_ptr()), a.reps)
        enc.profile_reset()
        enc.set_profile(True)
        enc.forward_device(x.data_ptr(), B, HW, HW, feat.data_ptr())
        per = [enc.profile(f"vgg_conv{l}")[0] for l in range(13)]
        enc.set_profile(False)
        say(f"B = {B:2d}: HIP encoder {t / B:7.3f} ms per scan ({t:8.3f} per batch, {2 * sum(macs) * B / t / 1e9:6.1f} "
            f"TFLOP/s fp32-equivalent)")
        say("    per layer, ms per batch (TFLOP/s): " + ", ".join(
            f"conv{l} {per[l]:.3f} ({2 * macs[l] * B / max(per[l], 1e-9) / 1e9:.0f})" for l in range(13)))
        with torch.no_grad():
            tt = timed(lambda: tm(x), max(3, a.reps // 2))
        say(f"        torch nn.Conv2d stack (MIOpen, fp32) {tt / B:7.3f} ms per scan ({tt:8.3f} per batch); "
            f"HIP / torch = {t / tt:.2f}")
        del x, feat
        torch.cuda.empty_cache()

    w = synth.make_world(7)
    base = [synth.lidar_scan(w, synth.se3(30.0 * k, (3.0 * k, -2.0 * k, 0)), 100 + k) for k in range(8)]
    for B in (1, 8):
        scans = [base[k % 8] for k in range(B)]
        t = timed(lambda: model(scans), max(3, a.reps // 2))
        say(f"B = {B:2d}: whole descriptor (host scans -> BEV -> encoder -> NetVLAD-FC -> host) {t / B:7.3f} ms per scan")
    model.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
