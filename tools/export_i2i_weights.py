"""Export the i2i model's weights for the command line (global_localization VALSET POSES MODEL):

    python tools/export_i2i_weights.py MODEL OUT

MODEL is what the reference's C++ loads (i2i_vgg_vlad.pt, traced by s2s_libtorch/gen_libtorch_i2i.py) or a training
checkpoint of VGGVLAD (`encoder.*` + `pool.*`, bare or under "state_dict").  OUT is a GLOCI2IW file, little-endian:
"GLOCI2IW", u32 version (1), u32 layers (13), per layer u32 cout, u32 cin, w [cout][cin][3][3] f32, b [cout] f32;
then u32 clusters, dim, out_dim, has_bias, conv_w [clusters][dim], conv_b [clusters] (if has_bias),
centroids [clusters][dim], fc_w [clusters * dim][out_dim] (NetVLAD's hidden1_weights), all f32.
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAGIC = b"GLOCI2IW"
VERSION = 1


def load_model(path):
    """i2i weights (gloc3d_amd.i2i.i2i_weights layout) from a TorchScript module or a checkpoint."""
    import torch
    from gloc3d_amd import i2i
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except (RuntimeError, ValueError):
        sd = torch.load(path, map_location="cpu", weights_only=False)
    return i2i.i2i_weights(sd)


def write(path, w):
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<II", VERSION, len(w["encoder"])))
        for wt, b in w["encoder"]:
            f.write(struct.pack("<II", wt.shape[0], wt.shape[1]))
            f.write(np.ascontiguousarray(wt, "<f4").tobytes())
            f.write(np.ascontiguousarray(b, "<f4").tobytes())
        K, D = w["conv_w"].shape
        has_bias = w["conv_b"] is not None
        f.write(struct.pack("<IIII", K, D, w["fc_w"].shape[1], int(has_bias)))
        f.write(np.ascontiguousarray(w["conv_w"], "<f4").tobytes())
        if has_bias:
            f.write(np.ascontiguousarray(w["conv_b"], "<f4").tobytes())
        f.write(np.ascontiguousarray(w["centroids"], "<f4").tobytes())
        f.write(np.ascontiguousarray(w["fc_w"], "<f4").tobytes())


def read(path):
    """The inverse of write(): the same dict."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != MAGIC:
        raise ValueError(f"{path}: not a GLOCI2IW file")
    version, n = struct.unpack_from("<II", data, 8)
    if version != VERSION:
        raise ValueError(f"{path}: version {version}")
    off = 16

    def arr(count, shape):
        nonlocal off
        a = np.frombuffer(data, "<f4", count, off).reshape(shape).astype(np.float32)
        off += 4 * count
        return a

    enc = []
    for _ in range(n):
        co, ci = struct.unpack_from("<II", data, off)
        off += 8
        enc.append((arr(co * ci * 9, (co, ci, 3, 3)), arr(co, (co,))))
    K, D, O, has_bias = struct.unpack_from("<IIII", data, off)
    off += 16
    conv_w = arr(K * D, (K, D))
    conv_b = arr(K, (K,)) if has_bias else None
    out = dict(encoder=enc, conv_w=conv_w, conv_b=conv_b, centroids=arr(K * D, (K, D)), fc_w=arr(K * D * O, (K * D, O)))
    if off != len(data):
        raise ValueError(f"{path}: {len(data) - off} trailing bytes")
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    write(argv[2], load_model(argv[1]))
    print(f"wrote {argv[2]} ({os.path.getsize(argv[2])} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
