"""Export the PointPillar-NetVLAD scan model's weights for the command line (s2s_feature_extract WEIGHTS SCAN.bin ...):

    python tools/export_pillar_weights.py CHECKPOINT OUT

CHECKPOINT is a PointPillarVLAD state_dict (`encoder.*` + `pool.*`, bare or under "state_dict") or a TorchScript export
of the model (s2s_libtorch/gen_libtorch_pointpillar.py); `encoder.conv_out_pose.*` is ignored.  OUT is a GLOCPPW file,
little-endian:
  "GLOCPPW\\0", u32 version (1);
  PointNet: u32 cout (64), u32 cin (14), w [cout][cin], BatchNorm1d weight, bias, running mean, running var [cout],
            f32 eps;
  u32 layers (13), per backbone layer (include/gloc3d.h, gloc_pillar_backbone_layer_shape): u32 cout, u32 cin,
            w [cout][cin][3][3], BatchNorm2d weight, bias, running mean, running var [cout], f32 eps;
  NetVLAD-FC: u32 clusters, dim, out_dim, has_bias, conv_w [clusters][dim], conv_b [clusters] (if has_bias),
            centroids [clusters][dim], fc_w [clusters * dim][out_dim] (hidden1_weights);
all arrays f32.  eps is torch's default, 1e-5: the reference's modules leave it there, and a state_dict does not hold it.
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAGIC = b"GLOCPPW\0"
VERSION = 1
EPS = 1e-5


def pillar_weights(sd, eps=EPS):
    """{pointnet: (w [64, 14], bn_w, bn_b, mean, var, eps), backbone: 13 x (w, bn_w, bn_b, mean, var, eps), conv_w,
    conv_b, centroids, fc_w} from a PointPillarVLAD state_dict (torch tensors or numpy arrays)."""
    from gloc3d_amd.pillar import BACKBONE_KEYS
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    f = lambda v: np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32)
    sd = {k: f(v) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    bn = lambda p: (sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"])
    pn = "encoder.pn.pointnet."
    conv_w = sd["pool.conv.weight"]
    return dict(pointnet=(sd[pn + "0.weight"].reshape(sd[pn + "0.weight"].shape[0], -1),) + bn(pn + "1") + (eps,),
                backbone=[(sd["encoder." + c + ".weight"],) + bn("encoder." + b) + (eps,) for c, b in BACKBONE_KEYS],
                conv_w=conv_w.reshape(conv_w.shape[0], -1), conv_b=sd.get("pool.conv.bias"),
                centroids=sd["pool.centroids"], fc_w=sd["pool.hidden1_weights"])


def load_model(path):
    import torch
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except (RuntimeError, ValueError):
        sd = torch.load(path, map_location="cpu", weights_only=False)
    return pillar_weights(sd)


def _arr(f, a):
    f.write(np.ascontiguousarray(a, "<f4").tobytes())


def write(path, w):
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<I", VERSION))
        pw = w["pointnet"]
        f.write(struct.pack("<II", pw[0].shape[0], pw[0].shape[1]))
        for a in pw[:5]:
            _arr(f, a)
        f.write(struct.pack("<f", pw[5]))
        f.write(struct.pack("<I", len(w["backbone"])))
        for layer in w["backbone"]:
            f.write(struct.pack("<II", layer[0].shape[0], layer[0].shape[1]))
            for a in layer[:5]:
                _arr(f, a)
            f.write(struct.pack("<f", layer[5]))
        K, D = w["conv_w"].shape
        has_bias = w["conv_b"] is not None
        f.write(struct.pack("<IIII", K, D, w["fc_w"].shape[1], int(has_bias)))
        _arr(f, w["conv_w"])
        if has_bias:
            _arr(f, w["conv_b"])
        _arr(f, w["centroids"])
        _arr(f, w["fc_w"])


def read(path):
    """The inverse of write(): the same dict."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != MAGIC:
        raise ValueError(f"{path}: not a GLOCPPW file")
    (version,) = struct.unpack_from("<I", data, 8)
    if version != VERSION:
        raise ValueError(f"{path}: version {version}")
    off = 12

    def u32(k):
        nonlocal off
        v = struct.unpack_from("<" + "I" * k, data, off)
        off += 4 * k
        return v

    def f32():
        nonlocal off
        (v,) = struct.unpack_from("<f", data, off)
        off += 4
        return v

    def arr(count, shape):
        nonlocal off
        a = np.frombuffer(data, "<f4", count, off).reshape(shape).astype(np.float32)
        off += 4 * count
        return a

    co, ci = u32(2)
    pointnet = (arr(co * ci, (co, ci)),) + tuple(arr(co, (co,)) for _ in range(4)) + (f32(),)
    backbone = []
    for _ in range(u32(1)[0]):
        co, ci = u32(2)
        backbone.append((arr(co * ci * 9, (co, ci, 3, 3)),) + tuple(arr(co, (co,)) for _ in range(4)) + (f32(),))
    K, D, O, has_bias = u32(4)
    conv_w = arr(K * D, (K, D))
    conv_b = arr(K, (K,)) if has_bias else None
    out = dict(pointnet=pointnet, backbone=backbone, conv_w=conv_w, conv_b=conv_b, centroids=arr(K * D, (K, D)),
               fc_w=arr(K * D * O, (K * D, O)))
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
