"""The i2i model restated for tests: seeded weights in the reference's checkpoint layout, and NetVLAD.forward
(model/netvlad_fc.py:73-109, normalize_input = True, vladv2 = False, no gating) in torch.  The VGG16 encoder itself is
gloc3d_amd.i2i.vgg16_encoder.  Weights are generated, never stored (59 MB of convolutions plus 67 MB of FC)."""
import numpy as np
import torch
import torch.nn.functional as F

from gloc3d_amd import i2i

SEED = 20261016


def make_state_dict(seed=SEED):
    """He-scaled convolutions, small biases, and a NetVLAD-FC head (dim 512, 64 clusters, out 512), from numpy's
    default_rng (PCG64: the same numbers on every numpy version).  Keys as the reference's VGGVLAD checkpoint."""
    rng = np.random.default_rng(seed)
    sd = {}
    for li, i in enumerate(i2i.ENCODER_CONV_IDX):
        ci, co, _, _ = i2i._shape(li)
        sd[f"encoder.{i}.weight"] = (rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
        sd[f"encoder.{i}.bias"] = (rng.standard_normal(co) * 0.01).astype(np.float32)
    K, D = i2i.CLUSTERS, i2i.DIM
    sd["pool.conv.weight"] = rng.standard_normal((K, D, 1, 1)).astype(np.float32)
    sd["pool.centroids"] = (rng.standard_normal((K, D)) * 0.05).astype(np.float32)
    sd["pool.hidden1_weights"] = (rng.standard_normal((K * D, i2i.OUT_DIM)) / np.sqrt(D)).astype(np.float32)
    return sd


def encoder(sd):
    """vgg16_encoder() with the `encoder.*` weights of `sd` (numpy or torch values), fp32, CPU, eval."""
    m = i2i.vgg16_encoder()
    m.load_state_dict({k[len("encoder."):]: torch.as_tensor(np.asarray(v)) for k, v in sd.items()
                       if k.startswith("encoder.")})
    return m.eval()


def netvlad(x, sd):
    """NetVLAD.forward of the reference, vectorised over clusters (the same sums per cluster): x [N, 512, h, w]."""
    t = lambda v: v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))
    conv_w = t(sd["pool.conv.weight"]).reshape(i2i.CLUSTERS, i2i.DIM)
    cent, fc = t(sd["pool.centroids"]), t(sd["pool.hidden1_weights"])
    N, C = x.shape[:2]
    x = F.normalize(x, p=2, dim=1)
    soft = F.softmax(torch.einsum("kc,nchw->nkhw", conv_w, x).reshape(N, i2i.CLUSTERS, -1), dim=1)
    xf = x.reshape(N, C, -1)
    vlad = torch.einsum("nkp,ncp->nkc", soft, xf) - cent[None] * soft.sum(-1)[..., None]
    vlad = F.normalize(vlad, p=2, dim=2).reshape(N, -1)
    vlad = F.normalize(vlad, p=2, dim=1)
    return vlad @ fc


def binary_image(rng, n, H, W, fill=0.1, inner=None):
    """n BEV-like inputs [n, 3, H, W] in {0, 1}: an inner window of pixels (1 = free, 0 = occupied, the same in the
    three channels) inside the (1, 0, 0) padding that crop_pad_occupancy leaves (loop_detector.cpp:83-106)."""
    x = np.zeros((n, 3, H, W), np.float32)
    x[:, 0] = 1.0
    ih, iw = inner or (H * 3 // 4, W * 2 // 3)
    y0, x0 = (H - ih) // 2, (W - iw) // 3
    occ = (rng.random((n, ih, iw)) >= fill).astype(np.float32)
    x[:, :, y0:y0 + ih, x0:x0 + iw] = occ[:, None]
    return x
