"""Golden vectors for the i2i descriptor (VGG16 features[:-2] + NetVLAD-FC), made on the build machine:
    python tests/golden/make_i2i_goldens.py
The encoder is VGG16's layer list restated in torch (gloc3d_amd.i2i.vgg16_encoder: torchvision is not needed); the head
is the REFERENCE's own model/netvlad_fc.py NetVLAD (normalize_input = True, vladv2 = False, no gating), imported as
make_vlad_goldens.py does; both in fp32 on the CPU.  Weights come from tests/i2i_ref.make_state_dict(seed) and are not
stored.  Two cases:
  i2i_small.npz  two 96 x 80 binary images (u8), the encoder output [2, 512, 6, 5] and the descriptors [2, 512];
  i2i_full.npz   one 768 x 768 binary image, bit-packed; a fixed sample of 4096 encoder outputs of [1, 512, 48, 48]
                 (flat indices + values) and the descriptor [1, 512]."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/ (i2i_ref)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository (gloc3d_amd)
import i2i_ref  # noqa: E402
from gloc3d_amd import i2i  # noqa: E402

REF = "/root/reference/model/netvlad_fc.py"


def reference_head(sd):
    spec = importlib.util.spec_from_file_location("ref_netvlad_fc", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    m = ref.NetVLAD(num_clusters=i2i.CLUSTERS, dim=i2i.DIM, vladv2=False, gating=False)
    m.load_state_dict({k[len("pool."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("pool.")})
    return m.eval()


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = i2i_ref.make_state_dict(i2i_ref.SEED)
    enc, head = i2i_ref.encoder(sd), reference_head(sd)
    rng = np.random.default_rng(7)
    with torch.no_grad():
        x = i2i_ref.binary_image(rng, 2, 96, 80)
        f = enc(torch.from_numpy(x))
        d = head(f)
        np.savez_compressed(os.path.join(HERE, "i2i_small.npz"), seed=np.int64(i2i_ref.SEED), x=x.astype(np.uint8),
                            feat=f.numpy(), desc=d.numpy())
        print("i2i_small", x.shape, "->", tuple(f.shape), float(f.abs().max()), tuple(d.shape))
        x = i2i_ref.binary_image(rng, 1, 768, 768, fill=0.08, inner=(600, 520))
        f = enc(torch.from_numpy(x))
        d = head(f)
        idx = np.sort(rng.choice(f.numel(), 4096, replace=False)).astype(np.int64)
        np.savez_compressed(os.path.join(HERE, "i2i_full.npz"), seed=np.int64(i2i_ref.SEED),
                            bits=np.packbits(x.astype(bool).reshape(-1)), shape=np.array(x.shape, np.int64), idx=idx,
                            feat_sample=f.numpy().reshape(-1)[idx], feat_absmax=np.float32(f.abs().max()),
                            desc=d.numpy())
        print("i2i_full", x.shape, "->", tuple(f.shape), float(f.abs().max()), tuple(d.shape))


if __name__ == "__main__":
    main()
