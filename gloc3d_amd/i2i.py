"""The reference's i2i place descriptor (VGG16 features[:-2] + NetVLAD-FC, s2s_libtorch/gen_libtorch_i2i.py:36-60,
main.py:531-541,594) on the device: scans -> HIP BEV (GLOC_BEV_F32_CHW) -> HIP VGG16 encoder (capi.VggEncoder) ->
HIP NetVLAD-FC (capi.NetVladFC), batched, on device buffers throughout.  torch is imported here only (device buffers,
streams, TorchScript loading), never by `import gloc3d_amd`.
"""
import numpy as np
import torch
import torch.nn as nn

from . import capi

# indices of the 13 convolutions in VGG16's `features` (torchvision's layer list), which the reference's checkpoint
# keeps as `encoder.<i>.weight / .bias`
ENCODER_CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
_VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
DIM, CLUSTERS, OUT_DIM = 512, 64, 512  # the i2i head: NetVLAD(num_clusters=64, dim=512, vladv2=False, gating=False)


def vgg16_encoder():
    """VGG16 `features[:-2]` restated in torch (torchvision is not needed): Conv2d(3x3, padding 1) + ReLU, MaxPool2d(2, 2),
    the final ReLU and pool removed -- the same module indices, so a reference state_dict loads into it."""
    layers, cin = [], 3
    for v in _VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers[:-2])


def _numpy_state(state_dict):
    if "state_dict" in state_dict and isinstance(state_dict["state_dict"], dict):
        state_dict = state_dict["state_dict"]
    out = {}
    for k, v in state_dict.items():
        k = k[len("module."):] if k.startswith("module.") else k
        out[k] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    return out


def i2i_weights(state_dict):
    """The reference checkpoint layout (`encoder.{0,2,...,28}.weight / .bias`, `pool.conv.weight`, `pool.centroids`,
    `pool.hidden1_weights`; bare or under "state_dict") -> dict(encoder=[13 x (w [Cout, Cin, 3, 3], b [Cout])],
    conv_w [64, 512], conv_b None, centroids [64, 512], fc_w [32768, 512]), float32."""
    sd = _numpy_state(state_dict)
    enc = []
    for li, i in enumerate(ENCODER_CONV_IDX):
        ci, co, _, _ = _shape(li)
        w = np.ascontiguousarray(sd[f"encoder.{i}.weight"], np.float32)
        b = np.ascontiguousarray(sd[f"encoder.{i}.bias"], np.float32)
        if w.shape != (co, ci, 3, 3) or b.shape != (co,):
            raise ValueError(f"encoder.{i}: expected [{co}, {ci}, 3, 3] + [{co}], got {w.shape} + {b.shape}")
        enc.append((w, b))
    conv_w = np.ascontiguousarray(sd["pool.conv.weight"], np.float32).reshape(CLUSTERS, DIM)
    conv_b = sd.get("pool.conv.bias")
    return dict(encoder=enc, conv_w=conv_w, conv_b=None if conv_b is None else np.ascontiguousarray(conv_b, np.float32),
                centroids=np.ascontiguousarray(sd["pool.centroids"], np.float32).reshape(CLUSTERS, DIM),
                fc_w=np.ascontiguousarray(sd["pool.hidden1_weights"], np.float32).reshape(CLUSTERS * DIM, OUT_DIM))


def _shape(layer):
    """(Cin, Cout, relu, pool) without loading the library."""
    convs = [v for v in _VGG16_CFG if v != "M"]
    ci = 3 if layer == 0 else convs[layer - 1]
    return ci, convs[layer], layer < 12, layer in (1, 3, 6, 9)


class I2iVladDescriptor:
    """Scans -> 512-D descriptors of the reference's i2i model.  `device` is a torch device index; a scan is [n, 3+]
    float32 (x y z ...).  Images are `width` x `height` (768 x 768 in the reference, loop_detector.cpp:142-143)."""

    def __init__(self, weights, device=0, width=768, height=768, bev_params=None):
        if width % 16 or height % 16:
            raise ValueError("the encoder needs width and height that are multiples of 16")
        self.device = device
        self.tdev = torch.device("cuda", device)
        self.width, self.height = width, height
        self.bev_params = bev_params or capi.default_bev_params(out_width=width, out_height=height,
                                                                 format=capi.BEV_F32_CHW)
        self.bev = capi.BevProjector(device)
        self.encoder = capi.VggEncoder(device)
        self.encoder.set_layers(weights["encoder"])
        self.pool = capi.NetVladFC(weights["conv_w"], weights["centroids"], weights["fc_w"], conv_b=weights["conv_b"],
                                   normalize_input=True, device=device)
        self.out_dim = self.pool.out_dim
        # a stream of our own: torch's default stream has handle 0, which the C ABI reads as "the handle's own stream"
        self.stream = torch.cuda.Stream(self.tdev)
        self.bev.set_stream(self.stream.cuda_stream)
        self.encoder.set_stream(self.stream.cuda_stream)
        self.pool.set_stream(self.stream.cuda_stream)

    @classmethod
    def from_state_dict(cls, state_dict, **kw):
        """A checkpoint of the reference's VGGVLAD (`encoder.*` + `pool.*`, or {"state_dict": ...})."""
        return cls(i2i_weights(state_dict), **kw)

    @classmethod
    def from_torchscript(cls, path, **kw):
        """The module the reference's C++ loads (i2i_vgg_vlad.pt, traced by gen_libtorch_i2i.py)."""
        return cls(i2i_weights(torch.jit.load(path, map_location="cpu").state_dict()), **kw)

    def close(self):
        self.bev.close()
        self.encoder.close()
        self.pool.close()

    def _images(self, scans, want_info=False):
        """[B, 3, H, W] torch tensor of BEV images on the device (issued on self.stream), and the infos."""
        scans = scans if isinstance(scans, (list, tuple)) else [scans]
        scans = [np.asarray(s, np.float32) for s in scans]
        host, off = capi._scan_batch([np.pad(s, ((0, 0), (0, 1))) if s.shape[1] == 3 else s for s in scans])
        pts = torch.from_numpy(host).to(self.tdev, non_blocking=False)
        imgs = torch.empty((len(off) - 1, 3, self.height, self.width), dtype=torch.float32, device=self.tdev)
        infos = self.bev.project_batch_device(pts.data_ptr(), off, host.shape[1], imgs.data_ptr(), self.bev_params,
                                              want_info=want_info)
        pts.record_stream(self.stream)
        return imgs, infos

    def _describe(self, imgs):
        n = imgs.shape[0]
        feat = torch.empty((n, DIM, self.height // 16, self.width // 16), dtype=torch.float32, device=self.tdev)
        self.encoder.forward_device(imgs.data_ptr(), n, self.height, self.width, feat.data_ptr())
        out = torch.empty((n, self.out_dim), dtype=torch.float32, device=self.tdev)
        self.pool.forward_device(feat.data_ptr(), n, feat.shape[2] * feat.shape[3], out.data_ptr())
        return feat, out

    @torch.no_grad()
    def images(self, scans):
        """The encoder's input, [B, 3, H, W] torch tensor on the device (the caller's stream waits for it)."""
        caller = torch.cuda.current_stream(self.tdev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            imgs, _ = self._images(scans)
        caller.wait_stream(self.stream)
        imgs.record_stream(caller)  # made on self.stream, used and freed on the caller's
        return imgs

    @torch.no_grad()
    def describe_images(self, imgs):
        """Encoder + head on [B, 3, H, W] device images: (feature map [B, 512, H/16, W/16], descriptors [B, 512]),
        torch tensors on the device."""
        imgs = imgs.to(self.tdev, torch.float32).contiguous()
        caller = torch.cuda.current_stream(self.tdev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            feat, out = self._describe(imgs)
            imgs.record_stream(self.stream)
        caller.wait_stream(self.stream)
        feat.record_stream(caller)  # made on self.stream, used and freed on the caller's
        out.record_stream(caller)
        return feat, out

    @torch.no_grad()
    def __call__(self, scans):
        """A scan [n, 3+] or a list of them -> descriptors [B, 512] (numpy)."""
        caller = torch.cuda.current_stream(self.tdev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            imgs, _ = self._images(scans)
            _, out = self._describe(imgs)
            res = out.cpu().numpy()
        return res

    @torch.no_grad()
    def place_feature(self, scan):
        """RpyPCLoopDetector::get_place_feature (registration/loop_detector.cpp:137-172) for one scan:
        (descriptor [512], occupancy_grid [height, width] u8, xy_res = (ox, oy, resolution))."""
        caller = torch.cuda.current_stream(self.tdev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            imgs, infos = self._images([scan], want_info=True)
            if infos[0]["empty"]:
                raise ValueError("no point of the scan lies within range")  # the reference aborts in cv::Mat
            _, out = self._describe(imgs)
            desc = out.cpu().numpy()[0]
        info = infos[0]
        return desc, self.bev.raw_image(info, 0), (info["ox"], info["oy"], info["resolution"])
