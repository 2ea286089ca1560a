"""PointPillar-NetVLAD scan descriptor (the reference's PointPillarVLAD, model/s2s_merged.py:113-255, as traced by
s2s_libtorch/gen_libtorch_pointpillar.py): the HIP canvas (capi.PillarEncoder), the PointPillarTest backbone -- this
project's restatement in torch (PillarBackbone, the default) or the library's HIP one (backbone="hip") -- and the HIP
NetVLAD-FC head (capi.NetVladFC).  torch is imported here only, never by `import gloc3d_amd`.
"""
import numpy as np
import torch
import torch.nn as nn

from . import capi


def _conv_bn_relu(cin, cout, stride=1, relu=True):
    layers = [nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False), nn.BatchNorm2d(cout)]
    if relu:
        layers.append(nn.ReLU(inplace=True))
    return layers


class _Block(nn.Module):
    """PillarBlock (s2s_merged.py:90-111): num_layers x (3x3 conv, BN, ReLU), the first with the stride; parameters
    under `layers.*` as in the reference."""

    def __init__(self, cin, cout, num_layers, stride):
        super().__init__()
        layers = []
        for i in range(num_layers):
            layers += _conv_bn_relu(cin if i == 0 else cout, cout, stride if i == 0 else 1)
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        return self.layers(x)


class PillarBackbone(nn.Module):
    """PointPillarTest after the scatter-mean (s2s_merged.py:152-188,219-247, vlad_mode): canvas [B, 64, gx * gy] ->
    .view(B, 64, gx, gy) -> block1-3, up1-3, concat, conv_out -> .transpose(3, 2): [B, 128, gy, gx]."""

    def __init__(self, gx, gy):
        super().__init__()
        self.gx, self.gy = gx, gy
        self.block1 = _Block(64, 64, 2, 1)
        self.block2 = _Block(64, 128, 3, 2)
        self.block3 = _Block(128, 256, 3, 2)
        self.up1 = nn.Sequential(*_conv_bn_relu(64, 64))
        self.up2 = nn.Sequential(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True), *_conv_bn_relu(128, 128))
        self.up3 = nn.Sequential(nn.Upsample(scale_factor=4, mode="bilinear", align_corners=True), *_conv_bn_relu(256, 256))
        self.conv_out = nn.Sequential(*_conv_bn_relu(448, 256), *_conv_bn_relu(256, 128, relu=False))

    def forward(self, canvas):
        x = canvas.view(canvas.shape[0], -1, self.gx, self.gy)   # the x-major index makes this (x, y) (Q3)
        f1 = self.block1(x)
        f2 = self.block2(f1)
        f3 = self.block3(f2)
        x = torch.cat([self.up1(f1), self.up2(f2), self.up3(f3)], dim=1)
        return self.conv_out(x).transpose(3, 2)


# (conv, BatchNorm) of the backbone's 13 layers in the order of gloc_pillar_backbone_layer_shape, as PillarBackbone
# (and the reference's PointPillarTest) names them in a state_dict
BACKBONE_KEYS = [("block1.layers.0", "block1.layers.1"), ("block1.layers.3", "block1.layers.4"),
                 ("block2.layers.0", "block2.layers.1"), ("block2.layers.3", "block2.layers.4"),
                 ("block2.layers.6", "block2.layers.7"),
                 ("block3.layers.0", "block3.layers.1"), ("block3.layers.3", "block3.layers.4"),
                 ("block3.layers.6", "block3.layers.7"),
                 ("up1.0", "up1.1"), ("up2.1", "up2.2"), ("up3.1", "up3.2"),
                 ("conv_out.0", "conv_out.1"), ("conv_out.3", "conv_out.4")]


def backbone_layers(sd, prefix="encoder."):
    """13 tuples (w, bn_weight, bn_bias, bn_mean, bn_var) from a state_dict of numpy arrays."""
    return [(sd[prefix + c + ".weight"], sd[prefix + b + ".weight"], sd[prefix + b + ".bias"],
             sd[prefix + b + ".running_mean"], sd[prefix + b + ".running_var"]) for c, b in BACKBONE_KEYS]


class PillarVladDescriptor:
    """Scans -> 128-D descriptors of PointPillarVLAD (encoder = PointPillarTest in vlad_mode, pool = NetVLAD 64 x 128 ->
    128).  `device` is a torch device index; scans may be numpy arrays (host) or a torch tensor on that device.
    backbone="torch" runs PillarBackbone (torch convolutions); "hip" runs the library's backbone, the canvas, backbone
    and head on one stream with no torch convolution in the path (loaded from the same `encoder.*` keys)."""

    def __init__(self, state_dict, params=None, device=0, pn_eps=1e-5, backbone="torch", bn_eps=1e-5):
        if backbone not in ("torch", "hip"):
            raise ValueError(f"backbone must be 'torch' or 'hip', not {backbone!r}")
        self.params = params or capi.default_pillar_params()
        gx, gy, gz = self.params.grid()
        if gz != 1:
            raise ValueError("the backbone views the canvas as [64, gx, gy]: zbound must give one cell")
        self.device = device
        self.tdev = torch.device("cuda", device)
        sd = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in state_dict.items()}
        self.encoder = capi.PillarEncoder(device)
        pn = "encoder.pn.pointnet."
        self.encoder.set_pointnet(sd[pn + "0.weight"].reshape(64, 14), sd[pn + "1.weight"], sd[pn + "1.bias"],
                                  sd[pn + "1.running_mean"], sd[pn + "1.running_var"], pn_eps)
        self.grid = (gx, gy)
        if backbone == "hip":
            self.backbone = None
            for layer, args in enumerate(backbone_layers(sd)):
                self.encoder.set_backbone_layer(layer, *args, eps=bn_eps)
        else:
            self.backbone = PillarBackbone(gx, gy)
            enc = {k[len("encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()
                   if k.startswith("encoder.") and not k.startswith(("encoder.pn.", "encoder.conv_out_pose."))}
            self.backbone.load_state_dict(enc)          # strict: every backbone parameter must be in the checkpoint
            self.backbone = self.backbone.to(self.tdev).eval()
        conv_w = sd["pool.conv.weight"].reshape(sd["pool.conv.weight"].shape[0], -1)
        self.pool = capi.NetVladFC(conv_w, sd["pool.centroids"], sd["pool.hidden1_weights"],
                                   conv_b=sd.get("pool.conv.bias"), normalize_input=True, device=device)
        self.out_dim = self.pool.out_dim
        # a stream of our own: torch's default stream has handle 0, which the C ABI reads as "the handle's own stream"
        self.stream = torch.cuda.Stream(self.tdev)
        self.encoder.set_stream(self.stream.cuda_stream)
        capi.lib().gloc_vlad_set_stream(self.pool._h, capi.C.c_void_p(self.stream.cuda_stream))

    @classmethod
    def from_state_dict(cls, state_dict, **kw):
        """A PointPillarVLAD checkpoint's state_dict (or {"state_dict": ...}): `encoder.*` and `pool.*` keys;
        `encoder.conv_out_pose.*` is ignored, as the reference's strict=False load does (gen_libtorch_pointpillar.py:40)."""
        if "state_dict" in state_dict and isinstance(state_dict["state_dict"], dict):
            state_dict = state_dict["state_dict"]
        return cls(state_dict, **kw)

    def close(self):
        self.encoder.close()
        self.pool.close()

    def canvas(self, scans):
        """[B, 64, nv] torch tensor on the device; the caller's current stream waits for it."""
        caller = torch.cuda.current_stream(self.tdev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            out = self._canvas(scans)
        caller.wait_stream(self.stream)
        return out

    def _points(self, scans):
        if torch.is_tensor(scans):
            pts = scans.to(self.tdev, torch.float32).contiguous()
            off = np.array([0, pts.shape[0]], np.uint64)
        else:
            host, off = capi._scan_batch(scans)
            pts = torch.from_numpy(host).to(self.tdev)
        pts.record_stream(self.stream)
        return pts, off, pts.shape[1] if pts.dim() == 2 else 4

    def _canvas(self, scans):
        pts, off, stride = self._points(scans)
        gx, gy, gz = self.params.grid()
        out = torch.empty((len(off) - 1, capi.PILLAR_FEATURES, gx * gy * gz), dtype=torch.float32, device=self.tdev)
        self.encoder.canvas_device(pts.data_ptr(), off, stride, out.data_ptr(), self.params)
        return out

    def _features(self, scans):
        """[B, 128, gy * gx] on the device (on self.stream): the torch or the HIP backbone behind the canvas."""
        if self.backbone is not None:
            feat = self.backbone(self._canvas(scans)).contiguous()     # [B, 128, gy, gx]
            return feat.view(feat.shape[0], feat.shape[1], -1)
        pts, off, stride = self._points(scans)
        gx, gy = self.grid
        feat = torch.empty((len(off) - 1, 128, gx * gy), dtype=torch.float32, device=self.tdev)
        self.encoder.features_device(pts.data_ptr(), off, stride, feat.data_ptr(), self.params)
        return feat

    @torch.no_grad()
    def __call__(self, scans):
        """A scan [n, 4+] or a list of them -> descriptors [B, 128] (numpy)."""
        caller = torch.cuda.current_stream(self.tdev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            feat = self._features(scans)                               # [B, 128, gy * gx]
            out = torch.empty((feat.shape[0], self.out_dim), dtype=torch.float32, device=self.tdev)
            self.pool.forward_device(feat.data_ptr(), feat.shape[0], feat.shape[2], out.data_ptr())
            res = out.cpu().numpy()
        return res
