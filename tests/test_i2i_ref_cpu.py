"""CPU: the i2i restatement (gloc3d_amd.i2i.vgg16_encoder + tests/i2i_ref.netvlad) against the goldens made with the
reference's NetVLAD, the checkpoint key mapping (state_dict, wrapped, TorchScript), and the GLOCI2IW exporter."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import i2i_ref as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def sd():
    return R.make_state_dict(R.SEED)


def test_seeded_weights_are_stable(sd):
    """The goldens depend on these numbers: PCG64 draws, He scale."""
    w0 = sd["encoder.0.weight"]
    assert w0.shape == (64, 3, 3, 3) and w0.dtype == np.float32
    assert abs(float(w0.std()) - np.sqrt(2 / 27)) < 0.02
    assert sd["pool.hidden1_weights"].shape == (64 * 512, 512)
    assert np.array_equal(R.make_state_dict(R.SEED)["encoder.28.bias"], sd["encoder.28.bias"])


def test_restatement_equals_small_golden(sd):
    g = np.load(os.path.join(GOLDEN, "i2i_small.npz"))
    assert int(g["seed"]) == R.SEED
    with torch.no_grad():
        f = R.encoder(sd)(torch.from_numpy(g["x"].astype(np.float32)))
        d = R.netvlad(f, sd)
    f, d = f.numpy(), d.numpy()
    assert f.shape == (2, 512, 6, 5)
    assert np.abs(f - g["feat"]).max() <= 1e-5 * np.abs(g["feat"]).max()
    assert np.abs(d - g["desc"]).max() <= 1e-5 * np.abs(g["desc"]).max()


def test_restatement_equals_full_size_golden(sd):
    g = np.load(os.path.join(GOLDEN, "i2i_full.npz"))
    shape = tuple(int(v) for v in g["shape"])
    assert shape == (1, 3, 768, 768)
    x = np.unpackbits(g["bits"])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
    assert (x[0, 0, 0] == 1).all() and (x[0, 1:, 0] == 0).all()   # the (1, 0, 0) padding
    with torch.no_grad():
        f = R.encoder(sd)(torch.from_numpy(x))
        d = R.netvlad(f, sd)
    f = f.numpy()
    assert f.shape == (1, 512, 48, 48)
    assert np.abs(f.reshape(-1)[g["idx"]] - g["feat_sample"]).max() <= 1e-5 * g["feat_absmax"]
    assert np.abs(d.numpy() - g["desc"]).max() <= 1e-5 * np.abs(g["desc"]).max()


def _check_weights(w, sd):
    from gloc3d_amd import i2i
    assert len(w["encoder"]) == 13
    for li, i in enumerate(i2i.ENCODER_CONV_IDX):
        assert np.array_equal(w["encoder"][li][0], sd[f"encoder.{i}.weight"])
        assert np.array_equal(w["encoder"][li][1], sd[f"encoder.{i}.bias"])
    assert np.array_equal(w["conv_w"], sd["pool.conv.weight"].reshape(64, 512)) and w["conv_b"] is None
    assert np.array_equal(w["centroids"], sd["pool.centroids"])
    assert np.array_equal(w["fc_w"], sd["pool.hidden1_weights"])


def test_key_mapping_state_dict_and_wrapped(sd):
    from gloc3d_amd import i2i
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    _check_weights(i2i.i2i_weights(tsd), sd)
    _check_weights(i2i.i2i_weights({"state_dict": tsd, "epoch": 3}), sd)
    bad = dict(tsd)
    bad["encoder.2.weight"] = torch.zeros(64, 64, 1, 1)
    with pytest.raises(ValueError):
        i2i.i2i_weights(bad)
    missing = {k: v for k, v in tsd.items() if k != "encoder.28.bias"}
    with pytest.raises(KeyError):
        i2i.i2i_weights(missing)


class _Head(torch.nn.Module):
    """The parameters of the reference's NetVLAD (netvlad_fc.py:34-40); forward only has to trace."""

    def __init__(self, sd):
        super().__init__()
        self.conv = torch.nn.Conv2d(512, 64, 1, bias=False)
        self.centroids = torch.nn.Parameter(torch.from_numpy(sd["pool.centroids"]))
        self.hidden1_weights = torch.nn.Parameter(torch.from_numpy(sd["pool.hidden1_weights"]))
        with torch.no_grad():
            self.conv.weight.copy_(torch.from_numpy(sd["pool.conv.weight"]))

    def forward(self, x):
        return R.netvlad(x, {"pool.conv.weight": self.conv.weight, "pool.centroids": self.centroids,
                             "pool.hidden1_weights": self.hidden1_weights})


class _VggVlad(torch.nn.Module):
    """VGGVLAD of gen_libtorch_i2i.py:21-32: encoder + pool."""

    def __init__(self, sd):
        super().__init__()
        self.encoder = R.encoder(sd)
        self.pool = _Head(sd)

    def forward(self, x):
        return self.pool(self.encoder(x))


@pytest.fixture(scope="module")
def traced(sd, tmp_path_factory):
    m = _VggVlad(sd).eval()
    path = str(tmp_path_factory.mktemp("ts") / "i2i_vgg_vlad.pt")
    with torch.no_grad():
        torch.jit.trace(m, torch.ones(1, 3, 32, 32)).save(path)
    return path


def test_key_mapping_torchscript(sd, traced):
    from gloc3d_amd import i2i
    _check_weights(i2i.i2i_weights(torch.jit.load(traced, map_location="cpu").state_dict()), sd)


def test_exporter_round_trips(sd, traced, tmp_path):
    import export_i2i_weights as X
    out = tmp_path / "i2i.bin"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "export_i2i_weights.py"), traced, str(out)],
                          cwd=ROOT)
    with open(out, "rb") as f:
        assert f.read(8) == b"GLOCI2IW"
    _check_weights(X.read(str(out)), sd)
    ckpt = tmp_path / "model_best.pth.tar"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "epoch": 1}, ckpt)
    out2 = tmp_path / "i2i_ckpt.bin"
    X.write(str(out2), X.load_model(str(ckpt)))
    assert out.read_bytes() == out2.read_bytes()
