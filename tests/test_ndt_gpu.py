"""GPU: NDT scan registration (gloc_reg_ndt_*, gloc_scan_store_add_approx_voxel) against the float64 restatement
tests/ndt_ref.py -- the source filter bit for bit, the target cells, the derivatives, whole alignments, batching and
determinism, degenerate inputs, and the global_registration command line with GLOC_REFINE=ndt."""
import os
import re
import subprocess

import numpy as np
import pytest

import ndt_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref_params(capi, prm=None):
    p = prm or capi.default_ndt_params()
    return {f: getattr(p, f) for f, _ in p._fields_}      # the float32 values the device sees


def _pose_err(A, B):
    E = np.linalg.inv(np.asarray(A, np.float64)) @ np.asarray(B, np.float64)
    return np.linalg.norm(E[:3, 3]), np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1))


@pytest.fixture(scope="module")
def env(capi):
    from gloc3d_amd import synth
    world = synth.make_world(1001, n_boxes=400, extent=50.0)
    truth = [synth.se3(2.0, (0.2, 0.0, 0.0)), synth.se3(-1.5, (0.1, 0.15, 0.02)), synth.se3(1.0, (-0.15, 0.1, 0.0), roll_deg=-0.5)]
    store = capi.ScanStore()
    ids = store.add_raycast(world, [np.eye(4)] + truth, np.array([5, 6, 7, 8], np.uint64), n_az=500)
    reg = capi.Registrar(store=store)
    tgt, srcs = ids[0], ids[1:]
    filt = {s: store.add_approx_voxel(s, 0.2) for s in srcs}
    tgt_pts = store.download(tgt)
    cells = R.build_cells(tgt_pts, 0.5)
    yield dict(store=store, reg=reg, tgt=tgt, srcs=srcs, truth=truth, filt=filt, cells=cells, world=world)
    reg.close()
    store.close()


def test_filter_equals_the_restatement_bit_for_bit(capi, env):
    st = env["store"]
    for s in env["srcs"]:
        dev = st.download(env["filt"][s])
        ref = R.approx_voxel(st.download(s), 0.2)
        assert len(dev) == len(ref) > 1000
        assert (R.sort_rows_by_bits(dev).view(np.uint32) == R.sort_rows_by_bits(ref).view(np.uint32)).all()
    rng = np.random.default_rng(7)
    base = st.download(env["srcs"][0])[:5000]
    nanc = base.copy()
    nanc[::5, 2] = np.nan
    nanc[::13, 0] = np.inf
    cases = [base - np.float32(37.3), nanc, np.array([[-1.25, 3.5, 0.75]], np.float32),
             (np.float32(0.41) + rng.random((300, 3)).astype(np.float32) * np.float32(0.15)),
             rng.uniform(-30, 30, (20000, 3)).astype(np.float32)]
    for c in cases:
        sid = st.add(c)
        fid = st.add_approx_voxel(sid, 0.2)
        dev = st.download(fid)
        ref = R.approx_voxel(c, 0.2)
        assert len(dev) == len(ref)
        assert (R.sort_rows_by_bits(dev).view(np.uint32) == R.sort_rows_by_bits(ref).view(np.uint32)).all()
        st.release(fid)
        st.release(sid)
    assert len(R.approx_voxel(cases[3], 0.2)) == 1 and len(R.approx_voxel(cases[4], 0.2)) > 16000


def test_cells_match_the_restatement(capi, env):
    st, reg = env["store"], env["reg"]
    from gloc3d_amd import synth
    far = st.add_variant(env["tgt"], synth.se3(0.0, (80.0, -35.0, 4.0)))     # fp32 coordinates near 80 m
    for sid in (env["tgt"], far):
        dev = reg.ndt_cells(sid)
        ref = R.build_cells(st.download(sid), 0.5)
        assert len(dev["count"]) == len(ref["count"]) > 500
        assert (dev["key3"] == ref["key3"]).all() and (dev["count"] == ref["count"]).all()
        assert np.abs(dev["mean"] - ref["mean"]).max() <= 1e-6 * np.abs(ref["mean"]).max()
        nrm = np.linalg.norm(ref["icov"].reshape(-1, 9), axis=1)
        assert (np.abs(dev["icov"] - ref["icov"]).reshape(-1, 9).max(1) <= 1e-4 * nrm).all()
    st.release(far)


def test_derivatives_match_the_restatement(capi, env):
    st, reg = env["store"], env["reg"]
    s = env["srcs"][0]
    x = st.download(env["filt"][s])
    for p in ([0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.15, -0.02, 0.01, 0.003, -0.002, 0.03],
              [0.2, 0.01, 0.0, 0.0, 0.0, 0.0349]):
        sd, gd, Hd = reg.ndt_derivatives(s, env["tgt"], p)
        sr, gr, Hr = R.derivatives(x, env["cells"], np.array(p))
        assert abs(sd - sr) <= 1e-5 * abs(sr) and sr > 0
        assert np.abs(gd - gr).max() <= 1e-4 * np.linalg.norm(gr)
        assert np.abs(Hd - Hr).max() <= 1e-4 * np.linalg.norm(Hr)


def test_alignment_recovers_the_pose_and_follows_the_restatement(capi, env):
    from gloc3d_amd import synth
    st, reg = env["store"], env["reg"]
    rp = _ref_params(capi)
    guesses = [np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32),
               synth.se3(0.0, (0.0, 0.0, 0.0), roll_deg=-0.3).astype(np.float32)]   # negative roll: p starts at rx ~ pi
    for s, truth, g in zip(env["srcs"], env["truth"], guesses):
        T, prob, iters, conv = reg.ndt_batch(s, [env["tgt"]], init_T=g[None])
        dt, da = _pose_err(truth, T[0])
        assert dt < 0.02 and np.degrees(da) < 0.1, (dt, np.degrees(da))
        assert conv[0] and 1 <= iters[0] <= 35 and prob[0] > 0
        r = R.align(st.download(env["filt"][s]), env["cells"], init_T=g, params=rp)
        dt, da = _pose_err(r["T"], T[0])
        assert dt < 1e-3 and da < 1e-3
        assert abs(int(iters[0]) - r["iters"]) <= 1
        assert abs(prob[0] - r["prob"]) <= 1e-3 * abs(r["prob"])


def test_a_batch_equals_single_calls_and_repeats_bit_for_bit(capi, env):
    from gloc3d_amd import synth
    st, reg = env["store"], env["reg"]
    s = env["srcs"][0]
    tg = [env["tgt"], env["srcs"][1], env["srcs"][2], env["tgt"]] * 5
    init = np.stack([synth.se3(0.2 * (i % 7), (0.02 * (i % 5), -0.01 * (i % 3), 0.0)) for i in range(20)]).astype(np.float32)
    T, prob, iters, conv = reg.ndt_batch(s, tg, init_T=init)
    T2, prob2, iters2, conv2 = reg.ndt_batch(s, tg, init_T=init)
    assert (T.view(np.uint32) == T2.view(np.uint32)).all() and (prob.view(np.uint64) == prob2.view(np.uint64)).all()
    assert (iters == iters2).all() and (conv == conv2).all()
    for c in range(20):
        t1, p1, i1, c1 = reg.ndt_batch(s, [tg[c]], init_T=init[c:c + 1])
        assert (t1[0].view(np.uint32) == T[c].view(np.uint32)).all()
        assert p1[0] == prob[c] and i1[0] == iters[c] and c1[0] == conv[c]


def test_degenerate_cases(capi, env):
    from gloc3d_amd import synth
    st, reg = env["store"], env["reg"]
    s = env["srcs"][0]
    far = st.add_variant(env["tgt"], synth.se3(0.0, (1000.0, 0.0, 0.0)))    # no cell in reach of the source
    g = synth.se3(1.0, (0.1, 0.0, 0.0)).astype(np.float32)
    T, prob, iters, conv = reg.ndt_batch(s, [far], init_T=g[None])
    assert np.abs(T[0] - g).max() < 1e-6 and iters[0] == 0 and prob[0] == 0.0
    # released and recycled ids: the result is the fresh one, equal to a new handle's on a new store
    st.release(far)
    other = st.add_variant(env["srcs"][1], None)
    assert other == far                                            # (the id came back)
    T, prob, iters, conv = reg.ndt_batch(s, [other])
    st2 = capi.ScanStore()
    reg2 = capi.Registrar(store=st2)
    a = st2.add(st.download(s))
    b = st2.add(st.download(other))
    T2, prob2, iters2, conv2 = reg2.ndt_batch(a, [b])
    assert (T.view(np.uint32) == T2.view(np.uint32)).all() and prob[0] == prob2[0] and iters[0] == iters2[0]
    reg2.close()
    st2.close()
    st.release(other)
    # invalid arguments
    for bad in (dict(resolution=0.0), dict(max_iters=0)):
        with pytest.raises(capi.GlocError) as e:
            reg.ndt_batch(s, [env["tgt"]], params=capi.default_ndt_params(**bad))
        assert e.value.code == 1
    with pytest.raises(capi.GlocError) as e:
        reg.ndt_batch(s, [123456])
    assert e.value.code == 1
    empty = st.add(np.full((10, 3), np.nan, np.float32))
    with pytest.raises(capi.GlocError) as e:
        reg.ndt_batch(empty, [env["tgt"]])
    assert e.value.code == 1
    with pytest.raises(capi.GlocError) as e:
        st.add_approx_voxel(123456)
    assert e.value.code == 1
    st.release(empty)


def test_command_line_refines_with_ndt(tmp_path):
    from gloc3d_amd import build as b, gloc_io, synth
    b.build_cli()
    w = synth.make_world(1001, n_boxes=400, extent=50.0)
    poses, files = [], []
    for i in range(6):
        T = synth.se3(0.5 * i, (0.6 * i, 0.1 * i, 0.0))
        f = str(tmp_path / f"db_{i:06d}.bin")
        synth.write_kitti_bin(f, synth.lidar_scan(w, T, seed=100 + i, n_az=360))
        poses.append(T)
        files.append(f)
    qfiles, qposes, positives = [], [], []
    for qi, j in enumerate((1, 3, 4)):
        T = synth.se3(0.5 * j + 1.0, (0.6 * j + 0.25, 0.1 * j - 0.2, 0.03))   # as test_pipeline_gpu's drive
        f = str(tmp_path / f"q_{qi:06d}.bin")
        synth.write_kitti_bin(f, synth.lidar_scan(w, T, seed=900 + qi, n_az=360))
        qfiles.append(f)
        qposes.append(T)
        positives.append([j - 1, j, j + 1])
    gloc_io.write_valset(tmp_path / "valset.txt", files, qfiles, positives)
    gloc_io.write_poses(tmp_path / "poses.txt", poses + qposes)
    exe = os.path.join(ROOT, "gloc3d_amd", "bin", "global_registration")
    p = subprocess.run([exe, str(tmp_path / "valset.txt"), str(tmp_path / "poses.txt")], cwd=tmp_path, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, GLOC_REFINE="ndt"))
    assert p.returncode == 0, p.stdout + p.stderr
    errs = re.findall(r"err_pos, err_rot: ([\d.eE+-]+), ([\d.eE+-]+)", p.stdout)
    assert len(errs) == 9
    assert re.search(r"^\d+, 9$", p.stdout, re.M)
    assert float(re.search(r"Success rate: ([\d.eE+-]+)", p.stdout).group(1)) > 0.9
    assert re.search(r"Rot error: ", p.stdout) and re.search(r"Pos error: ", p.stdout)
