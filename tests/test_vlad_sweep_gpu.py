"""GPU: the NetVLAD-FC pooling head (gloc_vlad_*) against the float64 reference over the case table of
vlad_cases.py -- every ragged edge of the kernels' tiling, each with a dense and a selection FC, inside the
tolerance test_vlad_cases_cpu.py derives from the reference alone -- and the properties a kernel without atomics
and with fixed summation orders has to keep bit for bit."""
import ctypes as C

import numpy as np
import pytest

import vlad_cases as T

pytestmark = pytest.mark.gpu
ERR_INVALID = 1


def head(capi, a, kind, gated=True):
    m = capi.NetVladFC(a.conv_w, a.centroids, a.fc[kind], conv_b=a.conv_b, normalize_input=a.normalize_input)
    if gated and a.gating is not None:
        m.set_gating(*a.gating)
    return m


def bits(y):
    return np.ascontiguousarray(y, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_case_within_reference_tolerance(capi, case, kind):
    a, b = T.inputs(case), T.bounds(case)[kind]
    m = head(capi, a, kind)
    got = m.forward(a.x)
    m.close()
    assert got.shape == b.ref.shape and np.isfinite(got).all()
    err = float(np.abs(got - b.ref).max())
    print(f"\n{case.name} {kind}: n={case.n} K={case.K} C={case.C} HW={case.H * case.W} out={got.shape[1]} "
          f"err {err:.2e} tol {b.tol:.2e} ({case.branch})")
    if "zero_cent" in case.flags:      # nothing to aggregate and nothing to subtract: zeros, not 0/0
        assert (got[1] == 0.0).all()
    assert err <= b.tol


def small(rng, n, K, C, HW, out, bias=True):
    x = np.maximum(rng.standard_normal((n, C, HW)), 0).astype(np.float32)
    w = (rng.standard_normal((K, C)) * 4.0 / np.sqrt(C)).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32) if bias else None
    c = rng.random((K, C)).astype(np.float32)
    fc = (rng.standard_normal((K * C, out)) / np.sqrt(C)).astype(np.float32)
    return x, w, b, c, fc


def test_same_call_twice_gives_the_same_bits(capi):
    for name in ("HW130_nonorm", "gate_out65"):
        a = T.inputs(T.BY_NAME[name])
        m = head(capi, a, "dense")
        y0, y1 = m.forward(a.x), m.forward(a.x)
        m.close()
        assert same_bits(y0, y1), name


def test_image_in_a_batch_equals_the_image_alone(capi):
    """FC passes of 8: image i of 17 sits in pass i // 8; alone and in a batch of 8 it is row 0 or i % 8 of the only pass."""
    x, w, b, c, fc = small(np.random.default_rng(11), 17, 20, 24, 70, 37)
    m = capi.NetVladFC(w, c, fc, conv_b=b)
    y17 = m.forward(x)
    for i in (0, 7, 8, 16):
        assert same_bits(m.forward(x[i:i + 1])[0], y17[i]), i
        idx = np.roll([(i + j) % 17 for j in range(8)], i % 8)
        assert idx[i % 8] == i
        assert same_bits(m.forward(x[idx])[i % 8], y17[i]), i
    m.close()


def test_gating_switched_off_equals_the_ungated_handle(capi):
    a = T.inputs(T.BY_NAME["gate_out65"])
    plain = head(capi, a, "dense", gated=False)
    y = plain.forward(a.x)
    plain.close()
    m = head(capi, a, "dense")
    yg = m.forward(a.x)
    m.set_gating(None)
    y_off = m.forward(a.x)
    m.close()
    assert same_bits(y_off, y) and not same_bits(yg, y)


def test_workspaces_that_only_grow_keep_no_stale_rows(capi):
    """partV / partS are indexed by the call's tile count and fc_part by its pass: a smaller call after a larger one
    reads only what it wrote."""
    rng = np.random.default_rng(12)
    K, Cc, out = 17, 20, 5
    _, w, b, c, fc = small(rng, 1, K, Cc, 1, out)
    xs = [np.maximum(rng.standard_normal((n, Cc, hw)), 0).astype(np.float32) for n, hw in ((2, 130), (1, 5), (17, 65))]
    xs.append(xs[0])
    m = capi.NetVladFC(w, c, fc, conv_b=b)
    reused = [m.forward(x) for x in xs]
    m.close()
    for x, y in zip(xs, reused):
        fresh = capi.NetVladFC(w, c, fc, conv_b=b)
        assert same_bits(fresh.forward(x), y), x.shape
        fresh.close()


def test_alternating_handles_of_different_width(capi):
    """The dynamic-LDS size is an attribute of the kernel, not of a handle: every call has to set its own."""
    rng = np.random.default_rng(13)
    sets = [small(rng, 2, 33, 300, 70, 6), small(rng, 2, 5, 8, 70, 6)]
    alone = []
    for x, w, b, c, fc in sets:
        m = capi.NetVladFC(w, c, fc, conv_b=b)
        alone.append(m.forward(x))
        m.close()
    ms = [capi.NetVladFC(w, c, fc, conv_b=b) for _, w, b, c, fc in sets]
    for _ in range(2):
        for m, s, y in zip(ms, sets, alone):
            assert same_bits(m.forward(s[0]), y)
    for m in ms:
        m.close()


@pytest.mark.parametrize("name", ["HW65_KC1024", "gate_out65"])
def test_device_path_equals_host_path(capi, name):
    """gloc_vlad_forward_device on torch buffers and a torch stream, as gloc3d_amd/i2i.py calls it."""
    import torch
    case = T.BY_NAME[name]
    a = T.inputs(case)
    m = head(capi, a, "dense")
    y_host = m.forward(a.x)
    tdev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(tdev)
    m.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        feat = torch.from_numpy(a.x.copy()).to(tdev)     # the table's arrays are read-only
        out = torch.empty((case.n, case.out), dtype=torch.float32, device=tdev)
        m.forward_device(feat.data_ptr(), case.n, case.H * case.W, out.data_ptr())
        y_dev = out.cpu().numpy()
    m.close()
    assert same_bits(y_dev, y_host)
    assert np.abs(y_dev - T.bounds(case)["dense"].ref).max() <= T.bounds(case)["dense"].tol


def _create(capi, K, Cc, out):
    """gloc_vlad_create on zero parameters of the stated sizes: (return code, handle, message)."""
    z = np.zeros(max(K * Cc * out, K * Cc, K, 1), np.float32)
    h = C.c_void_p(1)      # a refusal has to null it
    p = z.ctypes.data_as(C.c_void_p)
    rc = capi.lib().gloc_vlad_create(0, Cc, K, out, p, None, p, p, 1, C.byref(h))
    return rc, h, capi.lib().gloc_last_error().decode("utf-8", "replace")


def test_create_refuses_what_cannot_run(capi):
    """Host-side argument checks only: nothing here reaches a kernel.  The largest tiles that do fit, (64, 557) and
    (48, 560), run in the sweep above."""
    for K, Cc, out in ((64, 558, 1), (64, 560, 1), (49, 558, 1), (1, 561, 1), (65, 8, 1), (0, 8, 1), (8, 0, 1), (4, 8, 0),
                       (1, 1, 65537)):
        rc, h, msg = _create(capi, K, Cc, out)
        assert rc == ERR_INVALID and not h.value, (K, Cc, out, rc, msg)
    rc, h, msg = _create(capi, 64, 558, 1)
    assert "558" in msg and "64" in msg    # the LDS refusal names both numbers
    for K, Cc in ((64, 557), (48, 560), (1, 560)):
        rc, h, msg = _create(capi, K, Cc, 1)
        assert rc == 0 and h.value, (K, Cc, msg)
        assert capi.lib().gloc_vlad_destroy(h) == 0


def test_forward_refuses_empty_batches_and_gating_without_scale(capi):
    import torch
    x, w, b, c, fc = small(np.random.default_rng(14), 2, 5, 8, 15, 6)
    rng = np.random.default_rng(15)
    gate = ((rng.standard_normal((6, 6)) / 2).astype(np.float32), rng.standard_normal(6).astype(np.float32),
            rng.standard_normal(6).astype(np.float32))
    m = capi.NetVladFC(w, c, fc, conv_b=b)
    y = m.forward(x)
    L, h = capi.lib(), m._h
    out = np.empty((2, 6), np.float32)
    d = torch.zeros(x.size + out.size, device="cuda")     # real device memory: a missed check would stay inside it
    torch.cuda.synchronize()
    hp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    dp, dop = C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr() + 4 * x.size)
    for n, hw in ((0, 15), (2, 0), (0, 0)):
        assert L.gloc_vlad_forward(h, hp, n, hw, op) == ERR_INVALID
        assert L.gloc_vlad_forward_device(h, dp, n, hw, dop) == ERR_INVALID
    gp = [a.ctypes.data_as(C.c_void_p) for a in gate]
    # weights without scale (or shift): refused, and gating stays off ...
    assert L.gloc_vlad_set_gating(h, gp[0], None, gp[2]) == ERR_INVALID
    assert L.gloc_vlad_set_gating(h, gp[0], gp[1], None) == ERR_INVALID
    assert same_bits(m.forward(x), y)
    # ... or on, with the weights it had
    m.set_gating(*gate)
    yg = m.forward(x)
    assert not same_bits(yg, y)
    assert L.gloc_vlad_set_gating(h, gp[0], None, gp[2]) == ERR_INVALID
    assert same_bits(m.forward(x), yg)
    m.close()
