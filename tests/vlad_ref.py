"""float64 reference of the NetVLAD-FC pooling head, its float32 restatement in the kernels' summation order,
and the mutants the case table (vlad_cases.py) has to tell apart -- TEST INFRASTRUCTURE ONLY, numpy, no GPU.

The operation is NetVLAD.forward and GatingContext.forward of the reference (model/netvlad_fc.py:73-109,136-146)
exactly as oracle/vlad_oracle.py states it in float32:

    x^ = x / max(||x||_2 over channels, 1e-12)                (only with normalize_input)
    soft = softmax over clusters of (conv_w x^ + conv_b)
    vlad[k, c] = sum_p soft[k, p] x^[c, p] - centroid[k, c] sum_p soft[k, p]
    vlad[k, :] /= max(||vlad[k, :]||, 1e-12);  flatten;  v = vlad / max(||vlad||, 1e-12)
    y = v @ fc_w;   gated: y * sigmoid((y @ gating_w) * scale + shift)

Both halves are exposed (vlad64 -> head64) so that a test evaluates the expensive first half once and applies
several FC matrices to it; forward64 is their composition.
"""
import numpy as np

TILE = 64      # positions per tile of vlad_tile_kernel
SLAB = 512     # FC rows per slab of vlad_fc_kernel

# the mutants: one defect each that a kernel of this shape can have
M_LAST_CHANNEL, M_LAST_POSITION, M_LAST_CLUSTER, M_NO_BIAS, M_PADDED_WEIGHT = 1, 2, 3, 4, 5
M_LAST_FC_ROW, M_LAST_IMAGE, M_LAST_COLUMN, M_GATE_SHIFT = 6, 7, 8, 9
MUTANTS = {
    M_LAST_CHANNEL: "last channel left out of the norm, the logits and the aggregation",
    M_LAST_POSITION: "last position given no weight",
    M_LAST_CLUSTER: "last cluster left out of the softmax",
    M_NO_BIAS: "bias not added",
    M_PADDED_WEIGHT: "padded positions of the last tile keep their softmax weight",
    M_LAST_FC_ROW: "last row of the VLAD vector left out of the FC",
    M_LAST_IMAGE: "last image computed from the first image's features",
    M_LAST_COLUMN: "last FC output column zero",
    M_GATE_SHIFT: "gate applied with shift ignored",
}


def vlad64(x, conv_w, conv_b, centroids, normalize_input=True, mutant=0):
    """The normalised VLAD vector [N, K*C] in float64 (everything before the FC)."""
    x = np.asarray(x, np.float64)
    N, C = x.shape[:2]
    x = x.reshape(N, C, -1).copy()
    P = x.shape[2]
    w = np.asarray(conv_w, np.float64)
    cen = np.asarray(centroids, np.float64)
    K = w.shape[0]
    if mutant == M_LAST_IMAGE:
        x[-1] = x[0]
    if mutant == M_LAST_CHANNEL:
        x[:, -1, :] = 0.0
    if normalize_input:
        nrm = np.sqrt((x * x).sum(axis=1, keepdims=True))
        x = x / np.maximum(nrm, 1e-12)
    logits = np.einsum("kc,ncp->nkp", w, x)
    bias = np.zeros(K) if conv_b is None or mutant == M_NO_BIAS else np.asarray(conv_b, np.float64)
    logits = logits + bias[None, :, None]
    if mutant == M_LAST_CLUSTER:
        logits[:, -1, :] = -np.inf
    logits = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(logits)
    soft = e / e.sum(axis=1, keepdims=True)
    if mutant == M_LAST_POSITION:
        soft[:, :, -1] = 0.0
    S = soft.sum(axis=2)
    if mutant == M_PADDED_WEIGHT:
        pad = (-P) % TILE
        eb = np.exp(bias - bias.max())
        S = S + pad * (eb / eb.sum())[None, :]
    vlad = np.einsum("nkp,ncp->nkc", soft, x) - cen[None] * S[:, :, None]
    n1 = np.sqrt((vlad * vlad).sum(axis=2, keepdims=True))
    vlad = vlad / np.maximum(n1, 1e-12)
    vlad = vlad.reshape(N, K * C)
    n2 = np.sqrt((vlad * vlad).sum(axis=1, keepdims=True))
    return vlad / np.maximum(n2, 1e-12)


def gate64(y, gating, mutant=0):
    gw, scale, shift = (np.asarray(a, np.float64) for a in gating)
    g = (y @ gw) * scale + (0.0 if mutant == M_GATE_SHIFT else shift)
    with np.errstate(over="ignore"):
        return y * (1.0 / (1.0 + np.exp(-g)))


def head64(v, fc_w, gating=None, mutant=0, rows=None):
    """FC and optional gate on the vector of vlad64.  `rows` states that fc_w is selection_fc(K, C, rows): the product
    is then v[:, rows] exactly (one 1 per column), taken without forming the float64 matrix."""
    v = np.asarray(v, np.float64)
    if mutant == M_LAST_FC_ROW:
        v = v.copy()
        v[:, -1] = 0.0
    y = v[:, np.asarray(rows)] if rows is not None else v @ np.asarray(fc_w, np.float64)
    if mutant == M_LAST_COLUMN:
        y = y.copy()
        y[:, -1] = 0.0
    return y if gating is None else gate64(y, gating, mutant)


def forward64(x, conv_w, conv_b, centroids, fc_w, normalize_input=True, gating=None, mutant=0):
    """x [N, C, H, W] or [N, C, P] -> [N, out] float64; mutant = 0 is the operation itself."""
    return head64(vlad64(x, conv_w, conv_b, centroids, normalize_input, mutant), fc_w, gating, mutant)


def vlad32_ordered(x, conv_w, conv_b, centroids, normalize_input=True):
    """vlad64 in float32 with the position sums taken per tile of 64 and the tile partials added in tile order."""
    f = np.float32
    x = np.asarray(x, f)
    N, C = x.shape[:2]
    x = x.reshape(N, C, -1)
    P = x.shape[2]
    w = np.asarray(conv_w, f)
    cen = np.asarray(centroids, f)
    K = w.shape[0]
    V = np.zeros((N, K, C), f)
    S = np.zeros((N, K), f)
    for p0 in range(0, P, TILE):
        xt = x[:, :, p0:p0 + TILE]
        if normalize_input:
            nrm = np.sqrt((xt * xt).sum(axis=1, keepdims=True, dtype=f))
            xt = xt * (f(1) / np.maximum(nrm, f(1e-12)))
        lg = np.einsum("kc,ncp->nkp", w, xt).astype(f)
        if conv_b is not None:
            lg = lg + np.asarray(conv_b, f)[None, :, None]
        e = np.exp(lg - lg.max(axis=1, keepdims=True), dtype=f)
        soft = e * (f(1) / e.sum(axis=1, keepdims=True, dtype=f))
        V = V + np.einsum("nkp,ncp->nkc", soft, xt).astype(f)
        S = S + soft.sum(axis=2, dtype=f)
    vlad = V - cen[None] * S[:, :, None]
    ss = (vlad * vlad).sum(axis=2, keepdims=True, dtype=f)
    vlad = vlad * (f(1) / np.maximum(np.sqrt(ss), f(1e-12)))
    # the global scale is applied after the FC (vlad_fc_reduce_kernel): returned beside the vector
    g = (vlad * vlad).sum(axis=2, dtype=f).sum(axis=1, dtype=f)
    return vlad.reshape(N, K * C), f(1) / np.maximum(np.sqrt(g), f(1e-12))


def fc32_ordered(v, inv, fc_w, gating=None):
    """FC in float32: slabs of 512 rows, each added row by row, the slabs added in order; then the global scale."""
    f = np.float32
    fc_w = np.asarray(fc_w, f)
    N, KC = v.shape
    y = np.zeros((N, fc_w.shape[1]), f)
    for j0 in range(0, KC, SLAB):
        acc = np.zeros_like(y)
        for j in range(j0, min(j0 + SLAB, KC)):
            acc += v[:, j, None] * fc_w[j][None, :]
        y = y + acc
    y = y * inv[:, None]
    if gating is None:
        return y
    gw, scale, shift = (np.asarray(a, f) for a in gating)
    acc = np.zeros_like(y)
    for i in range(y.shape[1]):
        acc += y[:, i, None] * gw[i][None, :]
    with np.errstate(over="ignore"):
        return y * (f(1) / (f(1) + np.exp(-(acc * scale + shift), dtype=f)))


def forward32_ordered(x, conv_w, conv_b, centroids, fc_w, normalize_input=True, gating=None):
    v, inv = vlad32_ordered(x, conv_w, conv_b, centroids, normalize_input)
    return fc32_ordered(v, inv, fc_w, gating)


def rows_of_interest(K, C):
    """Rows of the VLAD vector a selection FC looks at: all of them up to 4096, else the first two and last two rows of
    every cluster and of every 512-row slab (where the kernels' loops begin and end)."""
    KC = K * C
    if KC <= 4096:
        return np.arange(KC)
    rows = set()
    for lo, hi in [(k * C, (k + 1) * C) for k in range(K)] + [(j, min(j + SLAB, KC)) for j in range(0, KC, SLAB)]:
        rows.update(r for r in (lo, lo + 1, hi - 2, hi - 1) if lo <= r < hi)
    rows = np.array(sorted(rows))
    assert len(rows) <= 4096
    return rows


def selection_fc(K, C, rows):
    """FC matrix [K*C][len(rows)] with a single 1 per column: the output is those entries of the VLAD vector."""
    rows = np.asarray(rows)
    fc = np.zeros((K * C, len(rows)), np.float32)
    fc[rows, np.arange(len(rows))] = 1.0
    return fc
