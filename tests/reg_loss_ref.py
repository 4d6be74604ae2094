"""Float64 numpy restatement of the regression criteria of dep_head_loss_reg: L1, SmoothL1(beta), Huber(delta)
and MSE on o = max(z, 0) (relu) or o = z, with per-row weights.  With d = o - target, a = |d| (torch's CPU formulas):

    l1         l = a                                            dl/do = sgn(d)                       (0 at d == 0)
    smooth_l1  l = a < beta  ? 0.5 d^2 / beta : a - 0.5 beta    dl/do = a < beta  ? d / beta : sgn(d)      (beta == 0: l1)
    huber      l = a < delta ? 0.5 d^2 : delta (a - 0.5 delta)  dl/do = a < delta ? d : delta sgn(d)
    mse        l = d^2                                          dl/do = 2 d

    row_i = w_i sum_c l_ic                       (w_i = 1 without weights)
    den   = C sum_i w_i                          (or the explicit `den` of a shard / micro-batch: the whole batch's)
    loss  = sum_i row_i / den
    dz_ic = w_i dl/do [not relu, or z > 0] / den

A row whose weight is exactly 0 is an ignored row: row_i and dz_i are exactly 0 -- selected, not multiplied -- whatever its target
holds, NaN included; its `out` row is still o.

Imports nothing from the package under test.  tests/test_reg_loss_cpu.py holds it against torch.nn.functional."""
import numpy as np

FORMS = ('l1', 'smooth_l1', 'huber', 'mse')


def denominator(B, C, weight=None):
    return float(B * C) if weight is None else float(C * np.asarray(weight, np.float64).sum())


def elementwise(d, form, param):
    """(l, dl/dd) per element."""
    a = np.abs(d)
    sg = np.sign(d)
    if form == 'l1':
        return a, sg
    if form == 'smooth_l1':
        quad = a < param
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(quad, 0.5 * d * d / param, a - 0.5 * param), np.where(quad, d / param, sg)
    if form == 'huber':
        quad = a < param
        return np.where(quad, 0.5 * d * d, param * (a - 0.5 * param)), np.where(quad, d, param * sg)
    assert form == 'mse'
    return d * d, 2.0 * d


def reg_loss(z, target, form, param=1.0, relu=True, weight=None, den=None):
    """-> (out, rows, loss, dz): out = o (B,C), rows (B,), loss a float (NaN when every weight is 0: den = 0), dz (B,C)."""
    assert form in FORMS
    z = np.asarray(z, np.float64)
    B, C = z.shape
    t = np.asarray(target, np.float64).reshape(B, C)
    w = np.ones(B) if weight is None else np.asarray(weight, np.float64).reshape(B)
    live = w != 0.0
    o = np.maximum(z, 0.0) if relu else z
    with np.errstate(invalid='ignore'):
        l, g = elementwise(o - t, form, float(param))
        rows = np.where(live, w * l.sum(1), 0.0)
        if den is None:
            den = denominator(B, C, weight)
        with np.errstate(divide='ignore'):
            loss = float(np.float64(rows.sum()) / np.float64(den))              # den = 0 with every row ignored: 0 / 0 = NaN
            passes = (z > 0) if relu else np.ones_like(z, dtype=bool)
            dz = np.where(live[:, None] & passes, w[:, None] * g / den, 0.0)
    return o, rows, loss, dz


def inputs_with_edges(rng, B, C, knee):
    """Test inputs: z = 2 N(0, 1) (ReLU cuts about half), targets uniform in [-1, 3]; the first elements are overwritten so that d is
    exactly +knee, -knee and 0 on a passing z > 0, and z is exactly 0 and negative where ReLU cuts (knee <= 0: 1 stands in).  The
    overwritten values are dyadic: every such d is exact in float32 and in float64."""
    z = rng.standard_normal((B, C)) * 2
    t = rng.uniform(-1.0, 3.0, (B, C))
    zf, tf = z.reshape(-1), t.reshape(-1)
    k = float(knee) if knee > 0 else 1.0
    edges = [(2.5, 2.5 - k), (1.25, 1.25 + k), (0.75, 0.75), (0.0, 0.5), (-1.5, 0.25), (0.0, 0.0)]
    for i, (zv, tv) in enumerate(edges[:zf.size]):
        zf[i] = zv; tf[i] = tv
    return z, t
