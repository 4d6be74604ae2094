"""Float64 numpy restatement of the weighted / smoothed / masked cross-entropy of the fused CE losses, for both
kinds: 'logits' (a = z) and 'on_softmax' (a = softmax(z), the reference's double softmax).  With lq = log_softmax(a), q = exp(lq),
w the class weights (ones when absent), W = sum_c w_c, eps the label smoothing, live_i = (y_i != ignore_index):

    row_i = live_i [ (1-eps) w[y_i] (-lq[i,y_i]) + (eps/C) sum_c w_c (-lq[i,c]) ]
    den   = sum_i live_i w[y_i]                     (or the explicit `den` of a shard / micro-batch: the whole batch's)
    loss  = sum_i row_i / den
    dL/da = live_i [ (1-eps) w[y_i] (q - onehot(y_i)) + (eps/C) (q W - w) ] / den
    dz    = dL/da  (logits) ;  p (dL/da - sum_c p_c dL/da_c), p = softmax(z)  (on_softmax)

Imports nothing from the package under test.  tests/test_weighted_loss_cpu.py holds it against torch.nn.functional.cross_entropy."""
import numpy as np

KINDS = ('logits', 'on_softmax')


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def log_softmax(a):
    a = np.asarray(a, np.float64)
    d = a - a.max(1, keepdims=True)
    return d - np.log(np.exp(d).sum(1, keepdims=True))


def denominator(y, weight=None, ignore_index=-100):
    y = np.asarray(y).reshape(-1).astype(np.int64)
    live = y != ignore_index
    if weight is None:
        return float(live.sum())
    return float(np.asarray(weight, np.float64)[y[live]].sum())


def weighted_ce(z, y, kind='logits', weight=None, label_smoothing=0.0, ignore_index=-100, den=None):
    """-> (out, rows, loss, dz): out = softmax(z) (B,C), rows (B,), loss a float (NaN when no row is live: den = 0), dz (B,C)."""
    assert kind in KINDS
    z = np.asarray(z, np.float64)
    y = np.asarray(y).reshape(-1).astype(np.int64)
    B, C = z.shape
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64).reshape(C)
    eps = float(label_smoothing)
    p = softmax(z)
    a = z if kind == 'logits' else p
    lq = log_softmax(a)
    q = np.exp(lq)
    live = y != ignore_index
    ys = np.where(live, y, 0)
    onehot = np.zeros((B, C)); onehot[np.arange(B), ys] = 1.0
    wy = w[ys]
    rows = np.where(live, (1.0 - eps) * wy * -lq[np.arange(B), ys] + (eps / C) * (-lq * w).sum(1), 0.0)
    if den is None:
        den = float((live * wy).sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        loss = float(np.float64(rows.sum()) / np.float64(den))                  # den = 0 with no live row: 0 / 0 = NaN, as in torch
        da = np.where(live[:, None], ((1.0 - eps) * wy[:, None] * (q - onehot) + (eps / C) * (q * w.sum() - w)) / den, 0.0)   # an ignored row: exactly 0
        dz = da if kind == 'logits' else p * (da - (p * da).sum(1, keepdims=True))
    return p, rows, loss, dz
