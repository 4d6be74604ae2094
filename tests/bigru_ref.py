"""Expectation builder of the bidirectional-GRU tests: a composition of the UNCHANGED oracle's unidirectional layer
(oracle/ref_numpy.py gru_layer_fwd / gru_layer_bwd).

The reverse direction of a layer is the forward layer on the time-flipped input, flipped back; a layer's output is
[y_fwd | y_rev] along the last axis (optionally times a dropout mask before the next layer); h_n is ordered
[l0_fwd, l0_rev, l1_fwd, ...] and the reverse entry is the state after step 0.  The backward splits the incoming gradient into
the two column halves, flips the reverse half, adds dh_n at the last step in sweep order, runs the layer's BPTT per direction and
sums the two input gradients.  The ragged form is a row loop in the style of tests/varlen_ref.py: row b is the dense result of
x[b:b+1, :lengths[b]] alone.  tests/test_bigru_cpu.py pins both forms against stock torch.nn.GRU(bidirectional=True).
"""
import numpy as np

from oracle import ref_numpy as R


def _sfx(l, d):
    return f'l{l}' + ('_reverse' if d else '')


def _w(P, prefix, l, d):
    s = _sfx(l, d)
    return [P[f'{prefix}.{n}_{s}'] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


def bigru_stack_fwd(x, P, prefix, L, masks=None):
    """x (B,T,F) -> top output (B,T,2H), h_n (2L,B,H), caches (one per layer and direction), per-layer outputs (before dropout)."""
    caches, hn, ys = [], [], []
    inp = x
    for l in range(L):
        outs = []
        for d in (0, 1):
            w_ih, w_hh, b_ih, b_hh = _w(P, prefix, l, d)
            y, c = R.gru_layer_fwd(np.ascontiguousarray(inp[:, ::-1]) if d else inp, w_ih, w_hh, b_ih, b_hh)
            hn.append(y[:, -1])                              # the state after the sweep's last step (reverse: step 0)
            outs.append(y[:, ::-1] if d else y); caches.append(c)
        out = np.concatenate(outs, -1)
        ys.append(out)
        inp = out
        if l < L - 1 and masks is not None and masks[l] is not None:
            inp = out * masks[l]
    return out, np.stack(hn, 0), caches, ys


def bigru_stack_bwd(dout, dhn, P, prefix, L, caches, masks=None):
    """dout (B,T,2H) gradient of the top output; dhn (2L,B,H) gradient of h_n.  Returns dx, {name: gradient}."""
    G = {}
    H = dhn.shape[-1]
    d = dout
    for l in range(L - 1, -1, -1):
        if l < L - 1 and masks is not None and masks[l] is not None:
            d = d * masks[l]
        dx_sum = 0.0
        for dd in (0, 1):
            w_ih, w_hh, _, _ = _w(P, prefix, l, dd)
            dyd = d[..., dd * H:(dd + 1) * H]
            dyd = np.array(dyd[:, ::-1] if dd else dyd)      # sweep order (a copy: dh_n is added below)
            dyd[:, -1] += dhn[2 * l + dd]
            dx, dWi, dWh, dbi, dbh = R.gru_layer_bwd(dyd, w_ih, w_hh, caches[2 * l + dd])
            s = _sfx(l, dd)
            G[f'{prefix}.weight_ih_{s}'] = dWi; G[f'{prefix}.weight_hh_{s}'] = dWh
            G[f'{prefix}.bias_ih_{s}'] = dbi; G[f'{prefix}.bias_hh_{s}'] = dbh
            dx_sum = dx_sum + (dx[:, ::-1] if dd else dx)
        d = dx_sum
    return d, G


def bigru(x, P, prefix, L, lengths=None, pool='none', dy=None, dpooled=None, dhn=None, masks=None):
    """Dense (lengths None: the whole batch at once) or ragged (a loop over rows) forward and, when a gradient is given, backward.
    Returns dict(y (B,T,2H), ys [per layer], pooled (B,2H), h_n (2L,B,H) [, dx, G]).  pool: 'mean' | 'sum' | 'none' over the live
    steps of y; dpooled (B,2H) is the gradient of that pool."""
    B, T, F = x.shape
    H = P[f'{prefix}.weight_hh_l0'].shape[1]
    want = dy is not None or dpooled is not None or dhn is not None
    res = dict(y=np.zeros((B, T, 2 * H)), ys=[np.zeros((B, T, 2 * H)) for _ in range(L)], pooled=np.zeros((B, 2 * H)),
               h_n=np.zeros((2 * L, B, H)))
    if want:
        res['dx'] = np.zeros((B, T, F))
        res['G'] = {k: np.zeros_like(v) for k, v in P.items() if k.startswith(prefix + '.')}
    blocks = [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), int(lengths[b])) for b in range(B)]
    for rows, n in blocks:
        if n == 0:
            continue                                         # an empty row contributes nothing
        mb = None if masks is None else [None if m is None else m[rows, :n] for m in masks]
        y, hn, caches, ys = bigru_stack_fwd(x[rows, :n], P, prefix, L, mb)
        res['y'][rows, :n] = y; res['h_n'][:, rows] = hn
        for l in range(L):
            res['ys'][l][rows, :n] = ys[l]
        if pool != 'none':
            res['pooled'][rows] = y.mean(1) if pool == 'mean' else y.sum(1)
        if want:
            d = np.zeros_like(y)
            if dy is not None:
                d += dy[rows, :n]
            if dpooled is not None:
                d += dpooled[rows][:, None, :] * ((1.0 / n) if pool == 'mean' else 1.0)
            dh = dhn[:, rows] if dhn is not None else np.zeros((2 * L, y.shape[0], H))
            dx, G = bigru_stack_bwd(d, dh, P, prefix, L, caches, mb)
            res['dx'][rows, :n] = dx
            for k, v in G.items():
                res['G'][k] += v
    return res
