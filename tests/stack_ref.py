"""Expectation builder of the stack-depth tests: one recurrent stack of any (cell, dirs, L), composed from the UNCHANGED oracle's
layer functions (oracle/ref_numpy.py gru_layer_fwd / gru_layer_bwd, lstm_dir_fwd / lstm_dir_bwd), the way tests/bigru_ref.py is.

A GRU's reverse direction is the forward layer on the time-flipped input, flipped back; the LSTM's layer function has its own
`reverse`.  A layer's output is [y_fwd | y_rev] along the last axis (times a dropout mask before the next layer); h_n is ordered
[l0_fwd, l0_rev, l1_fwd, ...], (L*dirs, B, H).  The backward takes the gradient of the top output and dh_n for EVERY layer and
direction, added at the sweep's last live step (GRU: onto dy there; LSTM: lstm_dir_bwd's own dhn), and carries the summed input
gradient of the directions down.  The ragged form is the row loop of tests/varlen_ref.py: row b is the dense result of
x[b:b+1, :lengths[b]] alone, an empty row contributes nothing.  tests/test_stack_ref_cpu.py pins all of it against stock
torch.nn.GRU / torch.nn.LSTM in float64, and at L = 2 against the oracle's own gru_stack_* / bilstm_stack_*.
"""
import numpy as np

from oracle import ref_numpy as R


def _sfx(l, d):
    return f'l{l}' + ('_reverse' if d else '')


def _w(P, prefix, l, d):
    s = _sfx(l, d)
    return [P[f'{prefix}.{n}_{s}'] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


def stack_fwd(x, P, prefix, cell, dirs, L, masks=None):
    """x (B,T,F) -> top output (B,T,dirs*H), h_n (L*dirs,B,H), caches (one per layer and direction), per-layer outputs (undropped)."""
    caches, hn, ys = [], [], []
    inp = x
    for l in range(L):
        outs = []
        for d in range(dirs):
            w_ih, w_hh, b_ih, b_hh = _w(P, prefix, l, d)
            if cell == 'gru':
                y, c = R.gru_layer_fwd(np.ascontiguousarray(inp[:, ::-1]) if d else inp, w_ih, w_hh, b_ih, b_hh)
                hn.append(y[:, -1])                          # the state after the sweep's last step (reverse: step 0)
                outs.append(y[:, ::-1] if d else y)
            else:
                y, h, c = R.lstm_dir_fwd(inp, w_ih, w_hh, b_ih, b_hh, bool(d))
                hn.append(h); outs.append(y)
            caches.append(c)
        out = outs[0] if dirs == 1 else np.concatenate(outs, -1)
        ys.append(out)
        inp = out
        if l < L - 1 and masks is not None and masks[l] is not None:
            inp = out * masks[l]
    return out, np.stack(hn, 0), caches, ys


def stack_bwd(dout, dhn, P, prefix, cell, dirs, L, caches, masks=None):
    """dout (B,T,dirs*H) gradient of the top output; dhn (L*dirs,B,H) gradient of h_n.  Returns dx, {name: gradient}."""
    G = {}
    H = dhn.shape[-1]
    d = dout
    for l in range(L - 1, -1, -1):
        if l < L - 1 and masks is not None and masks[l] is not None:
            d = d * masks[l]
        dxs = []
        for dd in range(dirs):
            w_ih, w_hh, _, _ = _w(P, prefix, l, dd)
            dyd = d[..., dd * H:(dd + 1) * H]
            if cell == 'gru':
                dyd = np.array(dyd[:, ::-1] if dd else dyd)  # sweep order (a copy: dh_n is added below)
                dyd[:, -1] += dhn[l * dirs + dd]
                dx, dWi, dWh, dbi, dbh = R.gru_layer_bwd(dyd, w_ih, w_hh, caches[l * dirs + dd])
                dx = dx[:, ::-1] if dd else dx
            else:
                dx, dWi, dWh, dbi, dbh = R.lstm_dir_bwd(dyd, dhn[l * dirs + dd], w_ih, w_hh, caches[l * dirs + dd])
            s = _sfx(l, dd)
            G[f'{prefix}.weight_ih_{s}'] = dWi; G[f'{prefix}.weight_hh_{s}'] = dWh
            G[f'{prefix}.bias_ih_{s}'] = dbi; G[f'{prefix}.bias_hh_{s}'] = dbh
            dxs.append(dx)
        d = dxs[0] if dirs == 1 else 0.0 + dxs[0] + dxs[1]   # (the summation order of R.bilstm_stack_bwd)
    return d, G


def stack(x, P, prefix, cell, dirs, L, lengths=None, pool='none', dy=None, dpooled=None, dhn=None, masks=None):
    """Dense (lengths None: the whole batch at once) or ragged (a loop over rows) forward and, when a gradient is given, backward.
    Returns dict(y (B,T,dirs*H), ys [per layer], pooled (B,dirs*H), h_n (L*dirs,B,H) [, dx, G]).  pool: 'mean' | 'sum' | 'none' over
    the live steps of y; dpooled (B,dirs*H) is the gradient of that pool; masks: one (B,T,dirs*H) array (or None) per lower layer."""
    assert cell in ('gru', 'lstm') and dirs in (1, 2) and L >= 1 and pool in ('none', 'mean', 'sum')
    assert dpooled is None or pool != 'none'
    B, T, F = x.shape
    H = P[f'{prefix}.weight_hh_l0'].shape[1]
    W = dirs * H
    want = dy is not None or dpooled is not None or dhn is not None
    res = dict(y=np.zeros((B, T, W)), ys=[np.zeros((B, T, W)) for _ in range(L)], pooled=np.zeros((B, W)), h_n=np.zeros((L * dirs, B, H)))
    if want:
        res['dx'] = np.zeros((B, T, F))
        res['G'] = {k: np.zeros_like(v) for k, v in P.items() if k.startswith(prefix + '.')}
    blocks = [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), int(lengths[b])) for b in range(B)]
    for rows, n in blocks:
        if n == 0:
            continue                                         # an empty row contributes nothing
        mb = None if masks is None else [None if m is None else m[rows, :n] for m in masks]
        y, hn, caches, ys = stack_fwd(x[rows, :n], P, prefix, cell, dirs, L, mb)
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
            dh = dhn[:, rows] if dhn is not None else np.zeros((L * dirs, y.shape[0], H))
            dx, G = stack_bwd(d, dh, P, prefix, cell, dirs, L, caches, mb)
            res['dx'][rows, :n] = dx
            for k, v in G.items():
                res['G'][k] += v
    return res
