"""Yardstick of the recurrent-state tests: a float64 numpy GRU / LSTM stack of any (dirs, L) with an initial state coming in
(hx, cx), the final states going out (h_n, c_n) and their gradients (dh_n, dc_n in; dhx, dcx out).

The oracle's layer functions (oracle/ref_numpy.py) start every sweep from zeros, so this file does not compose them: it is written
out step by step, gate order r, z, n / i, f, g, o as in torch.  tests/test_rnn_state_cpu.py pins it against stock torch.nn.GRU /
torch.nn.LSTM float64 autograd with a random state, and with a zero state against tests/stack_ref.py (the unchanged oracle).

Conventions are those of include/dep_rnn.h: batch-first x (B,T,F); every state array (L*dirs, B, H) ordered [l0_fwd, l0_rev, l1_fwd,
...]; the reverse direction walks t = T-1 .. 0, starts from its own slice of hx / cx, and its h_n / c_n are the states after t = 0; a
layer's output is [y_fwd | y_rev], times a dropout mask before the next layer.
"""
import numpy as np


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _sfx(l, d):
    return f'l{l}' + ('_reverse' if d else '')


def _w(P, prefix, l, d):
    s = _sfx(l, d)
    return [P[f'{prefix}.{n}_{s}'] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


def _order(T, reverse):
    return range(T - 1, -1, -1) if reverse else range(T)


def gru_dir_fwd(x, w_ih, w_hh, b_ih, b_hh, h0, reverse):
    """One direction of one GRU layer.  Returns y (B,T,H), h_n (B,H), cache."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    y = np.zeros((B, T, H))
    steps = {}
    h = h0
    for t in _order(T, reverse):
        gi = x[:, t] @ w_ih.T + b_ih
        gh = h @ w_hh.T + b_hh
        r = _sig(gi[:, :H] + gh[:, :H])
        z = _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        n = np.tanh(gi[:, 2 * H:] + r * hn)
        hnew = (1.0 - z) * n + z * h
        steps[t] = (h, r, z, n, hn)
        y[:, t] = hnew
        h = hnew
    return y, h, (x, steps, reverse)


def gru_dir_bwd(dy, dhn, w_ih, w_hh, cache):
    """dy (B,T,H) gradient of y, dhn (B,H) gradient of h_n.  Returns dx, dW_ih, dW_hh, db_ih, db_hh, dh0."""
    x, steps, reverse = cache
    B, T, _ = x.shape
    dx = np.zeros_like(x)
    dWi = np.zeros_like(w_ih); dWh = np.zeros_like(w_hh)
    dbi = np.zeros(w_ih.shape[0]); dbh = np.zeros(w_hh.shape[0])
    dh = np.array(dhn)
    for t in reversed(list(_order(T, reverse))):
        hp, r, z, n, hn = steps[t]
        d = dh + dy[:, t]
        dn = d * (1.0 - z)
        dan = dn * (1.0 - n * n)
        daz = d * (hp - n) * z * (1.0 - z)
        dar = dan * hn * r * (1.0 - r)
        dgi = np.concatenate([dar, daz, dan], 1)
        dgh = np.concatenate([dar, daz, dan * r], 1)
        dx[:, t] = dgi @ w_ih
        dWi += dgi.T @ x[:, t]; dWh += dgh.T @ hp
        dbi += dgi.sum(0); dbh += dgh.sum(0)
        dh = d * z + dgh @ w_hh
    return dx, dWi, dWh, dbi, dbh, dh


def lstm_dir_fwd(x, w_ih, w_hh, b_ih, b_hh, h0, c0, reverse):
    """One direction of one LSTM layer.  Returns y (B,T,H), h_n, c_n (B,H), cache."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    y = np.zeros((B, T, H))
    steps = {}
    h, c = h0, c0
    for t in _order(T, reverse):
        a = x[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
        i = _sig(a[:, :H]); f = _sig(a[:, H:2 * H]); g = np.tanh(a[:, 2 * H:3 * H]); o = _sig(a[:, 3 * H:])
        cnew = f * c + i * g
        hnew = o * np.tanh(cnew)
        steps[t] = (h, c, i, f, g, o, cnew)
        y[:, t] = hnew
        h, c = hnew, cnew
    return y, h, c, (x, steps, reverse)


def lstm_dir_bwd(dy, dhn, dcn, w_ih, w_hh, cache):
    """Returns dx, dW_ih, dW_hh, db_ih, db_hh, dh0, dc0."""
    x, steps, reverse = cache
    B, T, _ = x.shape
    dx = np.zeros_like(x)
    dWi = np.zeros_like(w_ih); dWh = np.zeros_like(w_hh)
    db = np.zeros(w_ih.shape[0])
    dh = np.array(dhn); dc = np.array(dcn)
    for t in reversed(list(_order(T, reverse))):
        hp, cp, i, f, g, o, cn = steps[t]
        d = dh + dy[:, t]
        tc = np.tanh(cn)
        dct = d * o * (1.0 - tc * tc) + dc
        da = np.concatenate([dct * g * i * (1.0 - i), dct * cp * f * (1.0 - f), dct * i * (1.0 - g * g), d * tc * o * (1.0 - o)], 1)
        dx[:, t] = da @ w_ih
        dWi += da.T @ x[:, t]; dWh += da.T @ hp
        db += da.sum(0)
        dh = da @ w_hh
        dc = dct * f
    return dx, dWi, dWh, db, db.copy(), dh, dc


def stack(x, P, prefix, cell, dirs, L, hx=None, cx=None, pool='none', dy=None, dpooled=None, dhn=None, dcn=None, masks=None):
    """Forward and, when a gradient is given, backward of a dense stack.  hx, cx, dhn, dcn: (L*dirs,B,H) or None (= zeros); cx / dcn
    are the LSTM's.  pool: 'mean' | 'sum' | 'none' over T of the top output, dpooled its gradient; masks: one (B,T,dirs*H) array (or
    None) per lower layer.  Returns dict(y, ys [per layer, undropped], pooled, h_n, c_n (LSTM) [, dx, G, dhx, dcx (LSTM)])."""
    assert cell in ('gru', 'lstm') and dirs in (1, 2) and L >= 1 and pool in ('none', 'mean', 'sum')
    assert cell == 'lstm' or (cx is None and dcn is None)
    B, T, F = x.shape
    H = P[f'{prefix}.weight_hh_l0'].shape[1]
    zero = np.zeros((L * dirs, B, H))
    hx = zero if hx is None else hx
    cx = zero if cx is None else cx
    caches, hn, cn, ys = [], [], [], []
    inp = x
    for l in range(L):
        outs = []
        for d in range(dirs):
            k = l * dirs + d
            if cell == 'gru':
                y, h, c = gru_dir_fwd(inp, *_w(P, prefix, l, d), hx[k], bool(d))
            else:
                y, h, cc, c = lstm_dir_fwd(inp, *_w(P, prefix, l, d), hx[k], cx[k], bool(d))
                cn.append(cc)
            outs.append(y); hn.append(h); caches.append(c)
        out = outs[0] if dirs == 1 else np.concatenate(outs, -1)
        ys.append(out)
        inp = out
        if l < L - 1 and masks is not None and masks[l] is not None:
            inp = out * masks[l]
    res = dict(y=out, ys=ys, h_n=np.stack(hn, 0), pooled=None)
    if cell == 'lstm':
        res['c_n'] = np.stack(cn, 0)
    if pool != 'none':
        res['pooled'] = out.mean(1) if pool == 'mean' else out.sum(1)
    if dy is None and dpooled is None and dhn is None and dcn is None:
        return res
    g = np.zeros_like(out)
    if dy is not None:
        g = g + dy
    if dpooled is not None:
        assert pool != 'none'
        g = g + dpooled[:, None, :] * ((1.0 / T) if pool == 'mean' else 1.0)
    dhn = zero if dhn is None else dhn
    dcn = zero if dcn is None else dcn
    G = {}
    dhx = np.zeros_like(zero); dcx = np.zeros_like(zero)
    for l in range(L - 1, -1, -1):
        if l < L - 1 and masks is not None and masks[l] is not None:
            g = g * masks[l]
        dxs = []
        for d in range(dirs):
            k = l * dirs + d
            w_ih, w_hh, _, _ = _w(P, prefix, l, d)
            gd = g[..., d * H:(d + 1) * H]
            if cell == 'gru':
                dx, dWi, dWh, dbi, dbh, dhx[k] = gru_dir_bwd(gd, dhn[k], w_ih, w_hh, caches[k])
            else:
                dx, dWi, dWh, dbi, dbh, dhx[k], dcx[k] = lstm_dir_bwd(gd, dhn[k], dcn[k], w_ih, w_hh, caches[k])
            s = _sfx(l, d)
            G[f'{prefix}.weight_ih_{s}'] = dWi; G[f'{prefix}.weight_hh_{s}'] = dWh
            G[f'{prefix}.bias_ih_{s}'] = dbi; G[f'{prefix}.bias_hh_{s}'] = dbh
            dxs.append(dx)
        g = dxs[0] if dirs == 1 else dxs[0] + dxs[1]
    res.update(dx=g, G=G, dhx=dhx)
    if cell == 'lstm':
        res['dcx'] = dcx
    return res
