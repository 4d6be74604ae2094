"""Expectation builder of the ragged recurrent-state tests (dep_rnn_forward_state_varlen / dep_rnn_backward_state_varlen): a Python
loop over rows around the UNCHANGED tests/hx_ref.stack (float64 numpy, pinned against stock torch in tests/test_rnn_state_cpu.py).

Row b of a ragged state call is, by definition, what the dense state call gives for that row alone: x[b:b+1, :len_b] with the row's
slices of hx / cx / dh_n / dc_n and the row's dropout masks, at T' = len_b.  Positions t >= len_b of every output sequence and of dx
are 0; weight gradients are the sum over rows; the pool follows the varlen rule (the mean divides by len_b).

len_b = 0 is written out explicitly, the state passes through: h_n[:, b] = hx[:, b], c_n[:, b] = cx[:, b], dhx[:, b] = dh_n[:, b],
dcx[:, b] = dc_n[:, b]; y, pooled, dx of the row are 0 and it adds nothing to a weight gradient.  This is the only rule under which
chunks compose (tests/test_state_varlen_cpu.py, chunk composition): a row that ended in an earlier chunk must hand its state, and on
the way back its state gradient, through the later chunks untouched.

tests/test_state_varlen_cpu.py pins this builder against stock torch's packed nn.GRU / nn.LSTM with a random state.
"""
import numpy as np

import hx_ref


def stack(x, lengths, P, prefix, cell, dirs, L, hx=None, cx=None, pool='none', dy=None, dpooled=None, dhn=None, dcn=None, masks=None):
    """Same arguments and results as hx_ref.stack, plus lengths (B ints in [0, T]).  Returns dict(y, ys, pooled, h_n, c_n (LSTM)
    [, dx, G, dhx, dcx (LSTM)]); pooled is None for pool == 'none'."""
    B, T, F = x.shape
    H = P[f'{prefix}.weight_hh_l0'].shape[1]
    K, W = L * dirs, dirs * H
    lstm = cell == 'lstm'
    zero = np.zeros((K, B, H))
    hx = zero if hx is None else hx
    cx = zero if cx is None else cx
    want = dy is not None or dpooled is not None or dhn is not None or dcn is not None
    dhn_ = zero if dhn is None else dhn
    dcn_ = zero if dcn is None else dcn
    res = dict(y=np.zeros((B, T, W)), ys=[np.zeros((B, T, W)) for _ in range(L)], h_n=np.zeros((K, B, H)),
               pooled=None if pool == 'none' else np.zeros((B, W)))
    if lstm:
        res['c_n'] = np.zeros((K, B, H))
    if want:
        res.update(dx=np.zeros((B, T, F)), dhx=np.zeros((K, B, H)),
                   G={k: np.zeros_like(v) for k, v in P.items() if k.startswith(prefix + '.')})
        if lstm:
            res['dcx'] = np.zeros((K, B, H))
    for b in range(B):
        n = int(lengths[b])
        assert 0 <= n <= T
        if n == 0:
            # the state passes through; everything else of the row stays 0
            res['h_n'][:, b] = hx[:, b]
            if lstm:
                res['c_n'][:, b] = cx[:, b]
            if want:
                res['dhx'][:, b] = dhn_[:, b]
                if lstm:
                    res['dcx'][:, b] = dcn_[:, b]
            continue
        row = lambda a: None if a is None else a[:, b:b + 1]
        mb = None if masks is None else [None if m is None else m[b:b + 1, :n] for m in masks]
        r = hx_ref.stack(x[b:b + 1, :n], P, prefix, cell, dirs, L, hx=hx[:, b:b + 1], cx=cx[:, b:b + 1] if lstm else None, pool=pool,
                         dy=None if dy is None else dy[b:b + 1, :n], dpooled=None if dpooled is None else dpooled[b:b + 1],
                         dhn=row(dhn), dcn=row(dcn), masks=mb)
        res['y'][b, :n] = r['y'][0]
        for l in range(L):
            res['ys'][l][b, :n] = r['ys'][l][0]
        res['h_n'][:, b] = r['h_n'][:, 0]
        if pool != 'none':
            res['pooled'][b] = r['pooled'][0]
        if lstm:
            res['c_n'][:, b] = r['c_n'][:, 0]
        if want:
            res['dx'][b, :n] = r['dx'][0]
            res['dhx'][:, b] = r['dhx'][:, 0]
            if lstm:
                res['dcx'][:, b] = r['dcx'][:, 0]
            for k, g in r['G'].items():
                res['G'][k] += g
    return res
