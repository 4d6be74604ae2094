"""Expectation builder of the ragged-batch tests: a Python loop over rows around the UNCHANGED oracle (oracle/ref_numpy.py).

Row b of a ragged call is, by definition, what the dense path gives for that utterance alone, x[b:b+1, :lengths[b]], at
T' = lengths[b]; positions t >= lengths[b] of every output sequence are 0; weight gradients are the sum over rows; an empty row
contributes nothing.  tests/test_varlen_cpu.py pins this builder against stock torch's packed nn.GRU / nn.LSTM.
"""
import numpy as np

from oracle import ref_numpy as R


def lengths_mix(B, T, rng=None):
    """A length vector with, where B and T allow: a full row, 1, 0, a length on either side of a 16-row tile boundary (rows 15
    and 16 differ), and a whole 16-row tile of short rows (rows 16..31: lengths <= 2); the rest uniform in [0, T]."""
    rng = rng or np.random.default_rng(B * 131 + T)
    n = rng.integers(0, T + 1, B)
    fixed = [T, 1, 0]
    for i, v in enumerate(fixed[:B]):
        n[i] = min(v, T)
    if B > 16:
        n[15] = T; n[16] = min(1, T)
    if B >= 32:
        n[16:32] = rng.integers(0, min(2, T) + 1, 16)
        n[16] = min(1, T)
    if B >= 48:
        n[32] = T
    return n.astype(np.int32)


def _row_masks(masks, b, n):
    if masks is None:
        return None
    return [None if m is None else m[b:b + 1, :n] for m in masks]


def gru_ragged(x, lengths, P, prefix, L, pool='mean', dy=None, dpooled=None, dhn_top=None, masks=None):
    """Row loop around gru_stack_fwd / gru_stack_bwd.  Returns dict(y, pooled, h_n [, dx, G]).  h_n: (L, B, H), the state after each
    row's last step.  dhn_top: (B, H) gradient of the TOP layer's h_n (the oracle's BPTT has no other entry for it than dy)."""
    B, T, F = x.shape
    H = P[f'{prefix}.weight_hh_l0'].shape[1]
    y = np.zeros((B, T, H)); pooled = np.zeros((B, H)); h_n = np.zeros((L, B, H))
    want = dy is not None or dpooled is not None or dhn_top is not None
    dx = np.zeros((B, T, F)) if want else None
    G = {k: np.zeros_like(v) for k, v in P.items() if k.startswith(prefix + '.')} if want else None
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            continue
        mb = _row_masks(masks, b, n)
        yb, caches = R.gru_stack_fwd(x[b:b + 1, :n], P, prefix, L, mb)
        y[b, :n] = yb[0]
        pooled[b] = yb[0].mean(0) if pool == 'mean' else yb[0].sum(0)
        for l in range(L):
            h_n[l, b] = caches[l][1][0, -1]
        if want:
            d = np.zeros((1, n, H))
            if dy is not None:
                d += dy[b:b + 1, :n]
            if dpooled is not None:
                d += dpooled[b][None, None, :] * ((1.0 / n) if pool == 'mean' else 1.0)
            if dhn_top is not None:
                d[0, n - 1] += dhn_top[b]
            dxb, Gb = R.gru_stack_bwd(d, P, prefix, L, caches, mb)
            dx[b, :n] = dxb[0]
            for k, v in Gb.items():
                G[k] += v
    out = dict(y=y, pooled=pooled, h_n=h_n)
    if want:
        out.update(dx=dx, G=G)
    return out


def bilstm_ragged(x, lengths, P, prefix, L, dy=None, dhn=None, masks=None):
    """Row loop around bilstm_stack_fwd / bilstm_stack_bwd.  Returns dict(y (B,T,2H), h_n (2L,B,H) [, dx, G])."""
    B, T, F = x.shape
    H = P[f'{prefix}.weight_hh_l0'].shape[1]
    y = np.zeros((B, T, 2 * H)); h_n = np.zeros((2 * L, B, H))
    want = dy is not None or dhn is not None
    dx = np.zeros((B, T, F)) if want else None
    G = {k: np.zeros_like(v) for k, v in P.items() if k.startswith(prefix + '.')} if want else None
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            continue
        mb = _row_masks(masks, b, n)
        yb, hb, caches = R.bilstm_stack_fwd(x[b:b + 1, :n], P, prefix, L, mb)
        y[b, :n] = yb[0]; h_n[:, b] = hb[:, 0]
        if want:
            d = dy[b:b + 1, :n] if dy is not None else np.zeros((1, n, 2 * H))
            dh = dhn[:, b:b + 1] if dhn is not None else np.zeros((2 * L, 1, H))
            dxb, Gb = R.bilstm_stack_bwd(d, dh, P, prefix, L, caches, mb)
            dx[b, :n] = dxb[0]
            for k, v in Gb.items():
                G[k] += v
    out = dict(y=y, h_n=h_n)
    if want:
        out.update(dx=dx, G=G)
    return out


def attention_ragged(out, lengths, hn, Wa, ba, dctx=None):
    """Row loop around attention_fwd / attention_bwd: softmax over t < len_b; an empty row gives ctx = 0 and no gradient."""
    B, T, H2 = out.shape
    H = H2 // 2; K = hn.shape[0]
    ctx = np.zeros((B, H)); alpha = np.zeros((B, T))
    dout = np.zeros_like(out); dhn = np.zeros_like(hn); dWa = np.zeros_like(Wa); dba = np.zeros_like(ba)
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            continue
        c, cache = R.attention_fwd(out[b:b + 1, :n], hn[:, b:b + 1], Wa, ba)
        ctx[b] = c[0]; alpha[b, :n] = cache[5][0]
        if dctx is not None:
            do, dh, dW, db = R.attention_bwd(dctx[b:b + 1], Wa, cache)
            dout[b, :n] = do[0]; dhn[:, b] = dh[:, 0]; dWa += dW; dba += db
    res = dict(ctx=ctx, alpha=alpha)
    if dctx is not None:
        res.update(dout=dout, dhn=dhn, dWa=dWa, dba=dba)
    return res


def audio_ragged_step(P, x, lengths, y_t, cfg, variant):
    """One training step's loss and gradients of the audio model on a ragged batch: rows run alone through R.audio_forward /
    R.audio_backward, the loss is the batch mean (CE on probabilities for 'clf', L1 for 'reg')."""
    B = x.shape[0]
    outs, caches = [], []
    for b in range(B):
        n = int(lengths[b])
        o, c = R.audio_forward(P, x[b:b + 1, :n], cfg, variant)
        outs.append(o[0]); caches.append(c)
    out = np.stack(outs)
    loss, dout = (R.ce_on_probs(out, y_t) if variant == 'clf' else R.l1_loss(out, y_t))
    G = None
    for b in range(B):
        _, Gb = R.audio_backward(P, dout[b:b + 1], caches[b])
        G = Gb if G is None else {k: G[k] + Gb[k] for k in G}
    return out, loss, G


def text_ragged_step(P, x, lengths, y_t, cfg, variant):
    B = x.shape[0]
    outs, caches = [], []
    for b in range(B):
        n = int(lengths[b])
        o, c = R.text_forward(P, x[b:b + 1, :n], cfg, variant)
        outs.append(o[0]); caches.append(c)
    out = np.stack(outs)
    loss, dout = (R.ce_on_probs(out, y_t) if variant == 'clf' else R.smooth_l1_loss(out, y_t))
    G = None
    for b in range(B):
        _, Gb = R.text_backward(P, dout[b:b + 1], caches[b])
        G = Gb if G is None else {k: G[k] + Gb[k] for k in G}
    return out, loss, G
