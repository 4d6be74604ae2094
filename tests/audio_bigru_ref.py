"""Yardstick of the bidirectional audio encoder (AudioGRU with config['bidirectional'] = True): a float64 composition of what the
oracle already has, none of it restated --

    [LayerNorm (clf)] -> bidirectional GRU stack (tests/bigru_ref.py) -> attention_net_with_w(output, h_n) -> Dropout, Linear, ReLU,
    Dropout, Linear -> Softmax + CE on the probabilities (clf) | ReLU + L1 (reg)

with oracle.ref_numpy's layernorm_fwd/_bwd, attention_fwd/_bwd, mlp_head_fwd/_bwd, ce_on_probs / softmax_bwd / l1_loss and adam_step.
Dropout is fed ref_numpy.dropout_mask at the model's seed and sites: DEP_SITE_RNN0 + l over element (b, t, col) of the (B, T, 2H) output
of layer l, and the head's two sites as tests/head_ref.py draws them.  The ragged form loops over rows: row b is the encoder on
x[b:b+1, :lengths[b]] alone, a row of length 0 has ctx = 0 and passes no gradient into the encoder; the head and the loss see the
whole batch.  tests/test_audio_bigru_cpu.py pins the dense form against stock torch with autograd.
"""
import numpy as np

import head_ref
from bigru_ref import bigru
from oracle import ref_numpy as R

PX = 'lstm_net_audio'
SITE_RNN0 = 16                                      # DEP_SITE_RNN0 (include/dep_rnn.h)
HEAD_SITES = (1, 2)                                 # _lib.SITE_FC0, _lib.SITE_FC1


def key_list(variant, Lyr):
    """state_dict() keys of the reference class built with nn.GRU(..., bidirectional=True), in its definition order."""
    keys = ['attention_layer.0.weight', 'attention_layer.0.bias']
    for l in range(Lyr):
        for sfx in ('', '_reverse'):
            keys += [f'{PX}.{n}_l{l}{sfx}' for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    keys += ['ln.weight', 'ln.bias'] if variant == 'clf' else ['bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var', 'bn.num_batches_tracked']
    return keys + ['fc_audio.1.weight', 'fc_audio.1.bias', 'fc_audio.4.weight', 'fc_audio.4.bias']


def live_names(variant, Lyr):
    """The parameters that receive a gradient: everything but the regression class's unused BatchNorm."""
    return [k for k in key_list(variant, Lyr) if not k.startswith('bn.')]


def make_params(rng, F, H, Lyr, C, variant):
    """float32-rounded float64 parameters at nn.GRU / nn.Linear's init scale, gamma and beta off their defaults."""
    P = {}
    shapes = {'attention_layer.0.weight': (H, H), 'attention_layer.0.bias': (H,), 'fc_audio.1.weight': (H, H), 'fc_audio.1.bias': (H,),
              'fc_audio.4.weight': (C, H), 'fc_audio.4.bias': (C,)}
    for l in range(Lyr):
        for sfx in ('', '_reverse'):
            inp = F if l == 0 else 2 * H
            shapes.update({f'{PX}.weight_ih_l{l}{sfx}': (3 * H, inp), f'{PX}.weight_hh_l{l}{sfx}': (3 * H, H),
                           f'{PX}.bias_ih_l{l}{sfx}': (3 * H,), f'{PX}.bias_hh_l{l}{sfx}': (3 * H,)})
    k = 1.0 / np.sqrt(H)
    for name in live_names(variant, Lyr):
        if name == 'ln.weight':
            P[name] = head_ref.f64(1.0 + 0.3 * rng.standard_normal(F))
        elif name == 'ln.bias':
            P[name] = head_ref.f64(0.3 * rng.standard_normal(F))
        else:
            P[name] = head_ref.f64(rng.uniform(-k, k, shapes[name]))
    if variant == 'reg':                             # keep the output ReLU live: a row with z <= 0 passes no gradient at all
        P['fc_audio.4.bias'] = head_ref.f64(P['fc_audio.4.bias'] + 1.0)
    return P


def masks(B, T, H, Lyr, p, seed):
    """{'rnn': [mask of layer l's output (B, T, 2H) for l < Lyr - 1], 'fc0': (B, H), 'fc1': (B, H)} or {} at p = 0."""
    if not p > 0:
        return {}
    m0, m1 = head_ref.masks(B, H, H, p, seed, HEAD_SITES, True)
    rnn = [R.dropout_mask(B * T * 2 * H, p, seed, SITE_RNN0 + l).astype(np.float64).reshape(B, T, 2 * H) for l in range(Lyr - 1)]
    return {'rnn': rnn, 'fc0': m0, 'fc1': m1}


def _blocks(B, T, lengths):
    return [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), int(lengths[b])) for b in range(B)]


def step(P, x, y, variant, Lyr, lengths=None, masks=None):
    """One forward and, with a target, the backward.  x (B, T, F); y: class indices (clf) / values (reg) or None; lengths: None or B
    integers in [0, T].  Returns dict(out, z, ctx, alpha (B, T), and with y: loss, G {name: gradient of every live parameter})."""
    masks = masks or {}
    B, T, F = x.shape
    H = P['fc_audio.1.weight'].shape[0]
    clf = variant == 'clf'
    if clf:
        xin, ln_cache = R.layernorm_fwd(x, P['ln.weight'], P['ln.bias'])
    else:
        xin = x
    enc = bigru(xin, P, PX, Lyr, lengths=lengths, masks=masks.get('rnn'))
    Wa, ba = P['attention_layer.0.weight'], P['attention_layer.0.bias']
    ctx, alpha, att = np.zeros((B, H)), np.zeros((B, T)), []
    for rows, n in _blocks(B, T, lengths):
        if n == 0:
            att.append(None)                       # an empty row: ctx = 0, nothing to attend to
            continue
        c, cache = R.attention_fwd(enc['y'][rows, :n], enc['h_n'][:, rows], Wa, ba)
        ctx[rows] = c; alpha[rows, :n] = cache[5]; att.append(cache)
    z, head_cache = R.mlp_head_fwd(ctx, P['fc_audio.1.weight'], P['fc_audio.1.bias'], P['fc_audio.4.weight'], P['fc_audio.4.bias'],
                                   masks.get('fc0'), masks.get('fc1'))
    out = R.softmax(z, -1) if clf else np.maximum(z, 0.0)
    res = dict(out=out, z=z, ctx=ctx, alpha=alpha, h_n=enc['h_n'], y_top=enc['y'])
    if y is None:
        return res
    if clf:
        loss, dout = R.ce_on_probs(out, np.asarray(y).reshape(-1))
        dz = R.softmax_bwd(out, dout)
    else:
        loss, dout = R.l1_loss(out, np.asarray(y, np.float64).reshape(B, -1))
        dz = dout * (z > 0)
    dctx, dW1, db1, dW2, db2 = R.mlp_head_bwd(dz, P['fc_audio.1.weight'], P['fc_audio.4.weight'], head_cache)
    dseq, dhn = np.zeros_like(enc['y']), np.zeros_like(enc['h_n'])
    dWa, dba = np.zeros_like(Wa), np.zeros_like(ba)
    for (rows, n), cache in zip(_blocks(B, T, lengths), att):
        if cache is None:
            continue
        ds, dh, dw, db = R.attention_bwd(dctx[rows], Wa, cache)
        dseq[rows, :n] = ds; dhn[:, rows] = dh; dWa += dw; dba += db
    back = bigru(xin, P, PX, Lyr, lengths=lengths, dy=dseq, dhn=dhn, masks=masks.get('rnn'))
    G = dict(back['G'])
    G.update({'attention_layer.0.weight': dWa, 'attention_layer.0.bias': dba, 'fc_audio.1.weight': dW1, 'fc_audio.1.bias': db1,
              'fc_audio.4.weight': dW2, 'fc_audio.4.bias': db2})
    if clf:
        _, G['ln.weight'], G['ln.bias'] = R.layernorm_bwd(back['dx'], P['ln.weight'], ln_cache)
    res.update(loss=float(loss), G=G)
    return res


def train(P, x, y, variant, Lyr, nsteps, lr, seeds=None, p=0.0, lengths=None):
    """nsteps optimizer steps from P: AdamW with the scripts' two groups for clf (weight decay 1e-5, none on names containing 'ln'),
    Adam for reg.  seeds: the dropout seed of each step's forward (p > 0).  Returns (parameters after the last step, [loss per step],
    the first step's result)."""
    P = {k: np.array(v, np.float64) for k, v in P.items()}
    B, T, _ = x.shape
    H = P['fc_audio.1.weight'].shape[0]
    m = {k: np.zeros_like(v) for k, v in P.items()}; v = {k: np.zeros_like(w) for k, w in P.items()}
    losses, first = [], None
    for s in range(1, nsteps + 1):
        mk = masks(B, T, H, Lyr, p, seeds[s - 1]) if p > 0 else {}
        r = step(P, x, y, variant, Lyr, lengths=lengths, masks=mk)
        first = first or r
        losses.append(r['loss'])
        for k in P:
            wd = (0.0 if 'ln' in k else 1e-5) if variant == 'clf' else 0.0
            P[k], m[k], v[k] = R.adam_step(P[k], r['G'][k], m[k], v[k], s, lr, wd=wd, decoupled=variant == 'clf')
    return P, losses, first


def fold_ref(Ws, bs, gamma, beta, dWfs, dbfs):
    """The several-map fold in float64: [(Wf_k, bf_k)], [(dW_k, db_k)], dgamma, dbeta."""
    fwd = [(W * gamma, b + W @ beta) for W, b in zip(Ws, bs)]
    bwd = [(P * gamma + np.outer(q, beta), q.copy()) for P, q in zip(dWfs, dbfs)]
    dgamma = sum((P * W).sum(0) for P, W in zip(dWfs, Ws))
    dbeta = sum(W.T @ q for W, q in zip(Ws, dbfs))
    return fwd, bwd, dgamma, dbeta
