"""Yardstick of FusionNet.pretrained_feature with a bidirectional audio encoder and / or ragged pairs: a float64 composition of what the
suite already has, none of it restated --

    text:   ragged BiLSTM stack + attention (tests/varlen_ref.py)                      -> Dropout, Linear, ReLU, Dropout (fc_out.1)
    audio:  [LayerNorm (clf)] -> BiGRU -> attention  (tests/audio_bigru_ref.step up to ctx, the attention pair under its own name)
            or, unidirectional: [LayerNorm] -> GRU -> SUM over the row's own steps (varlen_ref.gru_ragged)
                                                                                       -> Dropout, Linear, ReLU, Dropout (fc_audio.1)

Every branch works row by row, so a dense batch is the ragged one with every length T.  Dropout is fed oracle.ref_numpy.dropout_mask at the
model's seeds and sites: the text stack at `seed`, the audio stack at `seed + 1`, site DEP_SITE_RNN0 + l over element (b, t, col) of layer l's
padded output; the text head at sites FC0 / FC1 and the audio head at FC2 / FC3, both at `seed` (tests/head_ref.masks).
"""
import numpy as np

import audio_bigru_ref
import head_ref
import varlen_ref as V
from oracle import ref_numpy as R

SITE_RNN0 = audio_bigru_ref.SITE_RNN0
TEXT_SITES, AUDIO_SITES = (1, 2), (3, 4)            # _lib.SITE_FC0 / FC1, SITE_FC2 / FC3


def key_list(variant, Lyr, bidirectional):
    """state_dict() keys of FusionNet in definition order."""
    def rnn(px, dirs):
        return [f'{px}.{n}_l{l}{sfx}' for l in range(Lyr) for sfx in ('', '_reverse')[:dirs] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    keys = ['attention_layer.0.weight', 'attention_layer.0.bias'] + rnn('lstm_net', 2) + ['fc_out.1.weight', 'fc_out.1.bias']
    keys += rnn('lstm_net_audio', 2 if bidirectional else 1)
    if bidirectional:
        keys += ['attention_layer_audio.0.weight', 'attention_layer_audio.0.bias']
    keys += ['fc_audio.1.weight', 'fc_audio.1.bias']
    if variant == 'clf':
        keys += ['ln.weight', 'ln.bias']
    return keys + ['modal_attn.weight', 'fc_final.0.weight']


def _rnn_masks(B, T, W, Lyr, p, seed):
    if not p > 0:
        return None
    return [R.dropout_mask(B * T * W, p, seed, SITE_RNN0 + l).astype(np.float64).reshape(B, T, W) for l in range(Lyr - 1)]


def _head(x, W1, b1, p, seed, sites):
    m0, m1 = head_ref.masks(x.shape[0], W1.shape[1], W1.shape[0], p, seed, sites, True)
    return head_ref.head_forward(x, W1, b1, None, None, m0, m1)[2]


def features(P, xa, xt, variant, Lyr, bidirectional, lengths=None, p=0.0, seed=0):
    """P: float64 state dict of the fusion model; xa (B, Ta, Fa), xt (B, Tt, Ft); lengths: None or (audio, text), each None or B integers.
    Returns (text_feature, audio_feature, audio context or pool)."""
    B, Ta, _ = xa.shape
    Tt = xt.shape[1]
    la, lt = lengths if lengths is not None else (None, None)
    la = np.full(B, Ta) if la is None else np.asarray(la)
    lt = np.full(B, Tt) if lt is None else np.asarray(lt)
    Ht, Ha = P['fc_out.1.weight'].shape[0], P['fc_audio.1.weight'].shape[0]
    enc = V.bilstm_ragged(xt, lt, P, 'lstm_net', Lyr, masks=_rnn_masks(B, Tt, 2 * Ht, Lyr, p, seed))
    ctx = V.attention_ragged(enc['y'], lt, enc['h_n'], P['attention_layer.0.weight'], P['attention_layer.0.bias'])['ctx']
    tf = _head(ctx, P['fc_out.1.weight'], P['fc_out.1.bias'], p, seed, TEXT_SITES)
    if bidirectional:
        Pa = {k: v for k, v in P.items() if k.startswith('lstm_net_audio.') or k.startswith('fc_audio.') or k.startswith('ln.')}
        Pa['attention_layer.0.weight'], Pa['attention_layer.0.bias'] = P['attention_layer_audio.0.weight'], P['attention_layer_audio.0.bias']
        Pa['fc_audio.4.weight'], Pa['fc_audio.4.bias'] = np.zeros((1, Ha)), np.zeros(1)          # (the classifier's last layer: not in the fusion model)
        mk = _rnn_masks(B, Ta, 2 * Ha, Lyr, p, seed + 1)
        pool = audio_bigru_ref.step(Pa, xa, None, variant, Lyr, lengths=la, masks={'rnn': mk} if mk else None)['ctx']
    else:
        xin = R.layernorm_fwd(xa, P['ln.weight'], P['ln.bias'])[0] if variant == 'clf' else xa
        pool = V.gru_ragged(xin, la, P, 'lstm_net_audio', Lyr, pool='sum', masks=_rnn_masks(B, Ta, Ha, Lyr, p, seed + 1))['pooled']
    af = _head(pool, P['fc_audio.1.weight'], P['fc_audio.1.bias'], p, seed, AUDIO_SITES)
    return tf, af, pool


def output(P, tf, af, variant):
    W = P['fc_final.0.weight']
    return R.fusion_clf_forward(W, tf, af) if variant == 'clf' else R.fusion_reg_forward(W, P['modal_attn.weight'], tf, af)


def loss_and_grad(P, tf, af, y, variant):
    W = P['fc_final.0.weight']
    return R.fusion_clf_loss(W, tf, af, np.asarray(y)) if variant == 'clf' else R.fusion_reg_loss(W, tf, af, np.asarray(y, np.float64))


def make_inputs(rng, B, Ta, Tt, Fa, Ft, ragged):
    """float32 inputs; ragged: lengths_mix drawn independently for each modality (T, 1, 0 and an interior length at B = 4), the padding zeros
    as pad_ragged leaves it."""
    xa = rng.standard_normal((B, Ta, Fa)).astype(np.float32)
    xt = (rng.standard_normal((B, Tt, Ft)) * 0.5).astype(np.float32)
    if not ragged:
        return xa, xt, None
    la, lt = V.lengths_mix(B, Ta, rng), V.lengths_mix(B, Tt, rng)
    xa[np.arange(Ta)[None, :] >= la[:, None]] = 0.0
    xt[np.arange(Tt)[None, :] >= lt[:, None]] = 0.0
    return xa, xt, (la.astype(np.int32), lt.astype(np.int32))
