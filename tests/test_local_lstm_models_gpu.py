"""The consumers of impl = 8 (the exchange-free LSTM forward): FusionNet(text_impl=8) runs its frozen text BiLSTM on it, TextBiLSTM
with config['eval_impl'] = 8 its eval() forwards.  Both load the default model's state dict and agree with it within the recurrent
paths' 1e-4; the default models launch what they launched before.  Small seeded models, text width 128, B = 6, T = 5."""
import re

import numpy as np
import pytest

import fusion_bi_ref as FR
from oracle import ref_numpy as R

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L, fuse_net, fuse_net_whole, models, nn

B, T, Ta, Fa, Ft, Ht, Ha, Lyr = 6, 5, 4, 8, 12, 128, 16, 2
SEED = 0x5DEECE66D
ATOL = 1e-4


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


class launched:
    """The recurrent sweeps enqueued inside the block, from the enqueue-order log."""

    def __enter__(self):
        L.order_log_enable(True)
        L.order_log_read(reset=True)
        return self

    def __exit__(self, *exc):
        log = L.order_log_read(reset=True)
        L.order_log_enable(False)
        self.sweeps = [re.sub(r'^\(|\)$', '', e[2:]) for e in log if e.startswith('K ') and re.search(r'(gru|lstm)2?_(fwd|bwd)_', e)]


def fusion_pair(variant, p=0.5):
    nc = 2 if variant == 'clf' else 1
    base = models.FusionNet(Ft, Ht, Lyr, p, nc, Ha, Fa, variant=variant, seed=3)
    local = models.FusionNet(Ft, Ht, Lyr, p, nc, Ha, Fa, variant=variant, seed=99, text_impl=8)
    assert list(local.state_dict().keys()) == list(base.state_dict().keys())
    local.load_state_dict(base.state_dict())
    assert base._rnn_t.impl == L.IMPL_AUTO and local._rnn_t.impl == L.IMPL_LOCAL_LSTM
    return base, local


def features(m, xa, xt, lengths, train, monkeypatch):
    m.train() if train else m.eval()
    monkeypatch.setattr(nn, 'next_dropout_seed', lambda: SEED)
    x = (torch.from_numpy(xa), torch.from_numpy(xt))
    with launched() as k:
        tf, af = m.pretrained_feature(x) if lengths is None else m.pretrained_feature(x, lengths=lengths)
    m.check_health()
    return tf, af, [s for s in k.sweeps if s.startswith('lstm_')]


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_fusion_features_agree_with_the_default_model(variant, train, ragged, monkeypatch):
    rng = np.random.default_rng(11 + 7 * train + 13 * ragged)
    xa = rng.standard_normal((B, Ta, Fa)).astype(np.float32); xt = rng.standard_normal((B, T, Ft)).astype(np.float32)
    lengths = None
    if ragged:
        la, lt = np.array([Ta, 1, 0, 2, Ta, 3]), np.array([T, 1, 0, 3, 2, T])
        xa[np.arange(Ta)[None, :] >= la[:, None]] = 0.0; xt[np.arange(T)[None, :] >= lt[:, None]] = 0.0
        lengths = (list(la), list(lt))
    base, local = fusion_pair(variant)
    tf0, af0, s0 = features(base, xa, xt, lengths, train, monkeypatch)
    tf8, af8, s8 = features(local, xa, xt, lengths, train, monkeypatch)
    rag = 'true' if ragged else 'false'
    assert s8 == ['lstm_fwd_local<true, %s>' % rag] * Lyr, s8
    assert s0 and all(s.startswith('lstm_fwd_cluster<') for s in s0), s0          # the default stays the cluster sweep
    assert local._rnn_t.last.desc.training == (L.RUN_DROPOUT_ONLY if train else L.RUN_EVAL)
    assert local._rnn_t.status_word() is None and len(local.status_words()) == len(base.status_words()) - 1      # no exchange buffer to watch
    P = {k: host(v) for k, v in base.state_dict().items()}
    tfr, afr, _ = FR.features(P, xa.astype(np.float64), xt.astype(np.float64), variant, Lyr, False, lengths, 0.5 if train else 0.0, SEED)
    e8, e0, ed = np.abs(host(tf8) - tfr).max(), np.abs(host(tf0) - tfr).max(), np.abs(host(tf8) - host(tf0)).max()
    print('%s %s %s: text feature, impl 8 vs oracle %.3g, default vs oracle %.3g, impl 8 vs default %.3g' % (
        variant, 'train' if train else 'eval', 'ragged' if ragged else 'dense', e8, e0, ed))
    assert np.isfinite(host(tf8)).all() and np.abs(tfr).max() > 1e-2
    assert ed < ATOL and e8 < ATOL
    assert torch.equal(af8, af0)                 # the audio branch is the same code on the same seeds


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_one_fusion_training_step(variant, monkeypatch):
    """fc_final.0.weight after one MyLoss + Adam step on the impl = 8 features: within 1e-6 (the bound tests/test_fusion_bi_gpu.py holds
    its step to) of the oracle's step on those features, and of the default model's step."""
    rng = np.random.default_rng(5)
    xa = rng.standard_normal((B, Ta, Fa)).astype(np.float32); xt = rng.standard_normal((B, T, Ft)).astype(np.float32)
    y = list(rng.integers(0, 2, B)) if variant == 'clf' else list(rng.uniform(0, 20, B).astype(np.float32))
    base, local = fusion_pair(variant)
    lr, after = 1e-3, []
    for m in (base, local):
        P = {k: host(v) for k, v in m.state_dict().items()}
        tf, af, _ = features(m, xa, xt, None, True, monkeypatch)
        opt = nn.Adam(m.parameters(), lr=lr)
        loss = models.MyLoss(variant)(tf, af, y, m)
        loss.backward(); opt.step()
        lref, gW = FR.loss_and_grad(P, host(tf), host(af), y, variant)
        W0 = P['fc_final.0.weight']
        Wn, _, _ = R.adam_step(W0, gW, np.zeros_like(W0), np.zeros_like(W0), 1, lr)
        now = {k: host(v) for k, v in m.state_dict().items()}
        print('%s impl %d: loss %.6f (oracle %.6f), fc_final vs the oracle step %.3g' % (variant, m._rnn_t.impl, loss.item(), lref,
                                                                                       np.abs(now['fc_final.0.weight'] - Wn).max()))
        assert abs(loss.item() - lref) < 1e-5 * max(1.0, abs(lref))
        assert np.abs(now['fc_final.0.weight'] - Wn).max() < 1e-6
        assert np.abs(now['fc_final.0.weight'] - W0).max() > 1e-4
        assert all(np.array_equal(now[k], P[k]) for k in P if k != 'fc_final.0.weight')
        after.append(now['fc_final.0.weight'])
    d = np.abs(after[1] - after[0]).max()
    print('%s: fc_final after the step, impl 8 vs default %.3g' % (variant, d))
    assert d < 1e-6


def text_config(**kw):
    c = dict(num_classes=2, dropout=0.5, rnn_layers=Lyr, embedding_size=Ft, batch_size=B, epochs=1, learning_rate=1e-3, hidden_dims=Ht,
             bidirectional=True, cuda=False)
    c.update(kw)
    return c


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_text_model_eval_impl(variant, ragged, monkeypatch):
    cfg = text_config(num_classes=2 if variant == 'clf' else 1)
    base = models.TextBiLSTM(cfg, variant=variant, seed=4)
    local = models.TextBiLSTM(dict(cfg, eval_impl=8), variant=variant, seed=77)
    local.load_state_dict(base.state_dict())
    rng = np.random.default_rng(21 + ragged)
    x = rng.standard_normal((B, T, Ft)).astype(np.float32)
    lengths = None
    if ragged:
        lengths = np.array([T, 1, 3, 2, T, 4])
        x[np.arange(T)[None, :] >= lengths[:, None]] = 0.0
    monkeypatch.setattr(nn, 'next_dropout_seed', lambda: SEED)
    outs, sweeps = {}, {}
    for name, m in (('base', base), ('local', local)):
        for mode in ('eval', 'train'):
            m.eval() if mode == 'eval' else m.train()
            with launched() as k:
                out = m(x) if lengths is None else m(x, lengths=list(lengths))
            m.check_health()
            outs[name, mode], sweeps[name, mode] = host(out.data), k.sweeps
    rag = 'true' if ragged else 'false'
    assert sweeps['local', 'eval'] == ['lstm_fwd_local<true, %s>' % rag] * Lyr, sweeps['local', 'eval']
    assert all(s.startswith('lstm_fwd_cluster<') for s in sweeps['base', 'eval']) and sweeps['base', 'eval']
    # train() mode is untouched: the same sweeps as the default model, and its bits
    assert sweeps['local', 'train'] == sweeps['base', 'train'] and not any('lstm_fwd_local' in s for s in sweeps['local', 'train'])
    assert np.array_equal(outs['local', 'train'], outs['base', 'train'])
    d = np.abs(outs['local', 'eval'] - outs['base', 'eval']).max()
    print('text %s %s: eval output, eval_impl 8 vs default %.3g' % (variant, 'ragged' if ragged else 'dense', d))
    assert np.isfinite(outs['local', 'eval']).all() and d < ATOL
    # a backward cannot follow the impl = 8 forward ...
    local.eval()
    out = local(x) if lengths is None else local(x, lengths=list(lengths))
    with pytest.raises(L.DepError, match='eval_impl'):
        local.backward(torch.zeros_like(out.data))
    # ... and follows a train() forward as before
    local.train()
    crit = nn.CrossEntropyLoss() if variant == 'clf' else None
    if crit is not None:
        loss = crit(local(x) if lengths is None else local(x, lengths=list(lengths)), list(rng.integers(0, 2, B)))
        loss.backward()
        g = dict(local.named_parameters())['lstm_net.weight_hh_l0'].grad
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_bad_choices_raise():
    for bad in (0, 3, 4, 9, '8', True):
        with pytest.raises(L.DepError, match='text_impl'):
            models.FusionNet(Ft, Ht, Lyr, 0.5, 2, Ha, Fa, text_impl=bad)
        with pytest.raises(L.DepError, match='eval_impl'):
            models.TextBiLSTM(text_config(eval_impl=bad))
    with pytest.raises(L.DepError, match='impl = 8'):          # the descriptor exists at H = 128 only
        models.FusionNet(Ft, 64, Lyr, 0.5, 2, Ha, Fa, text_impl=8)
    with pytest.raises(L.DepError, match='impl = 8'):
        models.TextBiLSTM(text_config(hidden_dims=64, eval_impl=8))
    for script in (fuse_net, fuse_net_whole):                    # config['text_impl'] reaches the model
        old = dict(script.config)
        try:
            script.config.update(text_embed_size=Ft, text_hidden_dims=Ht, audio_embed_size=Fa, audio_hidden_dims=Ha, text_impl=8)
            assert script.build(seed=1)._rnn_t.impl == L.IMPL_LOCAL_LSTM
            script.config['text_impl'] = 5
            with pytest.raises(L.DepError, match='text_impl'):
                script.build(seed=1)
        finally:
            script.config.clear(); script.config.update(old)
