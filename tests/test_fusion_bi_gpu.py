"""FusionNet with a bidirectional audio encoder (audio_bidirectional=True) and ragged pairs (pretrained_feature(x, lengths=(audio, text)))
against tests/fusion_bi_ref.py, at B = 3 dense / B = 4 ragged (lengths T, 1, 0 and an interior one, drawn for each modality on its own),
Ta = 5, Tt = 4, Fa = Ft = 8, Ht = 16, L = 2.  Ha runs 16 (the tile-MFMA sweeps), 64 (impl 7) and 512 (impl 7 and the H = 512 attention
instances).  Bounds: those tests/test_fullsize_gpu.py holds the unidirectional fusion to -- 1e-4 absolute on the features, 1e-5 on the output,
relerr 1e-4 on the gradient of fc_final.  In train mode (p = 0.5) the oracle draws the masks of the model's seeds and sites."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import fusion_bi_ref as FR
from oracle import ref_numpy as R

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_fusion_parent_bits as rec  # noqa: E402

if torch.cuda.is_available():
    from icassp2022_depression_amd import _common, _lib as L, fuse_net_whole, models, nn

Ta, Tt, Fa, Ft, Ht, Lyr = 5, 4, 8, 8, 16, 2
SEED = 0x5DEECE66D


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _model(variant, Ha, bi, p=0.5, seed=3):
    m = models.FusionNet(Ft, Ht, Lyr, p, 2 if variant == 'clf' else 1, Ha, Fa, variant=variant, seed=seed, audio_bidirectional=bi)
    if variant == 'clf':                         # a LayerNorm affine off its defaults
        rng = np.random.default_rng(1)
        sd = m.state_dict()
        sd['ln.weight'].copy_(torch.from_numpy((1.0 + 0.3 * rng.standard_normal(Fa)).astype(np.float32)))
        sd['ln.bias'].copy_(torch.from_numpy((0.3 * rng.standard_normal(Fa)).astype(np.float32)))
    return m


def _P(m):
    return {k: host(v) for k, v in m.state_dict().items()}


def _features(m, xa, xt, lengths, train, monkeypatch):
    m.train() if train else m.eval()
    monkeypatch.setattr(nn, 'next_dropout_seed', lambda: SEED)
    x = (torch.from_numpy(xa), torch.from_numpy(xt))
    return m.pretrained_feature(x) if lengths is None else m.pretrained_feature(x, lengths=lengths)


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('Ha', [16, 64, 512])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_features_output_and_head_step_against_the_oracle(variant, Ha, train, ragged, monkeypatch):
    B = 4 if ragged else 3
    rng = np.random.default_rng(Ha + 7 * train + 13 * ragged)
    xa, xt, lengths = FR.make_inputs(rng, B, Ta, Tt, Fa, Ft, ragged)
    m = _model(variant, Ha, True)
    assert m._rnn_a.impl == (L.IMPL_TILE if Ha == 16 else L.IMPL_CLUSTER_BIGRU_TRAIN)
    L.instance_log_read(reset=True)
    tf, af = _features(m, xa, xt, lengths, train, monkeypatch)
    m.check_health()
    log = L.instance_log_read(reset=True)
    assert m._rnn_a.last.desc.training == (L.RUN_DROPOUT_ONLY if train else L.RUN_EVAL) == m._rnn_t.last.desc.training
    if Ha == 512:
        assert any('attn_fwd2_kernel<128' in s for s in log), log
    P = _P(m)
    p = 0.5 if train else 0.0
    tfr, afr, ctxr = FR.features(P, xa.astype(np.float64), xt.astype(np.float64), variant, Lyr, True, lengths, p, SEED)
    print('%s Ha=%d %s %s: tf %.3g af %.3g' % (variant, Ha, 'train' if train else 'eval', 'ragged' if ragged else 'dense',
                                                 np.abs(host(tf) - tfr).max(), np.abs(host(af) - afr).max()))
    assert np.abs(host(tf) - tfr).max() < 1e-4 and np.abs(host(af) - afr).max() < 1e-4
    if ragged:                                   # a row of length 0: the head on the zero vector
        for feat, W, b, ln, sites in ((tf, 'fc_out.1', None, lengths[1], FR.TEXT_SITES), (af, 'fc_audio.1', None, lengths[0], FR.AUDIO_SITES)):
            empty = np.asarray(ln) == 0
            assert empty.any()
            z = FR._head(np.zeros((B, P[W + '.weight'].shape[1])), P[W + '.weight'], P[W + '.bias'], p, SEED, sites)
            assert np.abs(host(feat)[empty] - z[empty]).max() < 1e-6
    out = m(torch.cat((tf, af), dim=1))
    assert np.abs(host(out.data) - FR.output(P, host(tf), host(af), variant)).max() < 1e-5
    # one MyLoss + Adam step on fc_final, on the device's features
    y = list(rng.integers(0, 2, B)) if variant == 'clf' else list(rng.uniform(0, 20, B).astype(np.float32))
    m.train()
    lr = 1e-3
    opt = nn.Adam(m.parameters(), lr=lr)
    W0 = P['fc_final.0.weight'].copy()
    loss = models.MyLoss(variant)(tf, af, y, m)
    loss.backward(); opt.step()
    lref, gW = FR.loss_and_grad(P, host(tf), host(af), y, variant)
    assert abs(loss.item() - lref) < 1e-5 * max(1.0, abs(lref))
    assert relerr(host(dict(m.named_parameters())['fc_final.0.weight'].grad), gW) < 1e-4
    Wn, _, _ = R.adam_step(W0, gW, np.zeros_like(W0), np.zeros_like(W0), 1, lr)
    after = _P(m)
    assert np.abs(after['fc_final.0.weight'] - Wn).max() < 1e-6
    assert all(np.array_equal(after[k], P[k]) for k in P if k != 'fc_final.0.weight')


@pytest.mark.parametrize('bi', [True, False], ids=['bidirectional', 'unidirectional'])
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_ragged_unidirectional_and_row_by_row(variant, train, bi, monkeypatch):
    """The ragged call against the oracle for the unidirectional branch too (SUM over each row's own steps); a ragged batch in eval equals, row
    by row, the dense call on that row alone; a ragged call with every length T is bit-equal to the dense call, in both run modes."""
    Ha = 64
    rng = np.random.default_rng(41 + train)
    xa, xt, lengths = FR.make_inputs(rng, 4, Ta, Tt, Fa, Ft, True)
    m = _model(variant, Ha, bi)
    tf, af = _features(m, xa, xt, lengths, train, monkeypatch)
    m.check_health()
    P = _P(m)
    tfr, afr, _ = FR.features(P, xa.astype(np.float64), xt.astype(np.float64), variant, Lyr, bi, lengths, 0.5 if train else 0.0, SEED)
    assert np.abs(host(tf) - tfr).max() < 1e-4 and np.abs(host(af) - afr).max() < 1e-4
    full = (np.full(4, Ta, np.int32), torch.full((4,), Tt, dtype=torch.int32, device=m.device))         # a host sequence and a device vector
    d_tf, d_af = _features(m, xa, xt, None, train, monkeypatch)
    r_tf, r_af = _features(m, xa, xt, full, train, monkeypatch)
    assert torch.equal(d_tf, r_tf) and torch.equal(d_af, r_af)
    if not train:
        for b in range(4):
            na, nt = int(lengths[0][b]), int(lengths[1][b])
            if na == 0 or nt == 0:
                continue                         # (a dense call has no rows of length 0; the oracle above covers them)
            one_tf, one_af = _features(m, np.ascontiguousarray(xa[b:b + 1, :na]), np.ascontiguousarray(xt[b:b + 1, :nt]), None, False, monkeypatch)
            assert np.abs(host(one_tf) - host(tf)[b]).max() < 1e-4 and np.abs(host(one_af) - host(af)[b]).max() < 1e-4


@pytest.mark.parametrize('Ha', [16, 64, 512])
def test_reg_audio_feature_is_the_audio_models_own_encode(Ha, monkeypatch):
    """reg, eval: no LayerNorm, so the fusion branch enqueues the launches of AudioGRU.encode on the same operands -- af is bit-equal to
    _mlp_feature of the transplanted model's own context."""
    from icassp2022_depression_amd import fuse_net
    cfg = dict(num_classes=1, learning_rate=1e-3, dropout=0.5, hidden_dims=Ha, rnn_layers=Lyr, embedding_size=Fa, bidirectional=True)
    am = models.AudioGRU(cfg, variant='reg', seed=8)
    tm = models.TextBiLSTM(dict(cfg, hidden_dims=Ht, embedding_size=Ft, bidirectional=True), variant='reg', seed=9)
    m = _model('reg', Ha, True)
    fuse_net.transplant(m, tm.state_dict(), am.state_dict())
    rng = np.random.default_rng(Ha)
    xa, xt, lengths = FR.make_inputs(rng, 4, Ta, Tt, Fa, Ft, True)
    for ln in (None, lengths):
        tf, af = _features(m, xa, xt, ln, False, monkeypatch)
        am.eval()
        la = None if ln is None else torch.from_numpy(ln[0]).to(am.device)
        ctx, _ = am.encode(torch.from_numpy(xa).to(am.device), False, 0, la)
        P = am._params
        want = models._mlp_feature(ctx, P['fc_audio.1.weight'].data, P['fc_audio.1.bias'].data, 0.0, 0, (L.SITE_FC2, L.SITE_FC3))
        assert torch.equal(af, want)


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_flag_off_repeats_the_parents_feature_bits(variant):
    """sha256 of both features, eval and train, recorded on an MI355X from the commit before the flag (tests/golden/make_fusion_parent_bits.py)."""
    want = json.load(open(os.path.join(HERE, 'golden', 'fusion_parent_bits.json')))[variant]
    assert rec.feature_bits(models, nn, variant) == want


def test_refusals_on_the_device():
    m = _model('clf', 64, True)
    x = (torch.zeros(3, Ta, Fa), torch.zeros(3, Tt, Ft))
    L.instance_log_read(reset=True)
    for bad in (([5, 5], None), (None, torch.zeros(3, dtype=torch.float32, device=m.device)), (torch.zeros(4, dtype=torch.int32, device=m.device), None)):
        with pytest.raises(L.DepError, match='expected 3 integers'):
            m.pretrained_feature(x, lengths=bad)
    assert not L.instance_log_read(reset=True)   # before any launch
    mode = L.get_gemm_mode()
    try:                                         # GEMM modes 2 / 3 take no ragged call on impl 7: the library's own message
        L.set_gemm_mode(2)
        with pytest.raises(L.DepError):
            m.pretrained_feature(x, lengths=([5, 1, 0], [4, 1, 0]))
    finally:
        L.set_gemm_mode(mode)


def test_scripts_train_and_evaluate_on_a_ragged_corpus():
    """fuse_net_whole.train + evaluate, two epochs, nine ragged pairs, audio_bidirectional and ragged set: finite loss, clean health words, only
    fc_final.0.weight changes."""
    m = fuse_net_whole
    saved = dict(m.config)
    old = (m.fuse_features, m.fuse_targets, m.model, m.optimizer, m.criterion, m.max_f1)
    rng = np.random.default_rng(17)
    try:
        m.config.update(audio_embed_size=Fa, text_embed_size=Ft, audio_hidden_dims=64, text_hidden_dims=Ht, dropout=0.3, batch_size=4,
                        learning_rate=1e-2, audio_bidirectional=True, ragged=True)
        _common.invalidate_device_features()
        m.fuse_features = [[rng.standard_normal((int(rng.integers(0 if i else Ta, Ta + 1)), Fa)).astype(np.float32),
                            rng.standard_normal((int(rng.integers(1, Tt + 1)), Ft)).astype(np.float32)] for i in range(9)]
        m.fuse_targets = np.array([0, 1, 0, 1, 1, 0, 0, 1, 0])
        model = m.build(seed=2)
        m.max_f1 = 2.0                           # (no F1 beats it: evaluate() writes no checkpoint)
        assert model.audio_bidirectional
        before = _P(model)
        buf = io.StringIO()
        with redirect_stdout(buf):
            for ep in (1, 2):
                m.train(ep, [0, 1, 2, 3, 4, 5])
                total = m.evaluate(model, [6, 7, 8], 1, [0, 1, 2, 3, 4, 5])
        assert np.isfinite(total)
        model.check_health()
        assert all(w == 0 for w in model.status_words()) and all(w == 0 for w in model.fallback_words())
        after = _P(model)
        assert not np.array_equal(after['fc_final.0.weight'], before['fc_final.0.weight'])
        assert all(np.array_equal(after[k], before[k]) for k in before if k != 'fc_final.0.weight')
        assert all(np.isfinite(v).all() for v in after.values())
    finally:
        m.config.clear(); m.config.update(saved)
        m.fuse_features, m.fuse_targets, m.model, m.optimizer, m.criterion, m.max_f1 = old
        _common.invalidate_device_features()
