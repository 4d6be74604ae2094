"""Host logic of the bidirectional audio branch of FusionNet and of ragged pairs (no device): parameter names and flat layout, the transplant's
key mapping and refusals, PairFeeder(ragged=True).  The models are built with their flat buffers in host memory, as
tests/test_audio_bigru_cpu.py builds them."""
import json
import os
import sys

import numpy as np
import pytest

import fusion_bi_ref as FR

torch = pytest.importorskip('torch')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_fusion_parent_bits as rec  # noqa: E402


@pytest.fixture()
def host(monkeypatch):
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _common, _lib, fuse_net, fuse_net_whole, models, nn
    monkeypatch.setattr(nn, '_device', lambda: torch.device('cpu'))
    return dict(common=_common, L=_lib, reg=fuse_net, clf=fuse_net_whole, models=models)


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_default_layout_is_the_parents(host, variant):
    """Names, shapes, order and flat offsets with the flag off: the fixture recorded from the commit before the flag
    (tests/golden/make_fusion_parent_bits.py layout)."""
    want = json.load(open(os.path.join(HERE, 'golden', 'fusion_layout_parent.json')))[variant]
    assert rec.layout(rec.build(host['models'], variant)) == want
    assert rec.layout(rec.build(host['models'], variant, audio_bidirectional=False)) == want
    assert want['names'] == FR.key_list(variant, 2, False)


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_bidirectional_keys_shapes_and_sweeps(host, variant):
    L, models = host['L'], host['models']
    m = rec.build(models, variant, audio_bidirectional=True)
    sd = m.state_dict()
    assert list(sd) == FR.key_list(variant, 2, True)
    i = list(sd).index('attention_layer_audio.0.weight')
    assert list(sd)[i - 1] == 'lstm_net_audio.bias_hh_l1_reverse' and list(sd)[i + 1] == 'attention_layer_audio.0.bias'       # directly behind the stack
    Ha, Fa = rec.SHAPE['Ha'], rec.SHAPE['Fa']
    assert tuple(sd['attention_layer_audio.0.weight'].shape) == (Ha, Ha) and tuple(sd['attention_layer_audio.0.bias'].shape) == (Ha,)
    assert tuple(sd['lstm_net_audio.weight_ih_l0_reverse'].shape) == (3 * Ha, Fa) and tuple(sd['lstm_net_audio.weight_ih_l1'].shape) == (3 * Ha, 2 * Ha)
    assert [k for k, p in m._params.items() if p.live] == ['fc_final.0.weight']              # everything else is frozen
    assert m._rnn_a.args[4] == 2 and m._rnn_a.args[6] == L.POOL_NONE and m._rnn_a.impl == L.IMPL_TILE == m._bi_impl
    s = rec.SHAPE
    mk = lambda Ha: models.FusionNet(s['Ft'], s['Ht'], 2, 0.5, 2, Ha, s['Fa'], variant=variant, seed=1, audio_bidirectional=True)
    for H in (64, 128, 256, 512):                    # the rule is AudioGRU._bidirectional_impl's
        assert mk(H)._rnn_a.impl == L.IMPL_CLUSTER_BIGRU_TRAIN == models.AudioGRU._bidirectional_impl(s['Fa'], H, 2)
    for H in (32, 48, 96, 192):
        assert mk(H)._rnn_a.impl == L.IMPL_TILE
    with pytest.raises(L.DepError, match=r'64, 128, 256 and 512.*16, 32, 48, 96 and 192'):
        mk(40)
    uni = rec.build(models, variant)
    assert uni._rnn_a.impl == 0 and uni._rnn_a.args[4] == 1 and uni._rnn_a.args[6] == L.POOL_SUM


def _audio_checkpoint(models, variant, bidirectional, seed=4):
    s = rec.SHAPE
    cfg = dict(num_classes=2 if variant == 'clf' else 1, learning_rate=1e-3, dropout=0.5, hidden_dims=s['Ha'], rnn_layers=2, embedding_size=s['Fa'],
               bidirectional=bidirectional)
    return {k: v.clone() for k, v in models.AudioGRU(cfg, variant=variant, seed=seed).state_dict().items()}


def _text_checkpoint(models, variant, seed=6):
    s = rec.SHAPE
    cfg = dict(num_classes=2 if variant == 'clf' else 1, learning_rate=1e-3, dropout=0.5, hidden_dims=s['Ht'], rnn_layers=2, embedding_size=s['Ft'])
    return {k: v.clone() for k, v in models.TextBiLSTM(cfg, variant=variant, seed=seed, fc_idx=(1, 4)).state_dict().items()}


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_transplant_maps_and_refuses(host, variant):
    L, models, script = host['L'], host['models'], host[variant]
    tsd = _text_checkpoint(models, variant)
    asd_bi, asd_uni = _audio_checkpoint(models, variant, True), _audio_checkpoint(models, variant, False)
    m = rec.build(models, variant, audio_bidirectional=True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    script.transplant(m, tsd, asd_bi)
    sd = m.state_dict()
    for k in sd:
        if k.startswith('lstm_net_audio.') or k.startswith('fc_audio.1') or k.startswith('ln.'):
            assert torch.equal(sd[k], asd_bi[k]), k
        elif k.startswith('attention_layer_audio.0.'):
            assert torch.equal(sd[k], asd_bi[k.replace('attention_layer_audio', 'attention_layer')]), k
        elif k.startswith('attention_layer.0.') or k.startswith('lstm_net.') or k.startswith('fc_out.1'):
            assert torch.equal(sd[k], tsd[k]), k                                             # the TEXT attention keeps the text checkpoint's
        else:
            assert k in ('modal_attn.weight', 'fc_final.0.weight') and torch.equal(sd[k], before[k]), k
    assert not torch.equal(sd['attention_layer.0.weight'], sd['attention_layer_audio.0.weight'])        # two attentions, two checkpoints
    with pytest.raises(L.DepError, match='lstm_net_audio.weight_ih_l0_reverse'):             # the first missing key, by name
        script.transplant(rec.build(models, variant, audio_bidirectional=True), tsd, asd_uni)
    with pytest.raises(L.DepError, match='lstm_net_audio.weight_ih_l0_reverse'):
        script.transplant(rec.build(models, variant), tsd, asd_bi)
    no_att = {k: v for k, v in asd_bi.items() if k != 'attention_layer.0.bias'}
    with pytest.raises(L.DepError, match='attention_layer.0.bias'):
        script.transplant(rec.build(models, variant, audio_bidirectional=True), tsd, no_att)
    uni = rec.build(models, variant)                                                          # flag off: the listed keys, as before
    script.transplant(uni, tsd, asd_uni)
    assert torch.equal(uni.state_dict()['lstm_net_audio.weight_hh_l1'], asd_uni['lstm_net_audio.weight_hh_l1'])
    assert script.config['audio_bidirectional'] is False


def _ragged_pairs(rng, n, Fa=3, Ft=2):
    return [[rng.standard_normal((int(rng.integers(0, 5)) if i else 4, Fa)).astype(np.float32),
             rng.standard_normal((int(rng.integers(1, 4)), Ft)).astype(np.float32)] for i in range(n)]


def test_pair_feeder_ragged_pads_and_slices_lengths(host):
    C = host['common']
    C.invalidate_device_features()
    rng = np.random.default_rng(2)
    pairs = _ragged_pairs(rng, 7)
    idxs = [5, 0, 3, 3, 6]
    feed = C.PairFeeder(pairs, idxs, torch.device('cpu'), ragged=True)
    la = np.array([len(p[0]) for p in pairs]); lt = np.array([len(p[1]) for p in pairs])
    assert tuple(feed.Xa.shape) == (7, la.max(), 3) and tuple(feed.Xt.shape) == (7, lt.max(), 2)
    for i, (a, t) in enumerate(pairs):
        assert np.array_equal(feed.Xa[i, :len(a)].numpy(), a) and not feed.Xa[i, len(a):].any()
        assert np.array_equal(feed.Xt[i, :len(t)].numpy(), t) and not feed.Xt[i, len(t):].any()
    a_len, t_len = feed.lengths_rows(1, 4)
    assert a_len.dtype == torch.int32 and t_len.dtype == torch.int32
    assert a_len.tolist() == la[[0, 3, 3]].tolist() and t_len.tolist() == lt[[0, 3, 3]].tolist()
    assert a_len.data_ptr() == feed.len_dev[0].data_ptr() + 4 and a_len._base is feed.len_dev[0]          # views: no gather, no copy
    assert feed.idx_dev.tolist() == idxs
    again = C.PairFeeder(pairs, [1, 2], torch.device('cpu'), ragged=True)                                  # the cached padded arrays
    assert again.Xa is feed.Xa and again.lengths_rows(0, 2)[0].tolist() == la[[1, 2]].tolist()
    pairs[2][0] = np.zeros((6, 3), np.float32)                                                             # a length changed: the key covers it
    fresh = C.PairFeeder(pairs, [2], torch.device('cpu'), ragged=True)
    assert fresh.Xa is not feed.Xa and fresh.Xa.shape[1] == 6 and fresh.lengths_rows(0, 1)[0].tolist() == [6]
    with pytest.raises(IndexError):
        C.PairFeeder(pairs, [7], torch.device('cpu'), ragged=True)
    C.invalidate_device_features()


def test_default_pair_feeder_is_unchanged(host):
    C = host['common']
    C.invalidate_device_features()
    rng = np.random.default_rng(3)
    pairs = _ragged_pairs(rng, 5)
    feed = C.PairFeeder(pairs, [4, 1, 2], torch.device('cpu'))             # ragged items, default feeder: the list-slice fallback
    assert not feed.ok and feed.lengths_rows(0, 2) is None
    rows = feed.rows(1, 3)
    assert isinstance(rows, list) and rows[0] is pairs[1] and rows[1] is pairs[2]
    dense = [[rng.standard_normal((3, 4)).astype(np.float32), rng.standard_normal((2, 5)).astype(np.float32)] for _ in range(4)]
    feed = C.PairFeeder(dense, [0, 2], torch.device('cpu'))
    assert feed.ok and feed.lengths_rows(0, 2) is None and tuple(feed.Xa.shape) == (4, 3, 4) and tuple(feed.Xt.shape) == (4, 2, 5)
    C.invalidate_device_features()


def test_lengths_are_refused_before_any_launch(host):
    """A lengths member of the wrong size or dtype, or a lengths that is no pair: raised while the inputs are still being looked at (the host
    model has no device to launch on)."""
    L, models = host['L'], host['models']
    m = rec.build(models, 'clf', audio_bidirectional=True)
    x = (np.zeros((3, 5, 8), np.float32), np.zeros((3, 4, 8), np.float32))
    for bad in (([5, 5], None), (None, [4, 4, 4, 4]), ([5.0, 1.0, 0.0], None), (None, np.zeros((3, 1), np.int32))):
        with pytest.raises(L.DepError, match='expected 3 integers'):
            m.pretrained_feature(x, lengths=bad)
    with pytest.raises(L.DepError, match='pair'):
        m.pretrained_feature(x, lengths=[5, 5, 5])
