"""The bidirectional audio encoder, the parts that need no GPU: the yardstick of the GPU tests (tests/audio_bigru_ref.py) against
stock torch in float64 with autograd, the identities of the two-piece LayerNorm fold, and the model's parameter list, flat layout and
data-parallel plan (built on the host: the flat buffers of nn.Module need no kernel)."""
import numpy as np
import pytest

import audio_bigru_ref as ref

torch = pytest.importorskip('torch')


class TorchAudioBiGRU(torch.nn.Module):
    """The stock module tree: the reference audio class's members in its definition order, the GRU built with bidirectional=True,
    and the forward this project gives the flag (ln -> BiGRU -> attention over (output, h_n) -> fc_audio)."""

    def __init__(self, variant, F, H, Lyr, C):
        super().__init__()
        nn = torch.nn
        self.attention_layer = nn.Sequential(nn.Linear(H, H), nn.ReLU())
        self.lstm_net_audio = nn.GRU(F, H, num_layers=Lyr, dropout=0.0, batch_first=True, bidirectional=True)
        if variant == 'clf':
            self.ln = nn.LayerNorm(F)
        else:
            self.bn = nn.BatchNorm1d(3)
        self.fc_audio = nn.Sequential(nn.Dropout(0.0), nn.Linear(H, H), nn.ReLU(), nn.Dropout(0.0), nn.Linear(H, C),
                                      nn.Softmax(dim=1) if variant == 'clf' else nn.ReLU())
        self.variant = variant

    def attend(self, out, h_n):
        """The yardstick's attention in torch's words: halves of the output summed, the final states summed into the query."""
        H = out.shape[-1] // 2
        h = out[..., :H] + out[..., H:]
        q = self.attention_layer(h_n.sum(0))                                # (B, H)
        alpha = torch.softmax(torch.einsum('bj,btj->bt', q, torch.tanh(h)), -1)
        return torch.einsum('bt,btj->bj', alpha, h), alpha

    def forward(self, x):
        if self.variant == 'clf':
            x = self.ln(x)
        out, h_n = self.lstm_net_audio(x)
        ctx, alpha = self.attend(out, h_n)
        return self.fc_audio(ctx), alpha


@pytest.mark.parametrize('Lyr', [1, 2])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_yardstick_equals_torch_autograd(variant, Lyr):
    B, T, F, H = 3, 5, 6, 4
    C = 2 if variant == 'clf' else 1
    rng = np.random.default_rng(11 + Lyr + (variant == 'reg') * 10)
    P = ref.make_params(rng, F, H, Lyr, C, variant)
    x = rng.standard_normal((B, T, F))
    y = rng.integers(0, C, B) if variant == 'clf' else rng.uniform(0.0, 2.0, (B, 1))
    net = TorchAudioBiGRU(variant, F, H, Lyr, C).double()
    sd = net.state_dict()
    assert [k for k in sd if not k.startswith('bn.')] == ref.live_names(variant, Lyr)
    net.load_state_dict({k: torch.from_numpy(P[k]) if k in P else v for k, v in sd.items()})
    out_t, alpha_t = net(torch.from_numpy(x))
    if variant == 'clf':
        loss_t = torch.nn.CrossEntropyLoss()(out_t, torch.from_numpy(y))    # on the Softmax output, as the scripts do
    else:
        loss_t = torch.nn.L1Loss()(out_t, torch.from_numpy(y))
    loss_t.backward()
    r = ref.step(P, x, y, variant, Lyr)
    assert np.abs(r['out'] - out_t.detach().numpy()).max() < 1e-9
    assert np.abs(r['alpha'] - alpha_t.detach().numpy()).max() < 1e-9
    assert abs(r['loss'] - float(loss_t.detach())) < 1e-9
    named = dict(net.named_parameters())
    assert set(r['G']) == set(ref.live_names(variant, Lyr))
    for k, g in r['G'].items():
        gt = named[k].grad.numpy()
        assert np.abs(gt).max() > 0, k
        assert np.abs(g - gt).max() <= 1e-9 * max(1.0, np.abs(gt).max()), k
    # the ragged builder with full lengths is the dense builder
    rr = ref.step(P, x, y, variant, Lyr, lengths=np.full(B, T))
    assert np.abs(rr['out'] - r['out']).max() < 1e-12 and abs(rr['loss'] - r['loss']) < 1e-12
    for k in r['G']:
        assert np.abs(rr['G'][k] - r['G'][k]).max() < 1e-11, k


def test_ragged_yardstick_rows_stand_alone():
    """Row b of the ragged form is the model on x[b:b+1, :len_b]; an empty row has ctx = 0 and gives the encoder no gradient."""
    B, T, F, H, Lyr = 4, 5, 6, 4, 2
    rng = np.random.default_rng(5)
    P = ref.make_params(rng, F, H, Lyr, 1, 'reg')
    x = rng.standard_normal((B, T, F))
    lengths = np.array([T, 1, 0, 3])
    r = ref.step(P, x, None, 'reg', Lyr, lengths=lengths)
    for b, n in enumerate(lengths):
        if n == 0:
            assert not r['ctx'][b].any() and not r['alpha'][b].any()
            continue
        one = ref.step(P, x[b:b + 1, :n], None, 'reg', Lyr)
        assert np.abs(one['out'] - r['out'][b:b + 1]).max() < 1e-13
        assert abs(r['alpha'][b, :n].sum() - 1.0) < 1e-12 and not r['alpha'][b, n:].any()


@pytest.mark.parametrize('npieces', [1, 2])
def test_fold_identities_against_autograd(npieces):
    """(xhat * gamma + beta) W_k^T + b_k = xhat (W_k * gamma)^T + (b_k + W_k beta), and the gradients the folded pair's gradients give."""
    rows, J, F = 7, 5, 3
    rng = np.random.default_rng(3 + npieces)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s)).requires_grad_()
    xhat = torch.from_numpy(rng.standard_normal((rows, F)))
    gamma, beta = t(F), t(F)
    Ws, bs = [t(J, F) for _ in range(npieces)], [t(J) for _ in range(npieces)]
    up = [torch.from_numpy(rng.standard_normal((rows, J))) for _ in range(npieces)]
    ys = [(xhat * gamma + beta) @ W.T + b for W, b in zip(Ws, bs)]
    sum((y * u).sum() for y, u in zip(ys, up)).backward()
    n = lambda a: a.detach().numpy()
    dWfs = [n(u).T @ n(xhat) for u in up]                                   # what the stack returns for the folded pair
    dbfs = [n(u).sum(0) for u in up]
    fwd, bwd, dgamma, dbeta = ref.fold_ref([n(W) for W in Ws], [n(b) for b in bs], n(gamma), n(beta), dWfs, dbfs)
    for k in range(npieces):
        assert np.abs(n(xhat) @ fwd[k][0].T + fwd[k][1] - n(ys[k])).max() < 1e-12
        assert np.abs(bwd[k][0] - n(Ws[k].grad)).max() < 1e-12 and np.abs(bwd[k][1] - n(bs[k].grad)).max() < 1e-12
    assert np.abs(dgamma - n(gamma.grad)).max() < 1e-12 and np.abs(dbeta - n(beta.grad)).max() < 1e-12


# ----------------------------------------------------------------------------- the model's parameter list, on the host
@pytest.fixture()
def host_models(monkeypatch):
    """AudioGRU built with its flat buffers in host memory: construction launches nothing, and the size queries that choose the
    sweeps run without a GPU."""
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib, models, nn, parallel
    monkeypatch.setattr(nn, '_device', lambda: torch.device('cpu'))
    return _lib, models, parallel


def _config(F, H, Lyr, C, bidirectional=True):
    return dict(num_classes=C, learning_rate=1e-3, dropout=0.5, hidden_dims=H, rnn_layers=Lyr, embedding_size=F, bidirectional=bidirectional)


@pytest.mark.parametrize('Lyr', [1, 2, 3])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_model_keys_shapes_and_layout_are_the_torch_trees(host_models, variant, Lyr):
    _lib, models, parallel = host_models
    F, H, C = 24, 64, 2 if variant == 'clf' else 1
    m = models.AudioGRU(_config(F, H, Lyr, C), variant=variant, seed=0)
    net = TorchAudioBiGRU(variant, F, H, Lyr, C)
    sd, sd_t = m.state_dict(), net.state_dict()
    assert list(sd) == list(sd_t) == ref.key_list(variant, Lyr)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in sd_t.values()]
    assert m._bi_impl == _lib.IMPL_CLUSTER_BIGRU_TRAIN
    P = m._params
    live = [k for k, p in P.items() if p.live]
    assert live == ref.live_names(variant, Lyr)                             # the attention pair is live, bn is not
    # [no-decay | decay | dead]: 'ln' names first, every live range in definition order behind them
    order = sorted(live, key=lambda k: P[k].offset)
    assert order == [k for k in live if 'ln' in k] + [k for k in live if 'ln' not in k]
    assert all(P[k].offset >= m._n_live for k in P if not P[k].live)
    in_call, post = m.sync_plan()
    parallel.layer_buckets(list(in_call.values()) + list(post), m._n_live)  # every live float exactly once
    if variant == 'clf':                                                    # LayerNorm, attention and layer 0 wait for the fold's backward
        assert 0 not in in_call and len(post) == 1 and post[0][0] == P['ln.weight'].offset == 0
        assert sorted(in_call) == list(range(1, Lyr))
    else:
        assert post == [] and sorted(in_call) == list(range(Lyr)) and in_call[0][0] == P['attention_layer.0.weight'].offset
    top_end = P['fc_audio.4.bias'].offset + 4
    last = in_call[Lyr - 1] if Lyr - 1 in in_call else post[0]
    assert last[0] + last[1] == top_end == m._n_live                        # the head rides with the top layer


def test_widths_choose_the_sweeps_or_are_refused(host_models):
    _lib, models, _ = host_models
    for H in (64, 128, 256, 512):
        assert models.AudioGRU(_config(16, H, 2, 2), seed=0)._bi_impl == _lib.IMPL_CLUSTER_BIGRU_TRAIN
    for H in (16, 32, 48, 96, 192):
        assert models.AudioGRU(_config(16, H, 2, 2), seed=0)._bi_impl == _lib.IMPL_TILE
    with pytest.raises(_lib.DepError, match=r'64, 128, 256 and 512.*16, 32, 48, 96 and 192'):
        models.AudioGRU(_config(16, 40, 2, 2), seed=0)


def test_chunked_calls_are_refused_and_the_unidirectional_model_is_as_it_was(host_models):
    _lib, models, _ = host_models
    m = models.AudioGRU(_config(16, 64, 2, 2), seed=0)
    m.eval()
    with pytest.raises(_lib.DepError, match='cannot be cut into chunks'):
        m.stream()
    m.train()
    with pytest.raises(_lib.DepError, match='cannot be cut into chunks'):
        m.forward_chunked(np.zeros((1, 4, 16), np.float32), 2)
    uni = models.AudioGRU(_config(16, 64, 2, 2, bidirectional=False), seed=0)
    assert not uni._params['attention_layer.0.weight'].live and 'lstm_net_audio.weight_ih_l0_reverse' not in uni._params
    assert uni._rnns.impl == 0 and uni._rnns.args[4] == 1
