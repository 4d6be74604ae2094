"""GPU parity of the bidirectional audio encoder: AudioBiLSTM(config) with config['bidirectional'] = True, both variants, against
tests/audio_bigru_ref.py (float64, the model's own dropout masks from the oracle's Philox).

Tolerances are the project's own for the script-shaped modules (tests/test_models_gpu.py): outputs 1e-4 absolute, loss
1e-4 * max(1, |loss|), gradients relerr 1e-3, parameters after three optimizer steps 5e-5 + 2e-4 * max|v| (AdamW over get_param_group
for clf, Adam for reg, at the scripts' learning rates: one Adam step moves an element by at most lr, so an element whose tiny gradient
changed sign costs 2 lr per step, inside the bound).  Every case fills the gradient tensors and the reserve with NaN first and ends with
check_health() and a zero status word.  Every case fails on a build whose constructor refuses the flag.
Run on the MI355X box:  python -m pytest tests/test_audio_bigru_gpu.py -m gpu -q"""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

import audio_bigru_ref as ref
import test_bigru_cluster_bwd_gpu as bwd_base
import test_bigru_cluster_gpu as base
from conftest import ROOT
from test_audio_bigru_cpu import TorchAudioBiGRU
from varlen_ref import lengths_mix

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _common, audio_bilstm_perm, audio_gru_whole, nn, parallel
    from icassp2022_depression_amd import _lib as L

ATOL = 1e-4
NAN = float('nan')


def script(variant):
    return audio_gru_whole if variant == 'clf' else audio_bilstm_perm


def relerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-12))


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@contextlib.contextmanager
def gemm_mode(mode):
    """Mode 0 (exact fp32) or 1 (3-term bf16 split) forced on every contraction size, as tests/test_bigru_cluster_gpu.py does."""
    L.set_gemm_mode(mode, 0)
    try:
        yield
    finally:
        L.set_gemm_mode(1, 1 << 28)


def build(variant, F, H, Lyr, p, rng):
    mod = script(variant)
    C = 2 if variant == 'clf' else 1
    cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, rnn_layers=Lyr, dropout=p, bidirectional=True, num_classes=C)
    model = mod.AudioBiLSTM(cfg, seed=0)
    assert list(model.state_dict()) == ref.key_list(variant, Lyr)
    P = ref.make_params(rng, F, H, Lyr, C, variant)
    model.load_state_dict({k: torch.from_numpy(v.astype(np.float32)) for k, v in P.items()}, strict=False)
    return model, P, cfg


def problem(variant, B, T, F, rng, lengths=None):
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    if lengths is not None:
        x[np.arange(T)[None, :] >= np.asarray(lengths)[:, None]] = 0.0
    y = rng.integers(0, 2, B) if variant == 'clf' else rng.uniform(0.0, 3.0, B).astype(np.float32)
    return x, y


def make_optimizer(variant, model):
    if variant == 'clf':
        groups = audio_gru_whole.get_param_group(model)
        assert sorted(p.name for p in groups[1]['params']) == ['ln.bias', 'ln.weight']
        return nn.AdamW(groups, lr=audio_gru_whole.config['learning_rate']), audio_gru_whole.config['learning_rate']
    return nn.Adam(model.parameters(), lr=audio_bilstm_perm.config['learning_rate']), audio_bilstm_perm.config['learning_rate']


def healthy(model, cluster):
    model.check_health()
    words = [int(w.item()) for w in model.status_words()]
    assert words == ([0] if cluster else []), words             # the tile sweeps have no exchange buffer, so no status word


def expected_sweeps(H, Lyr, B, split, ragged):
    n = Lyr * bwd_base.chunks(H, B)
    return [base.forward_instance(H, split, ragged)] * n, [bwd_base.backward_instance(H, split, ragged)] * n


def train_case(monkeypatch, variant, shape, p, mode, ragged=False):
    """Three optimizer steps; the first is held against the yardstick output by output and gradient by gradient, and (on the cluster
    sweeps) its launches against the BI instances of the per-layer cluster kernels."""
    B, T, F, H, Lyr = shape
    rng = np.random.default_rng(9000 + B * 7 + T * 11 + H + Lyr + (variant == 'reg') * 5 + int(p * 10) + mode)
    lengths = None
    if ragged:
        lengths = lengths_mix(B, T, rng)
        lengths[3] = T // 2
        assert lengths.tolist()[:4] == [T, 1, 0, T // 2]
    with gemm_mode(mode):
        model, P, cfg = build(variant, F, H, Lyr, p, rng)
        cluster = model._bi_impl == L.IMPL_CLUSTER_BIGRU_TRAIN
        x, y = problem(variant, B, T, F, rng, lengths)
        opt, lr = make_optimizer(variant, model)
        crit = nn.CrossEntropyLoss() if variant == 'clf' else nn.L1Loss()
        model.train()
        model._rnns.get(B, T, L.RUN_TRAIN).reserve.fill_(NAN)
        seeds = [int(v) for v in rng.integers(1, 2 ** 63, 3)]      # the case's own dropout keys, whatever ran before it in the session
        draw = iter(seeds)
        monkeypatch.setattr(nn, 'next_dropout_seed', lambda: next(draw))
        losses, first = [], None
        for s in range(3):
            opt.zero_grad()
            for prm in model.parameters():
                if prm.live:
                    prm._grad.fill_(NAN)
            with base.launched() as kf:
                out = model(x, lengths=lengths)
            loss = crit(out, y if variant == 'clf' else y.reshape(-1, 1))
            with base.launched() as kb:
                loss.backward()
            losses.append(loss.item())
            healthy(model, cluster)
            if s == 0:
                first = dict(out=out.numpy().astype(np.float64), alpha=model.last_alpha.cpu().numpy().astype(np.float64),
                             G={k: q.grad.cpu().numpy().astype(np.float64) for k, q in model.named_parameters() if q.grad is not None},
                             fwd=kf.sweeps, bwd=kb.sweeps)
            opt.step()
        after = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    P_ref, losses_ref, r = ref.train(P, x.astype(np.float64), y, variant, Lyr, 3, lr, seeds=seeds, p=p, lengths=lengths)
    figures = [('out', float(np.abs(first['out'] - r['out']).max()))] + \
              [(f'loss{s}', abs(losses[s] - losses_ref[s])) for s in range(3)] + [(k, relerr(first['G'][k], r['G'][k])) for k in r['G']]
    print(f'audio-bigru {variant} {shape} p={p} mode={mode} ragged={ragged}: ' + ', '.join(f'{n} {e:.2e}' for n, e in figures))
    assert np.abs(first['out'] - r['out']).max() < ATOL
    live = lengths if lengths is not None else np.full(B, T)
    for b in range(B):
        if live[b]:
            assert np.abs(first['alpha'][b, :live[b]] - r['alpha'][b, :live[b]]).max() < ATOL
    for s in range(3):
        assert abs(losses[s] - losses_ref[s]) < ATOL * max(1.0, abs(losses_ref[s])), (s, losses[s], losses_ref[s])
    assert set(first['G']) == set(r['G']) == set(ref.live_names(variant, Lyr))
    for k, g in r['G'].items():
        assert np.isfinite(first['G'][k]).all(), k
        assert np.abs(g).max() > 0, f'{k}: the reference gradient is trivially zero'
        assert relerr(first['G'][k], g) < 1e-3, (k, relerr(first['G'][k], g))
    for k, v in P_ref.items():
        assert np.abs(after[k] - v).max() < 5e-5 + 2e-4 * np.abs(v).max(), k
    if cluster:
        fwd, bwd = expected_sweeps(H, Lyr, B, mode == 1, ragged)
        assert first['fwd'] == fwd and first['bwd'] == bwd, (first['fwd'], first['bwd'])     # once per layer and chunk, no gru_bwd_mfma
    else:
        assert first['fwd'] and all('_mfma<' in s for s in first['fwd'] + first['bwd']), (first['fwd'], first['bwd'])
    return model


# two tiles, the second with one live row; two members per cluster; inter-layer dropout over 2H columns
@pytest.mark.parametrize('mode', [1, 0], ids=['bf16x3', 'f32'])
@pytest.mark.parametrize('p', [0.0, 0.5])
def test_classifier_two_tiles(p, mode, monkeypatch):
    train_case(monkeypatch, 'clf', (17, 5, 24, 64, 2), p, mode)


def test_classifier_h256_all_gather_split_backward(monkeypatch):
    train_case(monkeypatch, 'clf', (3, 4, 32, 256, 2), 0.5, 1)


def test_classifier_h512_the_width_only_the_cluster_sweeps_train(monkeypatch):
    train_case(monkeypatch, 'clf', (2, 3, 16, 512, 2), 0.5, 1)


def test_classifier_h48_runs_the_tile_sweeps_without_an_exchange_buffer(monkeypatch):
    model = train_case(monkeypatch, 'clf', (2, 3, 16, 48, 2), 0.5, 1)
    assert model._bi_impl == L.IMPL_TILE and model._rnns.last.status_word() is None


def test_regression_one_layer_ragged(monkeypatch):
    """One layer: no inter-layer dropout, K = 2.  lengths T, 1, 0 and an interior one; the empty row has ctx = 0 (its output is the
    head of a zero row, as the yardstick computes it) and passes no gradient."""
    train_case(monkeypatch, 'reg', (4, 6, 16, 128, 1), 0.5, 1, ragged=True)


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_ragged_call_with_full_lengths_is_the_dense_call_bit_for_bit(variant):
    B, T, F, H, Lyr = 4, 6, 16, 128, 1
    rng = np.random.default_rng(31)
    model, P, _ = build(variant, F, H, Lyr, 0.5, rng)
    x, _ = problem(variant, B, T, F, rng)
    model.eval()
    dense = model(x).data.clone()
    rag = model(x, lengths=np.full(B, T)).data.clone()
    healthy(model, True)
    assert torch.equal(dense.view(torch.int32), rag.view(torch.int32))


def test_h40_is_refused_at_construction():
    cfg = dict(audio_gru_whole.config); cfg.update(embedding_size=16, hidden_dims=40, bidirectional=True)
    with pytest.raises(L.DepError, match='16, 32, 48, 96 and 192'):
        audio_gru_whole.AudioBiLSTM(cfg, seed=0)


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_eval_output_and_alpha(variant):
    """model.eval(): the yardstick without masks; last_alpha rows sum to 1 over the live steps."""
    B, T, F, H, Lyr = 5, 7, 24, 64, 2
    rng = np.random.default_rng(77 + (variant == 'reg'))
    lengths = np.array([T, 1, 0, 4, T - 1])
    model, P, _ = build(variant, F, H, Lyr, 0.5, rng)
    model.eval()
    for n in (None, lengths):
        x, _ = problem(variant, B, T, F, rng, n)
        out = model(x, lengths=n)
        healthy(model, True)
        r = ref.step(P, x.astype(np.float64), None, variant, Lyr, lengths=n)
        assert np.abs(out.numpy() - r['out']).max() < ATOL
        alpha = model.last_alpha.cpu().numpy().astype(np.float64)
        for b in range(B):
            k = T if n is None else int(n[b])
            if k:
                assert abs(alpha[b, :k].sum() - 1.0) < 1e-5 and np.abs(alpha[b, :k] - r['alpha'][b, :k]).max() < ATOL


# ----------------------------------------------------------------------------- the several-map fold
@pytest.mark.parametrize('JF', [(192, 24), (768, 256), (5, 3)], ids=base.ident)
@pytest.mark.parametrize('npieces', [1, 2])
def test_fold_for_several_maps(npieces, JF):
    J, F = JF
    rng = np.random.default_rng(J * 3 + F + npieces)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    Ws, bs, dWfs, dbfs = ([f32(J, F) for _ in range(npieces)], [f32(J) for _ in range(npieces)], [f32(J, F) for _ in range(npieces)],
                          [f32(J) for _ in range(npieces)])
    gamma, beta = f32(F), f32(F)
    dev, nans, bits = base.dev, base.nans, base.bits
    d = lambda ts: [dev(t) for t in ts]

    def run(order):
        pick = lambda ts: [ts[k] for k in order]
        Wf, bf, dW, db = ([nans(J, F) for _ in order], [nans(J) for _ in order], [nans(J, F) for _ in order], [nans(J) for _ in order])
        dg, dbt = nans(F), nans(F)
        L.ln_fold_fwd_multi(d(pick(Ws)), d(pick(bs)), dev(gamma), dev(beta), Wf, bf)
        L.ln_fold_bwd_multi(d(pick(Ws)), d(pick(dWfs)), d(pick(dbfs)), dev(gamma), dev(beta), dW, db, dg, dbt)
        return Wf, bf, dW, db, dg, dbt
    order = list(range(npieces))
    Wf, bf, dW, db, dg, dbt = run(order)
    again = run(order)
    assert np.array_equal(bits(dg), bits(again[4])) and np.array_equal(bits(dbt), bits(again[5])), 'dgamma / dbeta differ between two runs'
    if npieces == 1:                                           # the bits of the single-map entry points
        Wf1, bf1, dW1, db1, dg1, dbt1 = nans(J, F), nans(J), nans(J, F), nans(J), nans(F), nans(F)
        L.ln_fold_fwd(dev(Ws[0]), dev(bs[0]), dev(gamma), dev(beta), Wf1, bf1)
        L.ln_fold_bwd(dev(Ws[0]), dev(dWfs[0]), dev(dbfs[0]), dev(gamma), dev(beta), dW1, db1, dg1, dbt1)
        for name, a, b in (('Wf', Wf[0], Wf1), ('bf', bf[0], bf1), ('dW', dW[0], dW1), ('db', db[0], db1), ('dgamma', dg, dg1), ('dbeta', dbt, dbt1)):
            assert torch.isfinite(a).all() and np.array_equal(bits(a), bits(b)), name
        return
    f64 = lambda ts: [t.astype(np.float64) for t in ts]
    fwd, bwd, dg_ref, dbt_ref = ref.fold_ref(f64(Ws), f64(bs), gamma.astype(np.float64), beta.astype(np.float64), f64(dWfs), f64(dbfs))
    pairs = [('dgamma', dg, dg_ref), ('dbeta', dbt, dbt_ref)]
    for k in range(npieces):
        pairs += [(f'Wf{k}', Wf[k], fwd[k][0]), (f'bf{k}', bf[k], fwd[k][1]), (f'dW{k}', dW[k], bwd[k][0]), (f'db{k}', db[k], bwd[k][1])]
    errs = [(n, relerr(base.host(a), b)) for n, a, b in pairs]
    print(f'fold {npieces} pieces {JF}: ' + ', '.join(f'{n} {e:.2e}' for n, e in errs))
    for n, e in errs:
        assert e < 1e-6, (n, e)
    sw = run(order[::-1])                                      # the pieces swapped: dW_k swap, dgamma / dbeta move by one rounding of the one add
    for k in range(npieces):
        assert np.array_equal(bits(sw[2][k]), bits(dW[npieces - 1 - k])) and np.array_equal(bits(sw[3][k]), bits(db[npieces - 1 - k]))
    for a, b in ((sw[4], dg), (sw[5], dbt)):
        a, b = base.host(a), base.host(b)
        assert (np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))).all()


# ----------------------------------------------------------------------------- checkpoints, refusals, scripts
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_checkpoints(variant, tmp_path):
    F, H, Lyr = 16, 64, 2
    rng = np.random.default_rng(3)
    model, P, cfg = build(variant, F, H, Lyr, 0.5, rng)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    other = script(variant).AudioBiLSTM(cfg, seed=1)
    other.load_state_dict(sd, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    path = _common.export_reference_checkpoint(model, str(tmp_path / 'exported'))
    net = TorchAudioBiGRU(variant, F, H, Lyr, cfg['num_classes'])
    loaded = _common.load_checkpoint_state_dict(path)
    net.load_state_dict(loaded, strict=True)                   # the stock tree, on the CPU
    assert list(loaded) == list(net.state_dict())
    quiet(_common.save, model, str(tmp_path / 'saved'))
    assert list(_common.load_checkpoint_state_dict(str(tmp_path / 'saved.pt'))) == ref.key_list(variant, Lyr)
    opt, _ = make_optimizer(variant, model)
    _common.save_checkpoint(model, opt, str(tmp_path / 'resume'))
    _common.load_checkpoint(other, opt, str(tmp_path / 'resume'))


def test_chunked_and_streamed_calls_are_refused():
    model, _, _ = build('clf', 16, 64, 2, 0.5, np.random.default_rng(4))
    with pytest.raises(L.DepError, match='cannot be cut into chunks'):
        model.forward_chunked(np.zeros((2, 4, 16), np.float32), 2)
    model.eval()
    with pytest.raises(L.DepError, match='cannot be cut into chunks'):
        model.stream()


def _synthetic(variant, N, T, F, rng):
    feats = rng.standard_normal((N, T, F)).astype(np.float32)
    targs = (np.arange(N) % 2).astype(np.int64) if variant == 'clf' else rng.uniform(0.0, 20.0, N).astype(np.float32)
    return feats, targs


def _script_setup(variant, F, H, feats, targs, batch_size):
    m = script(variant)
    m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, batch_size=batch_size, bidirectional=True)
    m.audio_features, m.audio_targets = feats, targs
    m.model = m.AudioBiLSTM(m.config, seed=0)
    if variant == 'clf':
        m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate']); m.criterion = nn.CrossEntropyLoss()
    else:
        m.optimizer = nn.Adam(m.model.parameters(), lr=m.config['learning_rate']); m.criterion = nn.L1Loss()
    return m


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_scripts_train_and_evaluate_with_the_flag(variant):
    """The module-level train() / evaluate() of both audio scripts run a bidirectional model as they are."""
    N, T, F, H = 12, 5, 24, 64
    feats, targs = _synthetic(variant, N, T, F, np.random.default_rng(8))
    m = script(variant)
    saved = dict(m.config)
    gates = {k: getattr(m, k) for k in ('max_f1', 'max_acc', 'max_rec', 'max_prec', 'min_mae') if hasattr(m, k)}
    try:
        _script_setup(variant, F, H, feats, targs, 5)
        before = m.model._flat.clone()
        if variant == 'clf':
            m.max_f1 = m.max_acc = m.max_rec = m.max_prec = 2.0
            idx = list(range(N))
            quiet(m.train, 1, idx)
            loss = quiet(m.evaluate, m.model, idx, 1, idx, idx)
        else:
            m.train_dep_idxs, m.train_non_idxs = [0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10, 11]
            m.test_dep_idxs, m.test_non_idxs = [0, 1], [5, 6]
            m.min_mae = -1.0
            mae = quiet(m.train, 1)
            loss = quiet(m.evaluate, 0, m.model, mae)
        assert np.isfinite(loss) and not torch.equal(before, m.model._flat)
        healthy(m.model, True)
    finally:
        m.config.clear(); m.config.update(saved)
        for k, v in gates.items():
            setattr(m, k, v)


# ----------------------------------------------------------------------------- data parallel
def test_native_one_rank_communicator_reduces_every_range_once():
    """The C-ABI's own communicator with one rank (a SUM over one rank is the identity): the gradients are the plain backward's bits,
    and the order log shows the in-call ranges of sync_plan() once each and the rest as one grouped operation -- every live float once."""
    rng = np.random.default_rng(12)
    grads = {}
    try:
        for native in (False, True):
            if native:
                assert parallel.init_native_comm(force_single=True) is not None
            for variant, Lyr in (('clf', 2), ('reg', 2), ('clf', 1)):
                model, _, _ = build(variant, 24, 64, Lyr, 0.0, np.random.default_rng(5))
                x, y = problem(variant, 9, 5, 24, np.random.default_rng(6))
                model.train()
                crit = nn.CrossEntropyLoss() if variant == 'clf' else nn.L1Loss()
                loss = crit(model(x), y if variant == 'clf' else y.reshape(-1, 1))
                L.order_log_enable(True); L.order_log_read(reset=True)
                loss.backward()
                torch.cuda.synchronize()
                log = L.order_log_read(reset=True); L.order_log_enable(False)
                healthy(model, True)
                grads[(variant, Lyr, native)] = model.live_grad_bucket().clone()
                in_call, post = model.sync_plan()
                parallel.layer_buckets(list(in_call.values()) + list(post), model._n_live)
                if native:
                    single = sorted(int(e.split('n=')[1]) for e in log if e.startswith('C allreduce n='))
                    grouped = [int(e.split('n=')[1]) for e in log if e.startswith('C allreduce_ranges')]
                    assert single == sorted(c for _, c in in_call.values()), (log, in_call)
                    assert grouped == ([sum(c for _, c in post)] if post else []), (log, post)
                    assert sum(single) + sum(grouped) == model._n_live
    finally:
        parallel.destroy_native_comm()
    for variant, Lyr in (('clf', 2), ('reg', 2), ('clf', 1)):
        assert torch.equal(grads[(variant, Lyr, False)], grads[(variant, Lyr, True)]), (variant, Lyr)


def _dp_rank(rank, world, port, q):
    """One gloo rank on cuda:0: two epochs of audio_gru_whole.train() on a bidirectional classifier, batches of 5, 5, 2."""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    sys.path.insert(0, ROOT)
    from icassp2022_depression_amd import _lib as L, parallel
    parallel.init_from_env('gloo')
    feats, targs = _synthetic('clf', 12, 5, 24, np.random.default_rng(8))
    m = _script_setup('clf', 24, 64, feats, targs, 5)
    L.order_log_enable(True); L.order_log_read(reset=True)
    quiet(m.train, 1, list(range(12))); quiet(m.train, 2, list(range(12)))
    torch.cuda.synchronize()
    log = L.order_log_read(reset=True); L.order_log_enable(False)
    m.model.check_health()
    import torch.distributed as dist
    flat = m.model._flat.clone(); dist.broadcast(flat, src=0)
    diff = (m.model._flat - flat).abs().max().reshape(1); dist.all_reduce(diff, op=dist.ReduceOp.MAX)
    if rank == 0:
        q.put(({k: v.cpu().numpy() for k, v in m.model.state_dict().items()}, float(diff.item()), log))
    parallel.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_the_single_process():
    """Modelled on tests/test_dp_gpu.py's AudioGRU case, with its bound: two ranks on one GPU end bit-equal to each other and within
    2e-6 of the single-process run; every backward is followed by exactly one reduction of the live bucket."""
    import torch.multiprocessing as mp
    feats, targs = _synthetic('clf', 12, 5, 24, np.random.default_rng(8))
    m = audio_gru_whole
    saved = dict(m.config)
    try:
        _script_setup('clf', 24, 64, feats, targs, 5)
        quiet(m.train, 1, list(range(12))); quiet(m.train, 2, list(range(12)))
        healthy(m.model, True)
        single = {k: v.cpu().numpy() for k, v in m.model.state_dict().items()}
    finally:
        m.config.clear(); m.config.update(saved)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 25300 + os.getpid() % 500
    procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    sd, diff, log = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert diff == 0.0, 'the replicas differ'
    for k, v in single.items():
        assert np.abs(v - sd[k]).max() < 2e-6, k
    marks = ''.join('b' if e.startswith('N backward begin') else 'e' if e.startswith('N backward end') else
                    'c' if 'all_reduce of the live bucket' in e else '' for e in log)
    assert marks == 'bce' * 6, marks                           # 2 epochs x 3 mini-batches: one reduction inside every backward
