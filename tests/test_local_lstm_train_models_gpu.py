"""The consumer of impl = 9 (the exchange-free LSTM sweeps, forward and backward): TextBiLSTM with config['train_impl'] = 9 builds its one
cache on it -- train() and eval() forwards and the backward, dense and ragged, single GPU or data parallel.  It loads the default
model's state dict; the output, the loss and every gradient of one forward / backward / optimiser step agree with the default plan's
model (the cluster BiLSTM sweeps) at the recurrent paths' bars: 1e-4 absolute on outputs, 1e-4 of the largest magnitude on each gradient.
Small seeded models, text width 128, B = 6, T = 5."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L, models, nn, parallel, text_bilstm_whole

B, T, Ft, Ht, Lyr = 6, 5, 12, 128, 2
SEED = 0x5DEECE66D
ATOL = 1e-4
RTOL = 1e-4


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


def text_config(**kw):
    c = dict(num_classes=2, dropout=0.5, rnn_layers=Lyr, embedding_size=Ft, batch_size=B, epochs=1, learning_rate=1e-3, hidden_dims=Ht,
             bidirectional=True, cuda=False)
    c.update(kw)
    return c


def batch(ragged):
    rng = np.random.default_rng(31 + ragged)
    x = rng.standard_normal((B, T, Ft)).astype(np.float32)
    lengths = None
    if ragged:
        lengths = np.array([T, 1, 3, 2, T, 4])
        x[np.arange(T)[None, :] >= lengths[:, None]] = 0.0
    return x, lengths, list(rng.integers(0, 2, B))


def call(m, x, lengths):
    return m(x) if lengths is None else m(x, lengths=list(lengths))


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_one_training_step_agrees_with_the_default_plan(variant, ragged, monkeypatch):
    cfg = text_config(num_classes=2 if variant == 'clf' else 1)
    base = models.TextBiLSTM(cfg, variant=variant, seed=4)
    local = models.TextBiLSTM(dict(cfg, train_impl=9), variant=variant, seed=77)
    assert list(local.state_dict().keys()) == list(base.state_dict().keys())
    local.load_state_dict(base.state_dict())
    assert base._rnns.impl == L.IMPL_AUTO and local._rnns.impl == L.IMPL_LOCAL_LSTM_TRAIN and local._eval_rnns is None
    x, lengths, labels = batch(ragged)
    monkeypatch.setattr(nn, 'next_dropout_seed', lambda: SEED)
    rag = 'true' if ragged else 'false'
    res = {}
    for name, m in (('base', base), ('local', local)):
        opt = nn.AdamW(text_bilstm_whole.get_param_group(m), lr=1e-3) if variant == 'clf' else nn.Adam(m.parameters(), lr=1e-3)
        crit = nn.CrossEntropyLoss() if variant == 'clf' else nn.L1Loss()
        y = labels if variant == 'clf' else np.asarray(labels, np.float32) * 1.5
        before = {n: host(v) for n, v in m.state_dict().items()}
        m.eval()                                    # (before the step: both models still hold the same parameters)
        with launched() as ke:
            ev = host(call(m, x, lengths).data)
        m.check_health()
        m.train()
        opt.zero_grad()
        with launched() as k:
            out = call(m, x, lengths)
            loss = crit(out, y)
            loss.backward()
        m.check_health()
        grads = {n: host(p.grad) for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        after = {n: host(v) for n, v in m.state_dict().items()}
        moved = max(np.abs(after[n] - before[n]).max() for n in after)
        assert all(np.isfinite(v).all() for v in after.values()) and 1e-4 < moved < 1e-2, moved          # the optimiser step ran (lr = 1e-3)
        res[name] = dict(out=host(out.data), loss=float(loss.item()), grads=grads, eval=ev, sweeps=k.sweeps, eval_sweeps=ke.sweeps)
    loc, bas = res['local'], res['base']
    assert loc['sweeps'] == ['lstm_fwd_save_local<true, %s>' % rag] * Lyr + ['lstm_bwd_local<true, %s>' % rag] * Lyr, loc['sweeps']
    assert loc['eval_sweeps'] == ['lstm_fwd_local<true, %s>' % rag] * Lyr, loc['eval_sweeps']          # eval() on the same cache
    assert bas['sweeps'] and all(s.startswith(('lstm_fwd_cluster<', 'lstm_bwd_cluster<')) for s in bas['sweeps'] + bas['eval_sweeps'])
    assert local.status_words() == [] and local.fallback_words() == []                                # no status word: check_health passed without one
    figs = dict(out=np.abs(loc['out'] - bas['out']).max(), loss=abs(loc['loss'] - bas['loss']), eval=np.abs(loc['eval'] - bas['eval']).max())
    rel = {n: np.abs(loc['grads'][n] - g).max() / max(np.abs(g).max(), 1e-12) for n, g in bas['grads'].items()}
    worst = max(rel, key=rel.get)
    print('text %s %s train_impl 9 vs default: ' % (variant, rag) + ', '.join(f'{k} {v:.2e}' for k, v in figs.items()) +
          f', worst gradient {rel[worst]:.2e} ({worst}) of {len(rel)}')
    assert set(loc['grads']) == set(bas['grads']) and any('lstm_net.weight_hh' in n for n in rel)
    assert all(np.isfinite(v).all() for v in loc['grads'].values()) and np.isfinite(loc['out']).all() and np.isfinite(loc['eval']).all()
    for k, v in figs.items():
        assert v < ATOL, (k, v)
    for n, v in rel.items():
        if np.abs(bas['grads'][n]).max() == 0:          # (an L1 head's bias gradient is a sum of signs: it can be exactly 0, on both plans)
            assert not n.startswith('lstm_net.') and np.abs(loc['grads'][n]).max() == 0, n
        else:
            assert v < RTOL, (n, v)


def test_eval_impl_keeps_working_beside_train_impl(monkeypatch):
    m = models.TextBiLSTM(text_config(train_impl=9, eval_impl=8), seed=4)
    assert m._rnns.impl == L.IMPL_LOCAL_LSTM_TRAIN and m._eval_rnns.impl == L.IMPL_LOCAL_LSTM
    x, lengths, labels = batch(False)
    m.eval()
    with launched() as k:
        out = m(x)
    assert k.sweeps == ['lstm_fwd_local<true, false>'] * Lyr
    with pytest.raises(L.DepError, match='eval_impl'):
        m.backward(torch.zeros_like(out.data))
    m.train()
    with launched() as k:
        nn.CrossEntropyLoss()(m(x), labels).backward()
    assert k.sweeps == ['lstm_fwd_save_local<true, false>'] * Lyr + ['lstm_bwd_local<true, false>'] * Lyr


def test_bad_choices_raise():
    for bad in (0, 3, 8, '9', True):
        with pytest.raises(L.DepError, match='train_impl'):
            models.TextBiLSTM(text_config(train_impl=bad))
    with pytest.raises(L.DepError, match='impl = 9'):          # the descriptor exists at H = 128 only
        models.TextBiLSTM(text_config(hidden_dims=64, train_impl=9))


def test_overlapped_backward_on_a_one_rank_communicator_leaves_the_plain_gradients():
    """parallel.make_grad_sync on this config: dep_rnn_backward_overlapped[_varlen] on impl = 9 with the C-ABI's one-rank RCCL communicator
    (a one-rank SUM is the identity) must leave exactly the gradients of the plain backward, dense and ragged."""
    grads = {}
    try:
        for native in (False, True):
            if native:
                assert parallel.init_native_comm(force_single=True) is not None
            for ragged in (False, True):
                model = models.TextBiLSTM(text_config(dropout=0.0, train_impl=9), seed=3)
                x, lengths, labels = batch(ragged)
                model.train()
                with launched() as k:
                    nn.CrossEntropyLoss()(call(model, x, lengths), labels).backward()
                torch.cuda.synchronize()
                assert [s.split('<')[0] for s in k.sweeps] == ['lstm_fwd_save_local'] * Lyr + ['lstm_bwd_local'] * Lyr
                grads[ragged, native] = model.live_grad_bucket().clone()
    finally:
        parallel.destroy_native_comm()
    for ragged in (False, True):
        assert torch.isfinite(grads[ragged, False]).all() and float(grads[ragged, False].abs().max()) > 0
        assert torch.equal(grads[ragged, False], grads[ragged, True]), ragged


# ----------------------------------------------------------------------------- two ranks (tests/test_dp_gpu.py's check on this config)
def _run(rank, world, port, q, backend):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank) if backend == 'nccl' else '0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    sys.path.insert(0, ROOT)
    from icassp2022_depression_amd import nn, parallel, text_bilstm_whole as m
    torch.manual_seed(2024)
    if backend == 'nccl':
        torch.cuda.set_device(rank)
    if world > 1:
        parallel.init_from_env(backend)
    rng = np.random.default_rng(7)
    m.config.update(embedding_size=Ft, hidden_dims=Ht, dropout=0.0, batch_size=5, learning_rate=1e-3, train_impl=9)
    m.text_features = rng.standard_normal((12, T, Ft)).astype(np.float32); m.text_targets = rng.integers(0, 2, 12)
    m.model = m.TextBiLSTM(m.config, seed=0)
    m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate']); m.criterion = nn.CrossEntropyLoss()
    idx = list(range(12))                     # 5, 5, 2
    with contextlib.redirect_stdout(io.StringIO()):
        m.train(1, idx); m.train(2, idx)
    assert m.model._rnns.impl == 9
    if rank == 0:
        q.put(({k: v.cpu().numpy() for k, v in m.model.state_dict().items()}, int(m.train_acc)))
    if world > 1:
        parallel.barrier()
        parallel.destroy_native_comm()
        import torch.distributed as dist
        dist.destroy_process_group()


def two_rank_check(backend):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    res = {}
    for world in (1, 2):
        q = ctx.Queue()
        port = 25300 + os.getpid() % 500 + world
        procs = [ctx.Process(target=_run, args=(r, world, port, q, backend if world > 1 else 'gloo')) for r in range(world)]
        for p in procs:
            p.start()
        res[world] = q.get(timeout=300)
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    (sd1, acc1), (sd2, acc2) = res[1], res[2]
    assert acc1 == acc2
    for k in sd1:
        assert np.abs(sd1[k] - sd2[k]).max() < 2e-6 + 1e-5 * np.abs(sd1[k]).max(), k


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2, reason='needs two GPUs (a multi-GPU driver box)')
def test_two_rank_training_equals_single_process():
    """One process per GPU over the C-ABI's RCCL communicator: two epochs of text_bilstm_whole.train() with config['train_impl'] = 9 must
    leave the parameters of the single-process run (the equality check of tests/test_dp_gpu.py)."""
    two_rank_check('nccl')
