"""Gradient accumulation over micro-batches: dep_grad_accumulate, nn.Adam / AdamW(accumulate_steps=K), the declared row count and the
training loops over them.

Yardsticks.  The kernel is two fp32 roundings per element (product, sum, no FMA): numpy float32 reproduces it BIT FOR BIT, and its
partial sums of squares are compared on their bits with dep_grad_sqnorm's.  The models run the reference's recorded big batches
(tests/golden/) cut into micro-batches that declare the big batch's row count: the accumulated gradient, the first update and the
summed loss are held to exactly the bars tests/test_models_gpu.py applies to the same fixtures run as ONE batch (relerr 1e-3 on the
gradients, 2e-5 + 1e-4 max|v| on the parameters after the first update, 1e-4 on the loss); the clipped update to tests/test_clip_gpu.py's
(2e-7 against clip_ref on the gradient the device holds); the two-rank run to tests/test_dp_gpu.py's 2e-6 against one process.
"""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

from clip_ref import clip_coef, clipped_adam_step, sqnorm
from conftest import ROOT, load_golden

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L, nn, parallel
    from icassp2022_depression_amd import audio_bilstm_perm, audio_gru_whole, text_bilstm_perm, text_bilstm_whole
    DEV = torch.device('cuda:0')
    SLOTS = L.grad_norm_slots()
else:
    SLOTS = 256

ATOL = 1e-4
BUCKET = 1610242                        # the text classifier's gradient bucket
ACCUM_KERNEL = 'grad_accumulate_kernel'


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def relerr(a, b):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-12)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _values(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(rng.uniform(-6, 2, n))).astype(np.float32)      # magnitudes over several decades


def _sqnorm_partials(ranges):
    part = torch.full((SLOTS,), -1.0, dtype=torch.float64, device=DEV)
    L.grad_sqnorm(ranges, part)
    return host(part)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('scale', [1.0, 0.25, 1.0 / 3.0])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024, 1025, 256 * 1024 + 7])
def test_accumulate_bits_against_numpy(n, scale):
    g1, g2 = _values(n, 2 * n), _values(n, 2 * n + 1)
    sc = np.float32(scale)
    acc = torch.full((n,), float('nan'), dtype=torch.float32, device=DEV)
    L.grad_accumulate([acc], [dev(g1)], scale, first=True)                  # the accumulator is not read: the NaNs are gone
    want1 = (g1 * sc).astype(np.float32)
    assert host(acc).tobytes() == want1.tobytes()
    d2 = dev(g2)
    L.grad_accumulate([acc], [d2], scale)
    want2 = want1 + (g2 * sc).astype(np.float32)
    assert want2.dtype == np.float32 and host(acc).tobytes() == want2.tobytes()
    assert host(d2).tobytes() == g2.tobytes()                                # g is read only
    if scale == 1.0:
        assert want2.tobytes() == (g1 + g2).tobytes()                        # the plain IEEE add


SPLIT = [5, 1, 1023, 4097, 7, 3, 1025, 300001, 3, 65, 999, 5, 1, 2049, 77777, 13]        # 16 ranges of odd counts, two of one element


def test_sixteen_ranges_equal_one_range_and_the_partials_are_grad_sqnorms():
    assert len(SPLIT) == 16 and all(c % 2 for c in SPLIT)
    n = sum(SPLIT)
    a0, g = _values(n, 3), _values(n, 4)
    cuts = np.cumsum([0] + SPLIT)
    want = a0 + g

    def run(pieces_of, first=False):
        acc = pieces_of(a0); gs = pieces_of(g)                              # each range in an allocation of its own (16-byte aligned)
        part = torch.full((SLOTS,), -1.0, dtype=torch.float64, device=DEV)  # every slot must be overwritten
        L.grad_accumulate(acc, gs, 1.0, first, part)
        return np.concatenate([host(t) for t in acc]), host(part), _sqnorm_partials(acc)

    many = lambda v: [dev(v[a:b].copy()) for a, b in zip(cuts[:-1], cuts[1:])]
    one = lambda v: [dev(v)]
    r16, p16, s16 = run(many)
    r1, p1, s1 = run(one)
    assert r16.tobytes() == r1.tobytes() == want.tobytes()
    assert p16.tobytes() == s16.tobytes() and p1.tobytes() == s1.tobytes()  # the partials ARE dep_grad_sqnorm's of the stored result
    assert p16.tobytes() == p1.tobytes()                                     # ... however the data is cut
    ref = sqnorm([want])
    assert abs(p16.sum() - ref) <= 1e-9 * ref
    # first: the partials are those of g * scale, not of the old accumulator
    rf, pf, sf = run(many, first=True)
    assert rf.tobytes() == g.tobytes() and pf.tobytes() == sf.tobytes() and pf.tobytes() != p16.tobytes()
    # without partials the result is the same
    acc = many(a0)
    L.grad_accumulate(acc, many(g))
    assert np.concatenate([host(t) for t in acc]).tobytes() == want.tobytes()


def test_two_runs_are_bit_equal_at_the_bucket_size():
    a0, g = _values(BUCKET, 12), dev(_values(BUCKET, 13))
    out = []
    for _ in range(2):
        acc = dev(a0)
        part = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
        L.grad_accumulate([acc], [g], 1.0, False, part)
        out.append((host(acc).tobytes(), host(part).tobytes(), _sqnorm_partials([acc]).tobytes()))
    assert out[0] == out[1] and out[0][1] == out[0][2]


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_nonfinite_gradient_reaches_the_accumulator_and_the_update_is_skipped(bad):
    rng = np.random.default_rng(5)
    n = 3000
    a0, g = _values(n, 21), _values(n, 22)
    g[1234] = bad
    acc = dev(a0)
    part = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
    L.grad_accumulate([acc], [dev(g)], 1.0, False, part)
    got = host(acc)
    assert (np.isnan(got[1234]) if np.isnan(bad) else np.isinf(got[1234])) and np.isfinite(np.delete(got, 1234)).all()
    assert not np.isfinite(host(part).sum())
    p, m, v = (rng.uniform(-0.5, 0.5, n).astype(np.float32), (0.01 * rng.standard_normal(n)).astype(np.float32),
               (1e-4 * rng.random(n)).astype(np.float32))
    dp, dm, dv = dev(p), dev(m), dev(v)
    clip_out = torch.zeros(4, device=DEV); stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    L.adam_step_clipped(dp, acc, dm, dv, 1e-4, 0.9, 0.999, 1e-8, 1e-5, True, 1, part, 1.0, True, clip_out, stats)
    assert host(dp).tobytes() == p.tobytes() and host(dm).tobytes() == m.tobytes() and host(dv).tobytes() == v.tobytes()
    assert host(clip_out)[2] == 0.0 and host(stats).tolist() == [1.0, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------ models, recorded gradients
def _pads(model):
    """Indices of the flat gradient buffer that belong to no tensor: the alignment pads inside the live bucket."""
    used = np.zeros(model._flat_grad.numel(), bool)
    for p in model.parameters():
        if p.live:
            used[p.offset:p.offset + p.numel] = True
    return np.flatnonzero(~used)


def _make(mod, cls, g):
    B, T, F, H = [int(v) for v in g['shape']]
    cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0)
    model = getattr(mod, cls)(cfg, seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()}, strict=True)
    return model


def _kernels_logged(fn):
    torch.cuda.synchronize()
    L.order_log_enable(True)
    try:
        fn(); torch.cuda.synchronize()
        log = L.order_log_read(reset=True)
    finally:
        L.order_log_enable(False)
    return [e[2:] for e in log if e.startswith('K ')]


MODEL_CASES = [
    # fixture, module, class, optimizer, loss, micro-batch sizes, accumulate_steps (None: the number of micro-batches; larger: flush())
    ('audio_clf_mid', 'audio_gru_whole', 'AudioBiLSTM', 'adamw', 'ce', (2, 3, 1), None),
    ('audio_clf_mid', 'audio_gru_whole', 'AudioBiLSTM', 'adamw', 'ce', (2, 3, 1), 5),
    ('audio_clf_cfg1', 'audio_gru_whole', 'AudioBiLSTM', 'adamw', 'ce', (3, 5), None),
    ('text_clf_mid', 'text_bilstm_whole', 'TextBiLSTM', 'adamw', 'ce', (1, 2, 3), None),
    ('audio_reg_mid', 'audio_bilstm_perm', 'AudioBiLSTM', 'adam', 'l1', (4, 2), None),
    ('text_reg_mid', 'text_bilstm_perm', 'TextBiLSTM', 'adam', 'sl1', (3, 3), None),
    ('text_reg_mid', 'text_bilstm_perm', 'TextBiLSTM', 'adam', 'sl1', (3, 3), 3),
]


@pytest.mark.parametrize('name,modname,cls,opt,loss,split,K', MODEL_CASES)
def test_accumulated_gradient_and_first_update_against_the_recorded_big_batch(name, modname, cls, opt, loss, split, K):
    mod = {'audio_gru_whole': audio_gru_whole, 'audio_bilstm_perm': audio_bilstm_perm,
           'text_bilstm_whole': text_bilstm_whole, 'text_bilstm_perm': text_bilstm_perm}[modname]
    g = load_golden(name)
    model = _make(mod, cls, g)
    x, y = g['x'], g['y']
    B = x.shape[0]
    assert sum(split) == B
    flush = K is not None
    K = len(split) if K is None else K
    assert K >= len(split) and flush == (K > len(split))
    lr = float(g['lr'])
    optimizer = nn.AdamW(mod.get_param_group(model), lr=lr, accumulate_steps=K) if opt == 'adamw' \
        else nn.Adam(model.parameters(), lr=lr, accumulate_steps=K)
    crit = {'ce': nn.CrossEntropyLoss, 'l1': nn.L1Loss, 'sl1': nn.SmoothL1Loss}[loss]()
    model.train()
    before = {k: host(v).copy() for k, v in model.state_dict().items()}
    pads = _pads(model)
    losses = []
    parallel.set_accumulated_count(B)                                       # every micro-batch divides by the rows of the WHOLE batch
    try:
        at = 0
        for i, b in enumerate(split):
            optimizer.zero_grad()
            yy = y[at:at + b]
            l = crit(model(x[at:at + b]), yy if loss == 'ce' else yy.reshape(-1, 1))
            l.backward()
            assert not host(model._flat_grad)[pads].any()
            optimizer.step()
            losses.append(l.item())
            at += b
            if i + 1 < len(split) or flush:                                 # no update yet
                assert optimizer.pending == i + 1 and optimizer._step == 0
                for k, v in model.state_dict().items():
                    assert host(v).tobytes() == before[k].tobytes(), k
    finally:
        parallel.set_accumulated_count(None)
    if flush:
        optimizer.flush()
    assert optimizer.pending == 0 and optimizer._step == 1
    assert _kernels_logged(optimizer.flush) == [] and optimizer._step == 1   # nothing pending: a flush launches nothing
    acc = {k: optimizer.accumulated_grad(p) for k, p in model.named_parameters()}
    live = {k: a for k, a in acc.items() if a is not None}
    assert set(live) == set(g['grads']), sorted(set(live) ^ set(g['grads']))    # the dead parameters have none
    for k, gr in g['grads'].items():
        e = relerr(host(live[k]), gr)
        print('%s %s: accumulated gradient relerr %.3g' % (name, k, e))
        assert live[k].shape == gr.shape and e < 1e-3, (k, e)
    if 'after1' in g:
        sd = model.state_dict()
        for k, v in g['after1'].items():
            assert np.abs(host(sd[k]) - v).max() < 2e-5 + 1e-4 * np.abs(v).max(), k
    else:                                                                    # no recorded update: it must at least have happened
        assert any(host(v).tobytes() != before[k].tobytes() for k, v in model.state_dict().items())
    total = float(np.sum(np.asarray(losses, np.float64)))
    print('%s: summed micro-losses %.7f, recorded %.7f' % (name, total, g['losses'][0]))
    assert abs(total - g['losses'][0]) < ATOL * max(1.0, abs(g['losses'][0]))
    assert len(pads) > 0
    assert not host(model._flat_grad)[pads].any()
    assert not host(optimizer._accum[id(model)])[pads].any()               # the pads the norm of a clipped update runs over
    model.check_health()


@pytest.mark.parametrize('name', ['fuse_clf', 'fuse_reg'])
def test_fusion_losses_honour_the_declared_row_count(name):
    """Both MyLoss variants (split-weight cross-entropy / SmoothL1): the recorded 10-row batch as 3 + 6 + 1 rows on given features; the bars
    are tests/test_models_gpu.py::test_fusion's for the single batch."""
    from icassp2022_depression_amd import fuse_net as fuse_net_reg, fuse_net_whole
    g = load_golden(name)
    N, T, Fa, Ft, Ha, Ht = [int(v) for v in g['dims']]
    m = fuse_net_whole if name == 'fuse_clf' else fuse_net_reg
    saved_cfg = dict(m.config)
    try:
        m.config.update(audio_embed_size=Fa, text_embed_size=Ft, audio_hidden_dims=Ha, text_hidden_dims=Ht, dropout=0.0,
                        batch_size=4, learning_rate=float(g['lr']), accum_steps=3)
        model = m.build(seed=0)
        assert m.optimizer.accumulate_steps == 3                                      # build() passes config['accum_steps'] on
        model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
        model.eval()
        tf, af = model.pretrained_feature([[g['xa'][i], g['xt'][i]] for i in range(N)])
        model.train()
        y = g['y']
        W = dict(model.named_parameters())['fc_final.0.weight']
        losses = []
        parallel.set_accumulated_count(N)
        for a, b in ((0, 3), (3, 9), (9, 10)):
            m.optimizer.zero_grad()
            l = m.criterion(tf[a:b].contiguous(), af[a:b].contiguous(), y[a:b], model)
            l.backward()
            m.optimizer.step()
            losses.append(l.item())
        assert m.optimizer.pending == 0 and m.optimizer._step == 1
        assert relerr(host(m.optimizer.accumulated_grad(W)), g['gW']) < 1e-3
        assert abs(sum(losses) - g['losses'][0]) < ATOL * max(1.0, abs(g['losses'][0]))
    finally:
        m.config.clear(); m.config.update(saved_cfg)
        parallel.set_accumulated_count(None)


def _tiny(name):
    mod, cls, fix = {'audio': (audio_gru_whole, 'AudioBiLSTM', 'audio_clf_tiny'), 'text': (text_bilstm_whole, 'TextBiLSTM', 'text_clf_tiny')}[name]
    g = load_golden(fix)
    return mod, _make(mod, cls, g), g


@pytest.mark.parametrize('name', ['audio', 'text'])
def test_accumulated_steps_with_clipping_against_numpy(name):
    mod, model, g = _tiny(name)
    lr, max_norm = 1e-4, 1e-3
    opt = nn.AdamW(mod.get_param_group(model), lr=lr, max_grad_norm=max_norm, accumulate_steps=2)
    wd = {p.name: grp['weight_decay'] for grp in opt.param_groups for p in grp['params']}
    crit = nn.CrossEntropyLoss()
    model.train()
    params = dict(model.named_parameters())
    x, y = g['x'], g['y']
    B = x.shape[0]
    cut = B // 2 + 1
    assert 0 < cut < B
    M, V = {}, {}
    parallel.set_accumulated_count(B)
    try:
        for step in (1, 2, 3):
            live, P0 = None, None
            for a, b in ((0, cut), (cut, B)):
                opt.zero_grad()
                crit(model(x[a:b]), y[a:b]).backward()
                if a == 0:
                    live = [n for n, p in params.items() if p.grad is not None]
                    P0 = {n: host(params[n].data).astype(np.float64) for n in live}
                opt.step()
            assert len(live) >= 12 and opt.pending == 0
            G = {n: host(opt.accumulated_grad(params[n])).copy() for n in live}       # what the update was made from
            S = sqnorm(list(G.values()))
            coef = clip_coef(S, max_norm)
            stats = opt.grad_stats()
            assert stats['steps'] == step and stats['last_finite']                   # updates, not micro-steps
            assert abs(stats['last_coef'] - coef) <= 1e-6 * coef and abs(stats['last_norm'] - np.sqrt(S)) <= 1e-6 * np.sqrt(S)
            if step == 1:
                assert coef < 1.0 and stats['clipped'] == 1
            for n in live:
                if step == 1:
                    M[n] = np.zeros_like(P0[n]); V[n] = np.zeros_like(P0[n])
                pn, M[n], V[n] = clipped_adam_step(P0[n], G[n], M[n], V[n], step, lr, coef, wd=wd[n], decoupled=True)
                assert np.abs(host(params[n].data) - pn).max() < 2e-7, (step, n)
                assert np.abs(pn - P0[n]).max() > 0.1 * lr, (step, n)
            assert not host(opt._accum[id(model)])[_pads(model)].any()
    finally:
        parallel.set_accumulated_count(None)
    stats = opt.grad_stats()
    assert stats['steps'] == 3 and opt._step == 3 and stats['skipped'] == 0
    model.check_health()


# ------------------------------------------------------------------------------------------------ script level
def test_audio_clf_train_with_accum_steps_equals_the_recorded_big_batches():
    """batch_size 4, accum_steps 2 over the fixture's 15 training rows: micro-batches 4, 4, 4, 3 = the fixture's batches of 8 and 7."""
    g = load_golden('audio_clf_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    assert int(g['batch_size']) == 8 and len(g['train_idxs']) == 15
    m = audio_gru_whole
    saved_cfg = dict(m.config)
    try:
        m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, batch_size=4, accum_steps=2, learning_rate=float(g['lr']))
        m.audio_features = g['feats']; m.audio_targets = g['targs']
        m.model = m.AudioBiLSTM(m.config, seed=0)
        m.model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
        m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate'], accumulate_steps=m.config.get('accum_steps', 1))
        m.criterion = nn.CrossEntropyLoss()
        tr = g['train_idxs'].tolist()
        quiet(m.train, 1, tr); acc1 = m.train_acc
        quiet(m.train, 2, tr); acc2 = m.train_acc
        assert [acc1, acc2] == g['train_acc'].tolist()
        assert m.optimizer._step == 4 and m.optimizer.pending == 0                    # two updates per epoch
        assert parallel.loss_count(3) == 3                                            # the declared count was cleared
        sd = m.model.state_dict()
        for k, v in g['after'].items():
            assert np.abs(sd[k].cpu().numpy() - v).max() < 5e-5 + 2e-4 * np.abs(v).max(), k
    finally:
        m.config.clear(); m.config.update(saved_cfg)
        parallel.set_accumulated_count(None)


def test_audio_reg_train_with_accum_steps_equals_the_recorded_big_batches():
    """batch_size 2, accum_steps 2 over 11 rows: micro-batches 2, 2, 2, 2, 2, 1 = the fixture's batches of 4, 4, 3 (the last group is
    flushed); the predictions are stored per micro-batch."""
    g = load_golden('audio_reg_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    assert int(g['batch_size']) == 4
    m = audio_bilstm_perm
    saved_cfg = dict(m.config)
    try:
        m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, batch_size=2, accum_steps=2, learning_rate=float(g['lr']))
        m.audio_features = g['feats']; m.audio_targets = g['targs']
        m.model = m.AudioBiLSTM(m.config, seed=0)
        m.model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
        m.optimizer = nn.Adam(m.model.parameters(), lr=m.config['learning_rate'], accumulate_steps=m.config.get('accum_steps', 1))
        m.criterion = nn.L1Loss()
        m.train_dep_idxs = [0, 1, 2, 3, 4]; m.train_non_idxs = [5, 6, 7, 8, 9, 10]
        mae1 = quiet(m.train, 1); mae2 = quiet(m.train, 2)
        assert np.abs(np.array([mae1, mae2]) - g['train_mae']).max() < 1e-3
        assert m.optimizer._step == 6 and m.optimizer.pending == 0
        sd = m.model.state_dict()
        for k, v in g['after'].items():
            if sd[k].dtype.is_floating_point:
                assert np.abs(sd[k].cpu().numpy() - v).max() < 5e-5 + 2e-4 * np.abs(v).max(), k
    finally:
        m.config.clear(); m.config.update(saved_cfg)
        parallel.set_accumulated_count(None)


# ------------------------------------------------------------------------------------------------ launch sequence
def _step_kernels(opt_kw, n_logged):
    """Kernel lists of `n_logged` consecutive optimizer.step() calls (each behind a forward and a backward), after a warm-up of one full group."""
    mod, model, g = _tiny('audio')
    opt = nn.AdamW(mod.get_param_group(model), lr=1e-4, **opt_kw)
    crit = nn.CrossEntropyLoss()
    model.train()

    def fwd_bwd():
        opt.zero_grad(); crit(model(g['x']), g['y']).backward()
    for _ in range(opt.accumulate_steps):
        fwd_bwd(); opt.step()
    out = []
    for _ in range(n_logged):
        fwd_bwd()
        out.append(_kernels_logged(opt.step))
    return out


def test_which_kernels_launch_when():
    (plain,) = _step_kernels({}, 1)
    (k1,) = _step_kernels({'accumulate_steps': 1}, 1)
    assert k1 == plain and not any(ACCUM_KERNEL in k for k in plain)        # the default path: the same launches, no accumulate kernel
    n_adam = sum('adam_kernel' in k for k in plain)
    assert n_adam == 2 and len(plain) == n_adam
    first, boundary = _step_kernels({'accumulate_steps': 2}, 2)
    assert len(first) == 1 and ACCUM_KERNEL in first[0]                      # one accumulate launch, no update
    assert len(boundary) == 1 + n_adam and ACCUM_KERNEL in boundary[0] and all('adam_kernel' in k for k in boundary[1:])
    first, boundary = _step_kernels({'accumulate_steps': 2, 'max_grad_norm': 1.0}, 2)
    assert len(first) == 1 and ACCUM_KERNEL in first[0]
    assert not any('grad_sqnorm_kernel' in k for k in boundary)              # the boundary accumulate left the partials
    assert len(boundary) == 1 + n_adam and ACCUM_KERNEL in boundary[0] and all('adam_clipped_kernel' in k for k in boundary[1:])
    (clipped,) = _step_kernels({'max_grad_norm': 1.0}, 1)
    assert len(boundary) == len(clipped)                                     # an accumulated clipped update costs no more launches than a plain clipped step


def test_native_communicator_reduces_the_accumulator_between_the_last_accumulate_and_the_update():
    """The boundary collective on the C-ABI's RCCL path, with the one-rank communicator a single GPU allows (as tests/test_dp_gpu.py uses it):
    last accumulate -> ONE collective over the live bucket -> join -> optimizer step (dep_grad_sqnorm on the reduced accumulator, then the
    clipped updates); no collective on the other micro-steps or in a backward.  A one-rank SUM is the identity and the accumulate's partials are
    dep_grad_sqnorm's, so the parameters must equal the run without a communicator BIT FOR BIT."""
    def run(native):
        mod, model, g = _tiny('audio')
        opt = nn.AdamW(mod.get_param_group(model), lr=1e-4, max_grad_norm=1e-3, accumulate_steps=2)
        crit = nn.CrossEntropyLoss()
        model.train()
        x, y = g['x'], g['y']
        parallel.set_accumulated_count(x.shape[0])
        L.order_log_enable(True)
        try:
            for _ in range(2):
                for a, b in ((0, 3), (3, 4)):
                    opt.zero_grad(); crit(model(x[a:b]), y[a:b]).backward(); opt.step()
            torch.cuda.synchronize()
            log = L.order_log_read(reset=True)
        finally:
            L.order_log_enable(False)
            parallel.set_accumulated_count(None)
        model.check_health()
        return {k: host(v).copy() for k, v in model.state_dict().items()}, log, model._n_live

    sd0, log0, n_live = run(False)
    assert not any(e.startswith('C ') for e in log0)
    assert parallel.init_native_comm(force_single=True) is not None
    try:
        sd1, log1, _ = run(True)
    finally:
        parallel.destroy_native_comm()
    for k in sd0:
        assert sd0[k].tobytes() == sd1[k].tobytes(), k
    kinds = []
    for e in log1:
        if e.startswith('K ') and ACCUM_KERNEL in e: kinds.append('a')
        elif e.startswith('K ') and 'grad_sqnorm_kernel' in e: kinds.append('s')
        elif e.startswith('K ') and 'adam_clipped_kernel' in e: kinds.append('u')
        elif e.startswith('C '): kinds.append('c'); assert e == 'C allreduce n=%d' % n_live, e
        elif e.startswith('N join'): kinds.append('j')
        elif e.startswith('N optimizer step'): kinds.append('o')
        elif e.startswith('N backward begin'): kinds.append('b')
    assert ''.join(kinds) == 'babacjosuu' * 2, ''.join(kinds)       # per group: (backward, accumulate) x 2, collective, join, step: norm, two updates


# ------------------------------------------------------------------------------------------------ data parallel
def _run_rank(rank, world, port, q, backend):
    # backend 'nccl': one rank per GPU over the C-ABI's RCCL communicator; 'gloo': the ranks share cuda:0 (as tests/test_dp_gpu.py runs them)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank) if backend == 'nccl' else '0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    sys.path.insert(0, ROOT)
    from icassp2022_depression_amd import _lib as L, audio_gru_whole as m, nn, parallel
    if backend == 'nccl':
        torch.cuda.set_device(rank)
    if world > 1:
        parallel.init_from_env(backend)
    g = load_golden('audio_clf_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, batch_size=5, accum_steps=2, learning_rate=float(g['lr']))
    m.audio_features = g['feats']; m.audio_targets = g['targs']
    m.model = m.AudioBiLSTM(m.config, seed=0)
    m.model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
    m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate'], max_grad_norm=1e-3,
                           accumulate_steps=m.config['accum_steps'])
    m.criterion = nn.CrossEntropyLoss()
    L.order_log_enable(True)
    with contextlib.redirect_stdout(io.StringIO()):
        m.train(1, list(range(17)))                  # micro-batches 5, 5, 5, 2 -> groups of 10 and 7 rows: two updates
    torch.cuda.synchronize()
    log = L.order_log_read(reset=True)
    L.order_log_enable(False)
    # gradient collectives: `C ...` from the native communicator, a `C ...` note in front of a torch.distributed all-reduce
    colls = [e for e in log if e.startswith('C ') or e.startswith('N C ')]
    q.put((rank, {k: v.cpu().numpy() for k, v in m.model.state_dict().items()}, colls, m.optimizer.grad_stats(), int(m.train_acc)))
    if world > 1:
        parallel.barrier()
        parallel.destroy_native_comm()
        import torch.distributed as dist
        dist.destroy_process_group()


def _spawn(world, backend, port):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_rank, args=(r, world, port, q, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r, rest) for r, *rest in (q.get(timeout=240) for _ in range(world)))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize('backend', ['gloo', 'nccl'])
def test_two_ranks_exchange_the_accumulator_once_per_update(backend):
    """The gradient exchange is deferred to the update: each rank's order log holds ONE gradient collective per group (two groups here),
    not one per micro-batch (four); the replicas stay bit-identical (the norm of the clipped update is taken from the reduced sums)
    and equal the single-process run with the same settings."""
    if backend == 'nccl' and torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs (a multi-GPU driver box)')
    port = 25200 + os.getpid() % 1000 + 2 * (backend == 'nccl')
    (sd1, colls1, st1, acc1), = _spawn(1, 'gloo', port).values()
    assert colls1 == [] and st1['steps'] == 2
    res = _spawn(2, backend, port + 1)
    (sd_a, colls_a, st_a, acc_a), (sd_b, colls_b, st_b, acc_b) = res[0], res[1]
    assert len(colls_a) == 2 and len(colls_b) == 2, (colls_a, colls_b)
    assert st_a == st_b and st_a['steps'] == 2 and st_a['clipped'] >= 1
    assert acc_a == acc_b == acc1
    for k in sd_a:
        assert sd_a[k].tobytes() == sd_b[k].tobytes(), k
        assert np.abs(sd1[k] - sd_a[k]).max() < 2e-6, k
