"""dep_adam_step_ext (AMSGrad, the fused average of the parameters), dep_swap and the optimizer / checkpoint surface over them, on the
device.  The kernels are held to the float64 yardstick of optim_ext_ref.py (pinned against torch in test_optim_ext_cpu.py) within the
bounds derived there; everything that can be an equality of bits is one: the neutral struct against dep_adam_step /
dep_adam_step_clipped, AMSGrad on a sequence whose v never decreases against the plain step, ema_first and a decay of zero against the
stored parameter, a skipped step, the exchange, the resumed run against the uninterrupted one.
"""
import contextlib
import ctypes as C
import glob
import io
import os

import numpy as np
import pytest

import optim_ext_ref as X
from clip_ref import clip_coef, sqnorm
from conftest import load_golden

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _common, _lib as L, nn
    DEV = torch.device('cuda:0')

F32 = np.float32
LR, B1, B2, EPS = X.LR, X.B1, X.B2, X.EPS
SIZES = [1, 255, 256, 257, 2047, 2048, 2049, 100003]       # the 256-thread edge, the clipped kernels' 2048-element workgroup, an odd tail
DECAYS = [(True, 1e-2), (False, 0.0), (False, 1e-3)]
NEW_KERNELS = ('adam_ext_kernel', 'adam_clipped_ext_kernel', 'swap_kernel')


def dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def words(t):
    """The tensor's 32-bit words on the host: equality of bits, NaNs included."""
    return host(t).view(np.uint32)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def slots():
    return torch.empty(L.grad_norm_slots(), dtype=torch.float64, device=DEV)


# ------------------------------------------------------------------------------------------------ parity with the float64 reference
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('clipped', [False, True])
@pytest.mark.parametrize('amsgrad,d', [(True, None), (False, 0.9), (True, 0.9)])
@pytest.mark.parametrize('decoupled,wd', DECAYS)
def test_twenty_steps_against_the_reference(n, clipped, amsgrad, d, decoupled, wd):
    """p, m, v, vmax and the average after 20 steps of the shrinking gradient sequence, both launch forms (the clipped one with the
    global norm of each step's own gradient against max_norm 1); bounds: optim_ext_ref."""
    wd = float(F32(wd))
    rng = np.random.default_rng(10 * n + int(decoupled))
    p0 = X.r32(rng.uniform(-0.4, 0.4, n))
    grads = X.shrinking_gradients(n, X.STEPS, n + 1)
    ref, _ = X.run(p0, grads, amsgrad, d, wd=wd, decoupled=decoupled, max_norm=1.0 if clipped else None)
    pd, md, vd = dev(p0), dev(np.zeros(n)), dev(np.zeros(n))
    vmax = dev(np.zeros(n)) if amsgrad else None
    ema = dev(np.full(n, np.nan)) if d is not None else None
    part = slots()
    for k, g in enumerate(grads, 1):
        gd = dev(g)
        if clipped:
            L.grad_sqnorm([gd], part)
        L.adam_step_ext(pd, gd, md, vd, LR, B1, B2, EPS, wd, decoupled, k, vmax=vmax, ema=ema, ema_decay=d or 0.0, ema_first=k == 1,
                        partials=part if clipped else None, max_norm=1.0)
    assert np.abs(ref['p']).max() < 0.5
    assert np.abs(host(pd) - ref['p']).max() < X.P_TOL
    assert relerr(host(md), ref['m']) < X.M_TOL
    assert relerr(host(vd), ref['v']) < X.V_TOL
    if amsgrad:
        assert (ref['vmax'] > ref['v']).any() or n == 1
        assert relerr(host(vmax), ref['vmax']) < X.V_TOL
    if d is not None:
        assert np.abs(host(ema) - ref['ema']).max() < X.EMA_TOL
        assert np.abs(ref['ema'] - ref['p']).max() > 10 * X.EMA_TOL or n == 1       # the average is not the parameter


# ------------------------------------------------------------------------------------------------ neutral bits
def _raw_ext(p, g, m, v, k, wd, decoupled, ext, part=None, max_norm=1.0):
    L.check(L.load().dep_adam_step_ext(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), LR, B1, B2, EPS, wd, int(decoupled), k,
                                       ext, None if part is None else part.data_ptr(), max_norm, 0, None, None, L.stream()), 'dep_adam_step_ext')


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('clipped', [False, True])
def test_neutral_struct_gives_the_old_entry_points_bits(n, clipped):
    rng = np.random.default_rng(n)
    p0 = rng.uniform(-0.4, 0.4, n).astype(F32)
    grads = [rng.standard_normal(n).astype(F32) for _ in range(3)]
    part = slots()
    runs = {}
    for how in ('old', 'null', 'empty'):
        p, m, v = dev(p0), dev(np.zeros(n)), dev(np.zeros(n))
        for k, g in enumerate(grads, 1):
            gd = dev(g)
            if clipped:
                L.grad_sqnorm([gd], part)
            if how == 'old' and clipped:
                L.adam_step_clipped(p, gd, m, v, LR, B1, B2, EPS, 1e-2, True, k, part, 1.0)
            elif how == 'old':
                L.adam_step(p, gd, m, v, LR, B1, B2, EPS, 1e-2, True, k)
            else:
                ext = None if how == 'null' else C.byref(L.AdamExt(None, None, 0.5, 1))
                _raw_ext(p, gd, m, v, k, 1e-2, True, ext, part if clipped else None)
        runs[how] = [words(t) for t in (p, m, v)]
    for how in ('null', 'empty'):
        for a, b in zip(runs['old'], runs[how]):
            assert np.array_equal(a, b), how


@pytest.mark.parametrize('clipped', [False, True])
def test_amsgrad_equals_the_plain_step_while_v_never_decreases(clipped):
    n = 2049
    rng = np.random.default_rng(5)
    p0 = rng.uniform(-0.4, 0.4, n).astype(F32)
    grads = X.growing_gradients(n, X.STEPS, 6)
    part = slots()
    p, m, v = dev(p0), dev(np.zeros(n)), dev(np.zeros(n))
    q, mq, vq, vmax = dev(p0), dev(np.zeros(n)), dev(np.zeros(n)), dev(np.zeros(n))
    for k, g in enumerate(grads, 1):
        gd = dev(g)
        if clipped:
            L.grad_sqnorm([gd], part)
            L.adam_step_clipped(p, gd, m, v, LR, B1, B2, EPS, 1e-3, False, k, part, 1.0)
        else:
            L.adam_step(p, gd, m, v, LR, B1, B2, EPS, 1e-3, False, k)
        before = host(vq).copy()
        L.adam_step_ext(q, gd, mq, vq, LR, B1, B2, EPS, 1e-3, False, k, vmax=vmax, partials=part if clipped else None, max_norm=1.0)
        assert (host(vq) >= before).all()                                           # the condition on the inputs
    for a, b in ((p, q), (m, mq), (v, vq), (v, vmax)):
        assert np.array_equal(words(a), words(b))


# ------------------------------------------------------------------------------------------------ the average
@pytest.mark.parametrize('n', [1, 257, 2049])
@pytest.mark.parametrize('how', ['first', 'zero decay'])
def test_first_update_and_zero_decay_store_the_parameter_without_reading_the_average(n, how):
    rng = np.random.default_rng(n)
    p, g = dev(rng.uniform(-0.4, 0.4, n)), dev(rng.standard_normal(n))
    m, v, ema = dev(np.zeros(n)), dev(np.zeros(n)), dev(np.full(n, np.nan))
    L.adam_step_ext(p, g, m, v, LR, B1, B2, EPS, 1e-2, True, 1, ema=ema, ema_decay=0.9 if how == 'first' else 0.0, ema_first=how == 'first')
    assert np.array_equal(words(ema), words(p)) and not np.isnan(host(p)).any()


@pytest.mark.parametrize('n', [1, 257, 100003])
@pytest.mark.parametrize('clipped', [False, True])
def test_nothing_to_do_leaves_every_buffer_alone(n, clipped):
    """Zero gradient, zero moments, no decay, average equal to the parameter: p - step * (0 / eps) is p, and ema + w * 0 is ema."""
    rng = np.random.default_rng(n)
    p0 = rng.uniform(-2, 2, n).astype(F32)
    zero = np.zeros(n, F32)
    p, g, m, v, vmax, ema = dev(p0), dev(zero), dev(zero), dev(zero), dev(zero), dev(p0)
    part = slots()
    if clipped:
        L.grad_sqnorm([g], part)
    L.adam_step_ext(p, g, m, v, LR, B1, B2, EPS, 0.0, False, 1, vmax=vmax, ema=ema, ema_decay=0.9, partials=part if clipped else None, max_norm=1.0)
    for t, want in ((p, p0), (ema, p0), (m, zero), (v, zero), (vmax, zero)):
        assert np.array_equal(words(t), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ skipped step
@pytest.mark.parametrize('n', [257, 2049])
def test_skipped_step_leaves_all_five_buffers_bit_identical(n):
    rng = np.random.default_rng(n)
    arrs = [rng.uniform(0.1, 0.4, n).astype(F32) for _ in range(5)]
    p, m, v, vmax, ema = (dev(a) for a in arrs)
    g = rng.standard_normal(n).astype(F32); g[n // 2] = np.inf
    gd, part = dev(g), slots()
    clip_out, stats = torch.zeros(4, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)
    L.grad_sqnorm([gd], part)
    for first in (True, False):
        L.adam_step_ext(p, gd, m, v, LR, B1, B2, EPS, 1e-2, True, 3, vmax=vmax, ema=ema, ema_decay=0.9, ema_first=first, partials=part,
                        max_norm=1.0, skip_nonfinite=True, clip_out=clip_out, stats=stats)
    for t, a in zip((p, m, v, vmax, ema), arrs):
        assert np.array_equal(words(t), a.view(np.uint32))
    assert host(stats).tolist() == [2.0, 0.0, 2.0, 0.0] and host(clip_out)[2] == 0.0


# ------------------------------------------------------------------------------------------------ dep_swap
@pytest.mark.parametrize('n', [1, 255, 256, 257, 100003])
def test_swap_exchanges_bits_and_twice_is_the_identity(n):
    rng = np.random.default_rng(n)
    a0 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)           # every word pattern: NaN payloads, infinities, both zeros
    b0 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    guard = 8                                                                      # the floats behind each range must stay as they are
    a = torch.from_numpy(np.concatenate([a0, np.full(guard, 0xDEADBEEF, np.uint32)]).view(F32)).to(DEV)
    b = torch.from_numpy(np.concatenate([b0, np.full(guard, 0xFEEDF00D, np.uint32)]).view(F32)).to(DEV)
    L.swap(a[:n], b[:n])
    assert np.array_equal(words(a)[:n], b0) and np.array_equal(words(b)[:n], a0)
    assert (words(a)[n:] == 0xDEADBEEF).all() and (words(b)[n:] == 0xFEEDF00D).all()
    L.swap(a[:n], b[:n])
    assert np.array_equal(words(a)[:n], a0) and np.array_equal(words(b)[:n], b0)


# ------------------------------------------------------------------------------------------------ models
B, T, F, H = 4, 5, 8, 16


def _build(name, seed=0):
    from icassp2022_depression_amd import audio_gru_whole, text_bilstm_whole
    mod, cls = {'audio': (audio_gru_whole, 'AudioBiLSTM'), 'text': (text_bilstm_whole, 'TextBiLSTM')}[name]
    cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0, rnn_layers=2)
    model = getattr(mod, cls)(cfg, seed=seed)
    opt = nn.AdamW(mod.get_param_group(model), lr=1e-3, amsgrad=True, ema_decay=0.9, max_grad_norm=1.0)
    return mod, cfg, model, opt


def _batch():
    rng = np.random.default_rng(17)
    return rng.standard_normal((B, T, F)).astype(F32), rng.integers(0, 2, B)


def _steps(model, opt, n):
    x, y = _batch()
    crit = nn.CrossEntropyLoss()
    model.train()
    flats = []
    for _ in range(n):
        opt.zero_grad()
        crit(model(x), y).backward()
        opt.step()
        flats.append(host(model._flat).copy())
    return flats


@pytest.mark.parametrize('name', ['audio', 'text'])
def test_model_average_follows_the_recurrence_and_averaged_exchanges_it(name):
    """Six steps.  The average is the recurrence of optim_ext_ref applied on the host to the parameters read back after each step:
    the first update stores the parameter exactly, each of the five others rounds p - avg (relative 2**-24 of a difference far below
    one) and the result (at most 2**-24 while |avg| < 2, asserted): 6 * 1.1 * 2**-24 = 3.9e-7."""
    mod, cfg, model, opt = _build(name)
    flats = _steps(model, opt, 6)
    ema = opt._ext[id(model)][1]
    want = X.ema_recurrence(flats, 0.9)
    assert np.abs(want).max() < 2.0
    assert np.abs(host(ema) - want).max() < 6 * 1.1 * 2.0 ** -24
    assert np.abs(want - flats[-1]).max() > 1e-4                                    # and it is not the last iterate
    stats = opt.grad_stats()
    assert stats['steps'] == 6 and stats['skipped'] == 0
    x, _ = _batch()
    raw, avg = words(model._flat).copy(), words(ema).copy()
    model.eval()
    with opt.averaged():
        assert np.array_equal(words(model._flat), avg) and np.array_equal(words(ema), raw)
        out = model(x).numpy().copy()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        with pytest.raises(L.DepError):
            opt.step()
    assert np.array_equal(words(model._flat), raw) and np.array_equal(words(ema), avg)
    other = getattr(mod, type(model).__name__)(cfg, seed=5)
    other.load_state_dict(sd)
    other.eval()
    assert np.array_equal(other(x).numpy().view(np.uint32), out.view(np.uint32))
    assert not np.array_equal(model(x).numpy().view(np.uint32), out.view(np.uint32))   # the raw weights answer differently
    model.check_health()


def test_resumed_run_is_bit_identical_to_the_uninterrupted_one(tmp_path):
    _, _, model, opt = _build('audio')
    _steps(model, opt, 6)
    _, _, first, opt1 = _build('audio')
    _steps(first, opt1, 3)
    path = os.path.join(str(tmp_path), 'ckpt')
    with contextlib.redirect_stdout(io.StringIO()):
        _common.save_checkpoint(first, opt1, path)
    _, _, second, opt2 = _build('audio', seed=9)                                    # other initial weights: everything comes from the file
    _common.load_checkpoint(second, opt2, path)
    _steps(second, opt2, 3)
    assert opt2._step == 6 and opt2._ema_updates == 6
    pairs = [(model._flat, second._flat)] + list(zip(opt._state[id(model)] + opt._ext[id(model)], opt2._state[id(second)] + opt2._ext[id(second)]))
    assert len(pairs) == 5
    for a, b in pairs:
        assert np.array_equal(words(a), words(b))


# ------------------------------------------------------------------------------------------------ launch sequence
def _kernels_of_a_step(opt_kw):
    from icassp2022_depression_amd import audio_gru_whole as mod
    g = load_golden('audio_clf_tiny')
    _, _, F_, H_ = [int(v) for v in g['shape']]
    cfg = dict(mod.config); cfg.update(embedding_size=F_, hidden_dims=H_, dropout=0.0)
    model = mod.AudioBiLSTM(cfg, seed=0)
    opt = nn.AdamW(mod.get_param_group(model), lr=1e-4, **opt_kw)
    crit = nn.CrossEntropyLoss()
    model.train()

    def step():
        opt.zero_grad(); crit(model(g['x']), g['y']).backward(); opt.step()
    step(); torch.cuda.synchronize()
    L.order_log_enable(True)
    try:
        step(); torch.cuda.synchronize()
        log = L.order_log_read(reset=True)
    finally:
        L.order_log_enable(False)
    return [e[2:] for e in log if e.startswith('K ')]


def test_default_step_launches_what_it_launched_and_the_options_add_no_launch():
    plain = _kernels_of_a_step({})
    assert not [k for k in plain if any(n in k for n in NEW_KERNELS)], plain
    assert sum('adam_kernel' in k for k in plain) == 2                              # the two weight-decay groups
    strip = lambda ks: [k for k in ks if 'adam' not in k and 'grad_sqnorm' not in k]
    for kw in ({'ema_decay': 0.9}, {'amsgrad': True}, {'amsgrad': True, 'ema_decay': 0.9}):
        on = _kernels_of_a_step(kw)
        assert len(on) == len(plain) and sum('adam_ext_kernel' in k for k in on) == 2 and not any('adam_kernel' in k for k in on)
        assert strip(on) == strip(plain) and all('adam_ext_kernel' in k for k in on[-2:])
    clipped = _kernels_of_a_step({'max_grad_norm': 1.0})
    on = _kernels_of_a_step({'max_grad_norm': 1.0, 'ema_decay': 0.9})
    assert len(on) == len(clipped) and sum('adam_clipped_ext_kernel' in k for k in on) == 2 and strip(on) == strip(clipped)


# ------------------------------------------------------------------------------------------------ script
def test_script_evaluate_saves_the_averaged_weights(tmp_path, monkeypatch):
    """audio_gru_whole with config['ema_decay']: the checkpoint written through the save gate holds the average, not the raw weights."""
    from icassp2022_depression_amd import audio_gru_whole as m
    g = load_golden('audio_clf_train_eval')
    N, T_, F_, H_ = [int(v) for v in g['shape']]
    saved_cfg = dict(m.config)
    saved = (m.audio_features, m.audio_targets, m.model, m.optimizer, m.criterion, m.prefix, m.train_acc, m.max_f1)
    try:
        m.config.update(embedding_size=F_, hidden_dims=H_, dropout=0.0, batch_size=int(g['batch_size']), learning_rate=float(g['lr']), ema_decay=0.5)
        m.audio_features = g['feats']; m.audio_targets = g['targs']
        m.prefix = str(tmp_path)
        os.makedirs(os.path.join(m.prefix, 'Features/TextWhole'))
        m.model = m.AudioBiLSTM(m.config, seed=0)
        m.model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
        m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate'], max_grad_norm=m.config.get('max_grad_norm'),
                               accumulate_steps=m.config.get('accum_steps', 1), **_common.optim_options(m.config))
        assert m.optimizer.ema_decay == 0.5
        m.criterion = nn.CrossEntropyLoss()
        tr, te = g['train_idxs'].tolist(), g['test_idxs'].tolist()
        monkeypatch.setattr(_common, 'report_prf', lambda cm: (0.9, 0.9, 0.9, 0.9))  # through the save gate whatever the six rows say
        with contextlib.redirect_stdout(io.StringIO()):
            m.train(1, tr); m.train(2, tr)
            m.train_acc = len(tr); m.max_f1 = -1
            raw = words(m.model._flat).copy()
            avg = host(m.optimizer._ext[id(m.model)][1]).copy()
            m.evaluate(m.model, te, 1, tr, tr)
        assert np.array_equal(words(m.model._flat), raw)                           # the raw weights are back
        files = glob.glob(os.path.join(m.prefix, 'Model/ClassificationWhole/Audio/*.pt'))
        assert len(files) == 1
        sd = _common.load_checkpoint_state_dict(files[0])
        moved = 0
        for name, p in m.model.named_parameters():
            want = avg[p.offset:p.offset + p.numel].reshape(p.shape)
            assert np.array_equal(sd[name].numpy().view(np.uint32), want.view(np.uint32)), name
            moved += int(not np.array_equal(host(p.data), want))
        assert moved >= 12                                                          # every trained tensor differs from its average
    finally:
        m.config.clear(); m.config.update(saved_cfg)
        m.audio_features, m.audio_targets, m.model, m.optimizer, m.criterion, m.prefix, m.train_acc, m.max_f1 = saved
