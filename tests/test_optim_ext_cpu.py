"""AMSGrad, the fused average of the parameters and the optimizer checkpoints: the parts that need no GPU.

1. The yardstick of tests/test_optim_ext_gpu.py is pinned: optim_ext_ref.step against torch.optim.Adam / AdamW(amsgrad=True) on float64
   CPU tensors over 20 steps, and its average against torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)) fed the
   same iterates, both within 1e-12 (the bound tests/reg_loss_ref.py is held to).  The gradients shrink a hundredfold after step 5, and
   the reference itself shows the running maximum above v from then on.
2. dep_adam_step_ext and dep_swap refuse bad arguments (DEP_ERR_ARG) before any HIP call.
3. The optimizer's host logic against a recording stand-in of the binding.
4. state_dict() -> load_state_dict() on CPU stand-ins; mismatches raise.
5. The scripts' two config keys.
"""
import ctypes as C
import inspect

import numpy as np
import pytest

import optim_ext_ref as X
from optim_rec import ERR_ARG, _Owner, _params, lib, record_binding  # noqa: F401 -- lib is a fixture

torch = pytest.importorskip('torch')

SCRIPTS = ['audio_gru_whole', 'text_bilstm_whole', 'fuse_net_whole', 'audio_bilstm_perm', 'text_bilstm_perm', 'fuse_net']


# ----------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize('decoupled,wd', [(True, 1e-2), (False, 0.0), (False, 1e-3)])
def test_reference_equals_torch_amsgrad_and_averaged_model(decoupled, wd):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    n, d = 33, 0.9
    rng = np.random.default_rng(3)
    p0 = rng.uniform(-0.4, 0.4, n)
    grads = X.shrinking_gradients(n, X.STEPS, 4)
    mod = torch.nn.Module()
    mod.w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([mod.w], lr=X.LR, betas=(X.B1, X.B2), eps=X.EPS, weight_decay=wd,
                                                                  amsgrad=True)
    avg = AveragedModel(mod, multi_avg_fn=get_ema_multi_avg_fn(d))
    _, trail = X.run(p0, grads, True, d, wd=wd, decoupled=decoupled)
    above = []
    for g, ref in zip(grads, trail):
        mod.w.grad = torch.from_numpy(g.copy())
        opt.step()
        avg.update_parameters(mod)
        st = opt.state[mod.w]
        for mine, theirs in ((ref['p'], mod.w), (ref['m'], st['exp_avg']), (ref['v'], st['exp_avg_sq']),
                             (ref['vmax'], st['max_exp_avg_sq']), (ref['ema'], avg.module.w)):
            assert np.abs(mine - theirs.detach().numpy()).max() < 1e-12
        above.append(bool((ref['vmax'] > ref['v']).any()))
    assert all(above[5:])                                 # a condition on the inputs: the maximum is above v somewhere from step 6 on
    plain, _ = X.run(p0, grads, False, None, wd=wd, decoupled=decoupled)
    assert np.abs(plain['p'] - trail[-1]['p']).max() > 1e-6


def test_reference_average_is_the_recurrence_of_the_iterates():
    grads = X.shrinking_gradients(9, 6, 1)
    st, trail = X.run(np.linspace(-0.3, 0.3, 9), grads, False, 0.75)
    assert np.abs(st['ema'] - X.ema_recurrence([t['p'] for t in trail], 0.75)).max() < 1e-15


# ----------------------------------------------------------------------------------------------- 2. refusals
_P = C.c_void_p
A = 0x10000                      # never dereferenced: every call below is refused before any HIP call


class _Ext(C.Structure):
    _fields_ = [('vmax', _P), ('ema', _P), ('ema_decay', C.c_float), ('ema_first', C.c_int)]


def _ext_call(lib, p=A, g=2 * A, m=3 * A, v=4 * A, n=64, step=1, vmax=None, ema=None, decay=0.9, partials=None, max_norm=1.0):
    ext = _Ext(vmax, ema, decay, 0)
    return lib.dep_adam_step_ext(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, step, C.byref(ext), partials, max_norm, 0, None, None, None)


def test_adam_step_ext_refuses_what_the_old_entries_refuse(lib):
    for kw in ({'p': None}, {'g': None}, {'m': None}, {'v': None}, {'n': 0}, {'n': -5}, {'step': 0}):
        assert _ext_call(lib, vmax=5 * A, **kw) == ERR_ARG, kw
        assert _ext_call(lib, **kw) == ERR_ARG, kw                                  # the neutral struct too
    assert _ext_call(lib, vmax=5 * A, partials=6 * A, max_norm=float('nan')) == ERR_ARG
    assert lib.dep_adam_step_ext(None, 2 * A, 3 * A, 4 * A, 64, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1, None, None, 0.0, 0, None, None, None) == ERR_ARG
    assert b'bad argument' in lib.dep_last_error()


@pytest.mark.parametrize('decay', [float('nan'), 1.0, 1.5, -0.1, float('inf')])
def test_adam_step_ext_refuses_a_decay_outside_the_half_open_interval(lib, decay):
    assert _ext_call(lib, ema=5 * A, decay=decay) == ERR_ARG
    assert _ext_call(lib, ema=5 * A, decay=decay, partials=6 * A) == ERR_ARG


def test_adam_step_ext_refuses_aliasing(lib):
    n = 64
    for other in (A, 3 * A, 4 * A):                                                 # p, m, v
        for shift in (0, 4 * (n - 1), -4 * (n - 1)):                                # the same range, and one float of overlap at either end
            assert _ext_call(lib, vmax=other + shift, n=n) == ERR_ARG
            assert _ext_call(lib, ema=other + shift, n=n) == ERR_ARG
    assert _ext_call(lib, vmax=5 * A, ema=5 * A, n=n) == ERR_ARG                     # and each other


def test_swap_refuses(lib):
    for a, b, n in ((None, A, 8), (A, None, 8), (A, 2 * A, 0), (A, 2 * A, -1), (A + 4, 2 * A, 8), (A, 2 * A + 8, 8), (A, A, 8),
                    (A, A + 16, 8), (A + 16, A, 8)):
        assert lib.dep_swap(a, b, n, None) == ERR_ARG, (a, b, n)


# ----------------------------------------------------------------------------------------------- 3. host logic
def _recording(monkeypatch):
    """record_binding plus the two new entry points: ('ext', p pointer, elements, keywords) and ('swap', a pointer, b pointer); the
    stand-ins of grad_accumulate and swap also DO what the launches do, on the host tensors, so that state can be followed."""
    nn, log, names = record_binding(monkeypatch, adam_logs_p=False)

    def accumulate(acc, g, scale=1.0, first=False, partials=None):
        log.append(('accum', [t.data_ptr() for t in acc], [t.data_ptr() for t in g], scale, first, partials))
        for a, x in zip(acc, g):
            a.copy_(x * scale if first else a + x * scale)

    def swap(a, b):
        log.append(('swap', a.data_ptr(), b.data_ptr()))
        t = a.clone(); a.copy_(b); b.copy_(t)

    monkeypatch.setattr(nn.L, 'grad_accumulate', accumulate)
    monkeypatch.setattr(nn.L, 'swap', swap)
    monkeypatch.setattr(nn.L, 'adam_step_ext', lambda p, g, m, v, *a, **kw: log.append(('ext', p.data_ptr(), p.numel(), a, kw)))
    return nn, log


def _two_groups(nn, n_dead=0):
    """One owner, two groups over [8 | 12 (| dead 4)] floats: two ranges per update."""
    owner = _Owner(20 + n_dead, 20)
    owner._flat.copy_(torch.arange(20 + n_dead, dtype=torch.float32))
    ps = _params(nn, owner, [8, 12] + ([n_dead] if n_dead else []), dead=(2,) if n_dead else ())
    return owner, [{'params': ps[:1], 'weight_decay': 0.0}, {'params': ps[1:]}]


def test_default_optimizer_records_only_the_old_entries(monkeypatch):
    nn, log = _recording(monkeypatch)
    _, groups = _two_groups(nn)
    opt = nn.AdamW(groups, lr=1e-3)
    opt.step(); opt.step()
    assert [e[0] for e in log] == ['adam'] * 4
    del log[:]
    opt = nn.AdamW(groups, lr=1e-3, max_grad_norm=1.0)
    opt.step()
    assert [e[0] for e in log] == ['sqnorm', 'clipped', 'clipped']
    with pytest.raises(nn.L.DepError):
        with opt.averaged():
            pass


@pytest.mark.parametrize('kw', [{'amsgrad': True}, {'ema_decay': 0.9}, {'amsgrad': True, 'ema_decay': 0.9}])
@pytest.mark.parametrize('clip', [False, True])
def test_an_option_records_one_ext_entry_per_range(monkeypatch, kw, clip):
    nn, log = _recording(monkeypatch)
    owner, groups = _two_groups(nn, n_dead=4)
    opt = nn.AdamW(groups, lr=1e-3, **kw, **({'max_grad_norm': 1.0, 'skip_nonfinite': True} if clip else {}))
    for _ in range(3):
        opt.step()
    copies = [e for e in log if e[0] == 'accum']
    steps = [e for e in log if e[0] != 'accum']
    assert len(copies) == (1 if 'ema_decay' in kw else 0)                           # the average's initial copy, once, through the library
    assert [e[0] for e in steps] == ((['sqnorm'] if clip else []) + ['ext', 'ext']) * 3
    ext = [e for e in steps if e[0] == 'ext']
    assert [(e[1] - owner._flat.data_ptr(), e[2]) for e in ext] == [(0, 8), (32, 12)] * 3
    assert [e[4]['ema_first'] for e in ext] == [True, True] + [False] * 4           # true for the first UPDATE (both of its ranges)
    for i, e in enumerate(ext):
        k = e[4]
        assert (k['vmax'] is not None) == ('amsgrad' in kw) and (k['ema'] is not None) == ('ema_decay' in kw)
        assert k['ema_decay'] == kw.get('ema_decay', 0.0)
        assert (k['partials'] is not None) == clip and k['skip_nonfinite'] == clip
        assert (k['stats'] is not None) == (clip and i % 2 == 0) and (k['clip_out'] is not None) == (clip and i % 2 == 0)
        assert e[3][-1] == i // 2 + 1                                               # the step count
    if 'ema_decay' in kw:                                                           # laid out like _flat, dead parameters included
        ema = opt._ext[id(owner)][1]
        assert ema.numel() == 24 and torch.equal(ema, owner._flat)
        assert ext[1][4]['ema'].data_ptr() - ema.data_ptr() == 32 and ext[1][4]['ema'].numel() == 12


def test_micro_steps_record_no_ext_entry(monkeypatch):
    nn, log = _recording(monkeypatch)
    _, groups = _two_groups(nn)
    opt = nn.AdamW(groups, lr=1e-3, ema_decay=0.9, accumulate_steps=3)
    opt.step(); opt.step()
    assert [e[0] for e in log] == ['accum', 'accum']
    opt.step()
    assert [e[0] for e in log] == ['accum'] * 3 + ['accum', 'ext', 'ext']            # the third: accumulate, the average's copy, the update
    assert [e[4]['ema_first'] for e in log[-2:]] == [True, True]
    opt.step(); opt.flush()
    assert [e[0] for e in log[6:]] == ['accum', 'ext', 'ext'] and not log[-1][4]['ema_first']


def test_averaged_swaps_twice_per_owner_and_refuses_updates_inside(monkeypatch):
    nn, log = _recording(monkeypatch)
    a, b = _Owner(8), _Owner(12)
    a._flat.fill_(1.0); b._flat.fill_(2.0)
    opt = nn.Adam(_params(nn, a, [8]) + _params(nn, b, [12]), ema_decay=0.5, accumulate_steps=1)
    opt.step()
    ema_a, ema_b = opt._ext[id(a)][1], opt._ext[id(b)][1]
    ema_a.fill_(10.0); ema_b.fill_(20.0)
    del log[:]
    with pytest.raises(KeyError):
        with opt.averaged():
            assert a._flat[0] == 10.0 and b._flat[0] == 20.0 and ema_a[0] == 1.0
            for what in (opt.step, opt.flush, opt.state_dict, lambda: opt.averaged().__enter__()):
                with pytest.raises(nn.L.DepError):
                    what()
            raise KeyError('leaves through an exception')
    assert [e[0] for e in log] == ['swap'] * 4
    assert [e[1] for e in log] == [a._flat.data_ptr(), b._flat.data_ptr()] * 2
    assert a._flat[0] == 1.0 and b._flat[0] == 2.0 and ema_a[0] == 10.0 and ema_b[0] == 20.0
    opt.step()                                                                      # usable again
    assert log[-1][0] == 'ext'


# ----------------------------------------------------------------------------------------------- 4. round trip
def _built(nn, **kw):
    owner, groups = _two_groups(nn, n_dead=4)
    return owner, nn.AdamW(groups, lr=2e-3, betas=(0.8, 0.99), **kw)


def test_state_dict_round_trip(monkeypatch):
    nn, log = _recording(monkeypatch)
    owner, opt = _built(nn, amsgrad=True, ema_decay=0.9)
    opt.step(); opt.step()
    m, v = opt._state[id(owner)]
    vmax, ema = opt._ext[id(owner)]
    for i, t in enumerate((m, v, vmax, ema)):
        t.copy_(torch.arange(t.numel(), dtype=torch.float32) + 100 * i)
    sd = opt.state_dict()
    assert sd['step'] == 2 and sd['ema_updates'] == 2 and sd['amsgrad'] is True and sd['ema_decay'] == 0.9
    assert [g['weight_decay'] for g in sd['param_groups']] == [0.0, 1e-2] and sd['param_groups'][0]['betas'] == (0.8, 0.99)
    import io
    buf = io.BytesIO(); torch.save(sd, buf); buf.seek(0)
    sd = torch.load(buf, weights_only=True)                                         # tensors and plain numbers only
    owner2, groups2 = _two_groups(nn, n_dead=4)
    opt2 = nn.AdamW(groups2, lr=5.0, amsgrad=True, ema_decay=0.5)
    opt2.load_state_dict(sd)
    for mine, theirs in zip(opt2._state[id(owner2)] + opt2._ext[id(owner2)], (m, v, vmax, ema)):
        assert torch.equal(mine, theirs) and mine.data_ptr() != theirs.data_ptr()
    assert opt2._step == 2 and opt2._ema_updates == 2 and opt2.ema_decay == 0.9
    assert [(g['lr'], g['betas'], g['eps'], g['weight_decay']) for g in opt2.param_groups] == \
        [(g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']) for g in opt.param_groups]
    del log[:]
    opt2.step()
    assert [e[0] for e in log] == ['ext', 'ext'] and not log[0][4]['ema_first'] and log[0][3][-1] == 3     # no second copy, no second first
    again = opt2.state_dict()
    assert again['step'] == 3 and torch.equal(again['state'][0]['ema'], sd['state'][0]['ema'])


def test_state_dict_of_a_default_optimizer_and_before_any_step(monkeypatch):
    nn, _ = _recording(monkeypatch)
    owner, opt = _built(nn)
    sd = opt.state_dict()
    assert sd['step'] == 0 and sd['state'][0] == {'numel': 24, 'm': None, 'v': None, 'vmax': None, 'ema': None}
    opt.step()
    sd = opt.state_dict()
    assert sd['state'][0]['m'].numel() == owner._flat_grad.numel() and sd['state'][0]['vmax'] is None and sd['state'][0]['ema'] is None
    _, opt2 = _built(nn)
    opt2.load_state_dict(sd)
    assert opt2._step == 1 and not opt2._ext


def test_load_state_dict_names_the_mismatch(monkeypatch):
    nn, _ = _recording(monkeypatch)
    _, opt = _built(nn, amsgrad=True, ema_decay=0.9)
    opt.step()
    sd = opt.state_dict()
    with pytest.raises(ValueError, match='amsgrad'):
        _built(nn, ema_decay=0.9)[1].load_state_dict(sd)
    with pytest.raises(ValueError, match='ema_decay'):
        _built(nn, amsgrad=True)[1].load_state_dict(sd)
    with pytest.raises(ValueError, match='ema_decay'):
        opt.load_state_dict(_built(nn, amsgrad=True)[1].state_dict())
    owner = _Owner(28, 24)
    other = nn.AdamW([{'params': _params(nn, owner, [8, 16])}], amsgrad=True, ema_decay=0.9)
    with pytest.raises(ValueError, match='sizes'):
        other.load_state_dict(sd)
    adam = nn.Adam(_two_groups(nn, n_dead=4)[1], amsgrad=True, ema_decay=0.9)
    with pytest.raises(ValueError, match='AdamW'):
        adam.load_state_dict(sd)
    bad = dict(sd, state=[dict(sd['state'][0], vmax=torch.zeros(7))])
    with pytest.raises(ValueError, match='vmax'):
        _built(nn, amsgrad=True, ema_decay=0.9)[1].load_state_dict(bad)


def test_state_dict_refuses_the_middle_of_an_accumulation_group(monkeypatch):
    nn, _ = _recording(monkeypatch)
    _, opt = _built(nn, ema_decay=0.9, accumulate_steps=2)
    opt.step()
    with pytest.raises(nn.L.DepError, match='accumulation'):
        opt.state_dict()
    opt.step()
    assert opt.state_dict()['step'] == 1


def test_constructor_refuses_a_bad_decay(monkeypatch):
    nn, _ = _recording(monkeypatch)
    for d in (1.0, -0.5, float('nan')):
        with pytest.raises(ValueError):
            nn.Adam(_two_groups(nn)[1], ema_decay=d)


# ----------------------------------------------------------------------------------------------- 5. scripts
@pytest.mark.parametrize('name', SCRIPTS)
def test_script_config_keys(name):
    import importlib
    from icassp2022_depression_amd import _common
    mod = importlib.import_module('icassp2022_depression_amd.' + name)
    cfg = dict(mod.config)
    assert _common.optim_options(cfg) == {}                                         # absent: the optimizer is built as it always was
    assert _common.optim_options(dict(cfg, amsgrad=False, ema_decay=None)) == {}
    assert _common.optim_options(dict(cfg, amsgrad=True)) == {'amsgrad': True}
    assert _common.optim_options(dict(cfg, amsgrad=True, ema_decay=0.99)) == {'amsgrad': True, 'ema_decay': 0.99}
    for bad in ({'ema_decay': 1.0}, {'ema_decay': -0.1}, {'ema_decay': 'yes'}, {'ema_decay': True}, {'amsgrad': 1}):
        with pytest.raises(ValueError):
            _common.optim_options(dict(cfg, **bad))
    assert '**_common.optim_options(config)' in inspect.getsource(mod)              # read where the optimizer is built
    assert hasattr(mod.evaluate, '__wrapped__') and mod.evaluate.__name__ == 'evaluate'


def test_evaluate_runs_inside_averaged_only_with_an_average():
    from icassp2022_depression_amd import _common
    import contextlib
    seen = []

    class Opt:
        def __init__(self, d):
            self.ema_decay = d

        @contextlib.contextmanager
        def averaged(self):
            seen.append('in'); yield; seen.append('out')

    holder = {'opt': None}
    fn = _common.on_averaged_weights(lambda: holder['opt'])(lambda x: seen.append(x) or x + 1)
    assert fn(1) == 2 and seen == [1]
    holder['opt'] = Opt(None)
    assert fn(2) == 3 and seen == [1, 2]
    holder['opt'] = Opt(0.9)
    assert fn(3) == 4 and seen == [1, 2, 'in', 3, 'out']
