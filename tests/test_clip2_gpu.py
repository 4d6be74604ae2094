"""Value clamp, per-group norms and the landed step count on the device: dep_grad_clip_value, dep_adam_step_opt and the optimizer surface
over them, against the numpy fp64 yardstick of clip2_ref.py (pinned against torch in test_clip2_cpu.py).

Bounds.  One update from a given state is held to test_clip_gpu.py's bar for the clipped one: 2e-7 absolute on p at lr = 1e-4
(parameters below 1 in magnitude: three roundings of a value whose ulp is at most 6e-8), 2e-6 / 1e-4 relative on m / v (the kernel forms
1 - beta in fp32).  The clamp adds no rounding: the yardstick clamps the same fp32 product g * coef the kernel clamps.  Sequences are
compared step by step, each step from the parameters the device holds, so the one-step bound applies to every step.  The device's
bias factors (beta^t by squaring, within 7e-15 of the exact power) round to fp32 within one ulp of the yardstick's: 6e-8 relative of a
movement of at most 3.2 lr, far inside the 2e-7."""
import os
import sys

import numpy as np
import pytest

import clip2_ref
from clip_ref import clip_coef, sqnorm
from conftest import ROOT, load_golden
from optim_rec import _params
from oracle import ref_numpy as R

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L, nn
    DEV = torch.device('cuda:0')
    SLOTS = L.grad_norm_slots()

SIZES = (5000, 1, 2049)                 # a ragged tail over several workgroups; one element; one element past a workgroup's 2048
CASES = [(True, 1e-5), (False, 0.0), (False, 1e-3)]
LR = 1e-4
NEW_KERNELS = ('adam_opt_kernel', 'adam_opt_ext_kernel', 'grad_clip_value_kernel')


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _state(n, seed, fresh=False):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    g = (0.05 * rng.standard_normal(n)).astype(np.float32)
    m = np.zeros(n, np.float32) if fresh else (0.01 * rng.standard_normal(n)).astype(np.float32)
    v = np.zeros(n, np.float32) if fresh else (1e-4 * rng.random(n)).astype(np.float32)
    return p, g, m, v


def _check_update(got, st, gc, step, wd, decoupled):
    """got = (p, m, v) on the device after one update from st = (p, g, m, v) with the prepared gradient gc (float64)."""
    pn, mn, vn = R.adam_step(st[0].astype(np.float64), gc, st[2].astype(np.float64), st[3].astype(np.float64), step, LR, wd=wd,
                             decoupled=decoupled)
    p, m, v = (host(t) for t in got)
    print('n=%d: |dp| %.3g |dm| %.3g |dv| %.3g' % (p.size, np.abs(p - pn).max(), np.abs(m - mn).max(), np.abs(v - vn).max()))
    assert np.abs(p - pn).max() < 2e-7
    assert np.abs(m - mn).max() <= 2e-6 * np.abs(mn).max()
    assert np.abs(v - vn).max() <= 1e-4 * np.abs(vn).max()
    assert np.abs(pn - st[0]).max() > 1e-6                                   # the step moved something


# ------------------------------------------------------------------------------------------------ value clamp
@pytest.mark.parametrize('decoupled,wd', CASES)
@pytest.mark.parametrize('max_norm', [None, 0.5])
def test_clamp_against_numpy(decoupled, wd, max_norm):
    sts = [_state(n, 20 + i, fresh=(i == 1)) for i, n in enumerate(SIZES)]
    step = 3
    part, coef = None, np.float32(1.0)
    if max_norm is not None:
        part = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
        L.grad_sqnorm([dev(s[1]) for s in sts], part)
        coef = clip_coef(sqnorm([s[1] for s in sts]), max_norm)
        assert coef < 1.0
    scaled = np.abs(np.concatenate([s[1] for s in sts]) * coef)
    c = float(np.median(scaled))                                             # binds on about half of the elements
    assert 0.4 < np.mean(scaled > np.float32(c)) < 0.6
    for st in sts:
        p, g, m, v = (dev(a) for a in st)
        L.adam_step_opt(p, g, m, v, LR, 0.9, 0.999, 1e-8, wd, decoupled, step, partials=part, max_norm=max_norm or 0.0, max_grad_value=c)
        assert np.array_equal(host(g), st[1])                                # g is not written back
        _check_update((p, m, v), st, clip2_ref.clamped_gradient(st[1], coef, c), step, wd, decoupled)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('form', ['plain', 'clipped', 'ext', 'clipped-ext'])
def test_clamp_that_never_binds_gives_the_bits_of_the_step_without_it(n, form):
    st = _state(n, 31)
    clipped, ext = 'clipped' in form, 'ext' in form
    part = None
    if clipped:
        part = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
        L.grad_sqnorm([dev(st[1])], part)
    rng = np.random.default_rng(5)
    vmax0, ema0 = (1e-4 * rng.random(n)).astype(np.float32), rng.uniform(-0.5, 0.5, n).astype(np.float32)
    res = []
    for c in (None, 1e9):
        p, g, m, v = (dev(a) for a in st)
        vmax, ema = (dev(vmax0), dev(ema0)) if ext else (None, None)
        kw = dict(vmax=vmax, ema=ema, ema_decay=0.9) if ext else {}
        if c is not None:
            L.adam_step_opt(p, g, m, v, LR, 0.9, 0.999, 1e-8, 1e-3, False, 2, partials=part, max_norm=0.01, max_grad_value=c, **kw)
        elif ext:
            L.adam_step_ext(p, g, m, v, LR, 0.9, 0.999, 1e-8, 1e-3, False, 2, partials=part, max_norm=0.01, **kw)
        elif clipped:
            L.adam_step_clipped(p, g, m, v, LR, 0.9, 0.999, 1e-8, 1e-3, False, 2, part, 0.01)
        else:
            L.adam_step(p, g, m, v, LR, 0.9, 0.999, 1e-8, 1e-3, False, 2)
        res.append([t for t in (p, m, v, vmax, ema) if t is not None])
    assert not np.array_equal(host(res[0][0]), st[0])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _special_gradient(n, seed):
    st = _state(n, seed)
    g = st[1]
    g[0], g[1], g[2], g[3], g[4] = np.nan, np.inf, -np.inf, -0.0, 0.0
    return st


@pytest.mark.parametrize('decoupled,wd', [(True, 1e-5), (False, 1e-3)])
def test_clip_value_in_place_then_plain_update_equals_the_fused_clamp(decoupled, wd):
    sts = [_state(n, 40 + i) for i, n in enumerate(SIZES)] + [_special_gradient(9, 44)]
    c = 0.03
    gs = [dev(s[1]) for s in sts]
    L.grad_clip_value(gs, c)
    for st, g in zip(sts, gs):
        want = clip2_ref.clamp(st[1], c)
        assert host(g).tobytes() == want.tobytes()                           # bytes: NaN stays, +-inf -> +-c, the zeros keep their signs
        p, g0, m, v = (dev(a) for a in st)
        L.adam_step_opt(p, g0, m, v, LR, 0.9, 0.999, 1e-8, wd, decoupled, 4, max_grad_value=c)
        p1, _, m1, v1 = (dev(a) for a in st)
        L.adam_step(p1, g, m1, v1, LR, 0.9, 0.999, 1e-8, wd, decoupled, 4)
        assert host(p).tobytes() == host(p1).tobytes() and host(m).tobytes() == host(m1).tobytes() and host(v).tobytes() == host(v1).tobytes()
    p = host(p)
    assert np.isnan(p[0]) and np.isfinite(p[1:]).all()                       # the NaN element alone is lost; the inf ones moved as +-c
    pn, _, _ = R.adam_step(st[0].astype(np.float64), clip2_ref.clamped_gradient(st[1], 1.0, c), st[2].astype(np.float64),
                           st[3].astype(np.float64), 4, LR, wd=wd, decoupled=decoupled)
    assert np.abs(p[1:] - pn[1:]).max() < 2e-7


# ------------------------------------------------------------------------------------------------ stand-in owners on the device
class Owner:
    def __init__(self, n, n_live=None):
        self._flat = torch.zeros(n, device=DEV)
        self._flat_grad = torch.zeros(n, device=DEV)
        self._grad_ready = True
        self._n_live = n if n_live is None else n_live


def _fill(params, arrays, what):
    for p, a in zip(params, arrays):
        getattr(p.owner, what)[p.offset:p.offset + p.numel].copy_(dev(np.asarray(a, np.float32)))


def _three_ranges(seed):
    """Two owners, three ranges: (a, 0, 5000), (a, 5000, 5004), (b, 0, 2052).  Returns (params, their initial values)."""
    a, b = Owner(5004), Owner(2052)
    ps = _params(nn, a, SIZES[:2]) + _params(nn, b, SIZES[2:])
    rng = np.random.default_rng(seed)
    P = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n in SIZES]
    _fill(ps, P, '_flat')
    return ps, P


def _grads(seed, steps, scale=0.05):
    rng = np.random.default_rng(seed)
    return [[(scale * rng.standard_normal(n)).astype(np.float32) for n in SIZES] for _ in range(steps)]


def _values(ps, what='_flat'):
    return [host(getattr(p.owner, what)[p.offset:p.offset + p.numel]).copy() for p in ps]


def _moments(opt, ps):
    return [[host(opt._state[id(p.owner)][k][p.offset:p.offset + p.numel]).copy() for p in ps] for k in (0, 1)]


def _run_steps(opt, ps, G, groups, bounds, wds, max_value=None, skip=False, count_skipped=True, check=True):
    """Every step of G through opt.step(), each held to one yardstick step from the parameters the device holds before it."""
    M = V = None
    landed, recs = 0, []
    for k, gs in enumerate(G):
        _fill(ps, gs, '_flat_grad')
        P0 = _values(ps)
        opt.step()
        ref = clip2_ref.run(P0, [gs], groups=groups, bounds=bounds, max_value=max_value, skip_nonfinite=skip, count_skipped=count_skipped,
                            lr=LR, wds=wds, decoupled=opt.decoupled, M=M, V=V, step0=k, landed0=landed)
        M, V, landed = ref['M'], ref['V'], ref['landed']
        recs.append(ref['steps'][0])
        if check:
            for got, want, p0 in zip(_values(ps), ref['P'], P0):
                assert np.abs(got - want).max() < 2e-7, k
                if ref['steps'][0]['skipped']:
                    assert got.tobytes() == p0.tobytes()
    return recs, landed


# ------------------------------------------------------------------------------------------------ per-group norms
@pytest.mark.parametrize('decoupled,wd', CASES)
def test_per_group_norms_against_numpy(decoupled, wd):
    ps, _ = _three_ranges(60)
    groups, bounds = [[0], [1, 2]], [0.5, 0.05]
    opt = (nn.AdamW if decoupled else nn.Adam)([{'params': ps[:1], 'weight_decay': wd}, {'params': ps[1:], 'weight_decay': wd, 'max_grad_norm': 0.05}],
                                               lr=LR, max_grad_norm=0.5, clip_per_group=True, max_grad_value=0.02)
    G = _grads(61, 3)
    G[2] = [g * np.float32(0.01) for g in G[2]]                              # the third step clips nowhere
    recs, _ = _run_steps(opt, ps, G, groups, bounds, [wd, wd], max_value=0.02)
    # each slice holds exactly what dep_grad_sqnorm gives for that group alone
    for k, idx in enumerate(groups):
        alone = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
        L.grad_sqnorm([p.owner._flat_grad[p.offset:p.offset + (p.numel + 3) // 4 * 4] for p in (ps[i] for i in idx)], alone)
        assert torch.equal(opt._clip2[0][k * SLOTS:(k + 1) * SLOTS], alone)
    assert recs[0]['coefs'][0] < 1.0 and recs[0]['coefs'][1] < 1.0 and recs[2]['coefs'] == [1.0, 1.0]
    st = opt.grad_stats()
    assert st['steps'] == 3 and st['clipped'] == 2 and st['skipped'] == 0 and st['last_coef'] == 1.0
    assert abs(st['last_norm'] - recs[2]['norm']) <= 1e-6 * recs[2]['norm']
    for got, n, c in zip(st['groups'], recs[2]['norms'], recs[2]['coefs']):
        assert abs(got['last_norm'] - n) <= 1e-6 * n and abs(got['last_coef'] - c) <= 1e-6 * c
    # and of a step that clips
    _fill(ps, G[0], '_flat_grad')
    opt.step()
    st = opt.grad_stats()
    assert abs(st['last_coef'] - min(recs[0]['coefs'])) <= 1e-6 * min(recs[0]['coefs']) and abs(st['last_norm'] - recs[0]['norm']) <= 1e-6 * recs[0]['norm']
    for got, n, c in zip(st['groups'], recs[0]['norms'], recs[0]['coefs']):
        assert abs(got['last_norm'] - n) <= 1e-6 * n and abs(got['last_coef'] - c) <= 1e-6 * c


@pytest.mark.parametrize('kw', [dict(max_grad_norm=0.5), dict(max_grad_norm=0.5, skip_nonfinite=True, amsgrad=True, ema_decay=0.9), dict(skip_nonfinite=True)])
def test_one_group_per_group_gives_the_bits_of_the_global_path(kw):
    res = []
    for per_group in (False, True):
        ps, _ = _three_ranges(62)
        opt = nn.AdamW(ps, lr=LR, clip_per_group=per_group, **kw)
        for gs in _grads(63, 2):
            _fill(ps, gs, '_flat_grad')
            opt.step()
        st = opt.grad_stats()
        st.pop('groups', None)
        res.append((_values(ps), _moments(opt, ps), st))
    (pa, ma, sa), (pb, mb, sb) = res
    assert sa == sb and sa['steps'] == 2
    for a, b in zip(pa + ma[0] + ma[1], pb + mb[0] + mb[1]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('own,default', [(0.05, None), (0.05, 0.5), (None, 0.5)])
def test_one_active_group_is_clipped_against_its_own_bound(own, default):
    """Two groups, the first one holds no gradient: the launches carry one group, whose bound is its own -- not the optimizer's."""
    ps, _ = _three_ranges(68)
    opt = nn.AdamW([{'params': ps[:1]}, {'params': ps[1:], 'max_grad_norm': own}], lr=LR, weight_decay=1e-5, max_grad_norm=default,
                   clip_per_group=True, skip_nonfinite=True)
    ps[0].live = False
    live = ps[1:]
    G = [gs[1:] for gs in _grads(69, 2)]                                     # norm ~ 2.3: 0.05 and 0.5 both clip, None does not
    recs, _ = _run_steps(opt, live, G, [[0, 1]], [own], [1e-5], skip=True)
    want = 1.0 if own is None else own / (recs[1]['norms'][0] + 1e-6)
    assert (want < 0.1) == (own is not None) and abs(recs[1]['coefs'][0] - want) <= 1e-6 * want
    st = opt.grad_stats()
    assert st['groups'][0] == {'last_norm': None, 'last_coef': None}
    assert abs(st['groups'][1]['last_coef'] - want) <= 1e-6 * want and abs(st['last_coef'] - want) <= 1e-6 * want
    assert st['clipped'] == (0 if own is None else 2)


def test_nan_coefficient_of_one_group_shows_at_the_top_level():
    """No skip_nonfinite: a NaN in group 0 makes its coefficient NaN, and a finite coefficient of a later group does not hide it; the step
    still counts as clipped, because group 1's coefficient is below 1."""
    ps, _ = _three_ranges(72)
    opt = nn.AdamW([{'params': ps[:1]}, {'params': ps[1:]}], lr=LR, max_grad_norm=0.5, clip_per_group=True)
    gs = _grads(73, 1)[0]
    gs[0][3] = np.nan
    _fill(ps, gs, '_flat_grad')
    opt.step()
    st = opt.grad_stats()
    assert np.isnan(st['groups'][0]['last_coef']) and st['groups'][1]['last_coef'] < 1.0
    assert np.isnan(st['last_coef']) and st['clipped'] == 1 and st['last_finite'] is False
    assert np.isnan(_values(ps)[0]).all() and np.isfinite(_values(ps)[2]).all()


def test_nan_in_one_group_skips_every_group():
    ps, _ = _three_ranges(64)
    opt = nn.AdamW([{'params': ps[:1]}, {'params': ps[1:], 'max_grad_norm': None}], lr=LR, max_grad_norm=0.5, clip_per_group=True, skip_nonfinite=True)
    G = _grads(65, 2)
    _fill(ps, G[0], '_flat_grad')
    opt.step()
    before = (_values(ps), _moments(opt, ps))
    G[1][2][77] = np.nan                                                     # group 1 only
    _fill(ps, G[1], '_flat_grad')
    opt.step()
    after = (_values(ps), _moments(opt, ps))
    for a, b in zip(before[0] + before[1][0] + before[1][1], after[0] + after[1][0] + after[1][1]):
        assert a.tobytes() == b.tobytes()                                    # group 0's p, m, v as well
    st = opt.grad_stats()
    assert st['steps'] == 2 and st['skipped'] == 1 and st['last_finite'] is False
    n0 = np.sqrt(sqnorm([G[1][0]]))
    assert abs(st['groups'][0]['last_norm'] - n0) <= 1e-6 * n0 and np.isnan(st['groups'][1]['last_norm'])


def test_accumulated_gradient_with_all_three_options():
    """accumulate_steps = 2: the options act on the accumulated gradient, the fp32 sum of the two micro-steps' gradients."""
    ps, _ = _three_ranges(66)
    opt = nn.AdamW([{'params': ps[:1]}, {'params': ps[1:], 'max_grad_norm': 0.05}], lr=LR, weight_decay=1e-5, max_grad_norm=0.5, clip_per_group=True,
                   max_grad_value=0.02, skip_nonfinite=True, count_skipped=False, accumulate_steps=2)
    G = _grads(67, 2)
    P0 = _values(ps)
    for gs in G:
        _fill(ps, gs, '_flat_grad')
        opt.step()
    acc = [a + b for a, b in zip(*G)]                                        # float32 + float32: the accumulate launch's one rounding
    ref = clip2_ref.run(P0, [acc], groups=[[0], [1, 2]], bounds=[0.5, 0.05], max_value=0.02, skip_nonfinite=True, count_skipped=False, lr=LR,
                        wds=[1e-5, 1e-5], decoupled=True)
    assert ref['steps'][0]['coefs'][0] < 1.0 and ref['steps'][0]['coefs'][1] < 1.0
    for got, want, p0 in zip(_values(ps), ref['P'], P0):
        assert np.abs(got - want).max() < 2e-7 and np.abs(want - p0).max() > 1e-6
    assert opt.landed_steps() == 1 and opt.pending == 0 and opt.grad_stats()['steps'] == 1


# ------------------------------------------------------------------------------------------------ landed count
def _two_ranges(seed):
    """One owner, two ranges: a dead tensor between the two live ones."""
    o = Owner(5000 + 8 + 2052)
    ps = _params(nn, o, (5000, 7, 2049), dead=(1,))
    live = [ps[0], ps[2]]
    rng = np.random.default_rng(seed)
    P = [rng.uniform(-0.5, 0.5, p.numel).astype(np.float32) for p in live]
    _fill(live, P, '_flat')
    return live, P


def _five_steps(seed):
    rng = np.random.default_rng(seed)
    G = [[(0.05 * rng.standard_normal(n)).astype(np.float32) for n in (5000, 2049)] for _ in range(5)]
    G[1][1][5] = np.nan
    G[3][0][4999] = np.inf
    return G                                                                 # finite / NaN / finite / inf / finite


def _landed_run(count_skipped, check, stop=5, resume=None):
    ps, _ = _two_ranges(70)
    opt = nn.AdamW(ps, lr=LR, weight_decay=1e-5, max_grad_norm=0.5, skip_nonfinite=True, count_skipped=count_skipped)
    G = _five_steps(71)
    if resume is not None:
        sd, P = resume
        _fill(ps, P, '_flat')
        opt.load_state_dict(sd)
        for gs in G[stop:]:
            _fill(ps, gs, '_flat_grad')
            opt.step()
    else:
        _run_steps(opt, ps, G[:stop], None, [0.5], [1e-5], skip=True, count_skipped=count_skipped, check=check)
    return opt, ps


def test_skipped_steps_do_not_count_in_the_bias_correction():
    opt, ps = _landed_run(False, True)
    assert opt.landed_steps() == 3 and opt.grad_stats()['skipped'] == 2 and opt.grad_stats()['steps'] == 5
    assert opt.state_dict()['landed'] == 3 and opt.state_dict()['step'] == 5
    mine = _values(ps) + sum(_moments(opt, ps), [])
    opt2, ps2 = _landed_run(False, False)                                    # two runs: the same bits
    for a, b in zip(mine, _values(ps2) + sum(_moments(opt2, ps2), [])):
        assert a.tobytes() == b.tobytes()
    counted, psc = _landed_run(True, False)                                  # the counted path is another optimizer: the test measures the feature
    diff = max(np.abs(a - b).max() for a, b in zip(_values(ps), _values(psc)))
    assert diff > 10 * 2e-7, diff
    # a checkpoint after step 3, resumed: steps 4 and 5 bit for bit
    opt3, ps3 = _landed_run(False, False, stop=3)
    assert opt3.landed_steps() == 2
    opt4, ps4 = _landed_run(False, False, stop=3, resume=(opt3.state_dict(), _values(ps3)))
    assert opt4.landed_steps() == 3
    for a, b in zip(mine, _values(ps4) + sum(_moments(opt4, ps4), [])):
        assert a.tobytes() == b.tobytes()


def test_counted_path_against_numpy_on_the_same_sequence():
    opt, _ = _landed_run(True, True)                                         # the yardstick with t = the call count: the old behaviour
    assert opt.grad_stats()['skipped'] == 2


# ------------------------------------------------------------------------------------------------ model
def _pads(model):
    used = np.zeros(model._flat_grad.numel(), bool)
    for p in model.parameters():
        if p.live:
            used[p.offset:p.offset + p.numel] = True
    return np.flatnonzero(~used)


def _model():
    from icassp2022_depression_amd import audio_gru_whole as mod
    g = load_golden('audio_clf_tiny')
    B, T, F, H = [int(v) for v in g['shape']]
    cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0)
    model = mod.AudioBiLSTM(cfg, seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()}, strict=True)
    return mod, model, g


def test_model_steps_with_all_three_options_against_numpy():
    mod, model, g = _model()
    max_norm = 1e-3
    crit = nn.CrossEntropyLoss()
    model.train()
    params = dict(model.named_parameters())
    # the clamp's bound from the data, so that it binds on about half of the elements: the median of |g * coef| of the first gradients
    crit(model(g['x']), g['y']).backward()
    scaled = []
    for grp in mod.get_param_group(model):
        gs = [host(p.grad) for p in grp['params'] if p.grad is not None]
        scaled += [np.abs(a * clip_coef(sqnorm(gs), max_norm)).ravel() for a in gs]
    c = float(np.median(np.concatenate(scaled)))
    assert c > 0.0
    opt = nn.AdamW(mod.get_param_group(model), lr=LR, max_grad_norm=max_norm, clip_per_group=True, max_grad_value=c, skip_nonfinite=True,
                   count_skipped=False)
    M, V = {}, {}
    pads = _pads(model)
    assert len(pads) > 0
    for step in (1, 2):
        opt.zero_grad()
        crit(model(g['x']), g['y']).backward()
        names = [[p.name for p in grp['params'] if p.grad is not None] for grp in opt.param_groups]
        assert len(names) == 2 and all(names)
        P0 = {n: host(params[n].data).astype(np.float64) for ns in names for n in ns}
        G = {n: host(params[n].grad).copy() for ns in names for n in ns}
        assert not host(model._flat_grad)[pads].any()
        opt.step()
        st = opt.grad_stats()
        bound = binds = 0
        for gi, (grp, ns) in enumerate(zip(opt.param_groups, names)):
            S = sqnorm([G[n] for n in ns])
            coef = clip_coef(S, max_norm)
            assert abs(st['groups'][gi]['last_norm'] - np.sqrt(S)) <= 1e-6 * np.sqrt(S) and abs(st['groups'][gi]['last_coef'] - coef) <= 1e-6 * coef
            for n in ns:
                if step == 1:
                    M[n] = np.zeros_like(P0[n]); V[n] = np.zeros_like(P0[n])
                gc = clip2_ref.clamped_gradient(G[n], coef, c)
                bound += int((np.abs(gc) == np.float32(c)).sum()); binds += gc.size
                pn, M[n], V[n] = R.adam_step(P0[n], gc, M[n], V[n], step, LR, wd=grp['weight_decay'], decoupled=True)
                assert np.abs(host(params[n].data) - pn).max() < 2e-7, (step, n)
        assert 0 < bound < binds                                             # the clamp binds somewhere, not everywhere
        assert not host(model._flat_grad)[pads].any()
    assert opt.landed_steps() == 2 and opt.grad_stats()['steps'] == 2 and opt.grad_stats()['skipped'] == 0
    model.check_health()


# ------------------------------------------------------------------------------------------------ launch sequence
def _kernels_of_a_step(opt_kw):
    mod, model, g = _model()
    opt = nn.AdamW(mod.get_param_group(model), lr=LR, **opt_kw)
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


def test_launch_counts():
    plain = _kernels_of_a_step({})
    assert not [k for k in plain if any(n in k for n in NEW_KERNELS)], plain                 # defaults launch none of the new kernels
    clipped = _kernels_of_a_step({'max_grad_norm': 1.0})
    assert not [k for k in clipped if any(n in k for n in NEW_KERNELS)], clipped
    strip = lambda ks: [k for k in ks if 'adam' not in k and 'grad_sqnorm' not in k]
    clamp = _kernels_of_a_step({'max_grad_value': 1e-5})
    assert len(clamp) == len(plain) and sum('adam_opt_kernel' in k for k in clamp) == 2 and not any('grad_sqnorm' in k for k in clamp)
    assert strip(clamp) == strip(plain)                                                      # the clamp alone adds no launch
    per_group = _kernels_of_a_step({'max_grad_norm': 1.0, 'clip_per_group': True, 'skip_nonfinite': True, 'count_skipped': False})
    assert sum('grad_sqnorm_kernel' in k for k in per_group) == 2 and sum('adam_opt_kernel' in k for k in per_group) == 2
    assert len(per_group) == len(plain) + 2 == len(clipped) + 1                              # G launches instead of one
    assert strip(per_group) == strip(plain)


# ------------------------------------------------------------------------------------------------ data parallel
def _run_rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    sys.path.insert(0, ROOT)
    import contextlib
    import io
    from icassp2022_depression_amd import audio_gru_whole as m, nn, parallel
    parallel.init_from_env('gloo')
    g = load_golden('audio_clf_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, batch_size=5, learning_rate=float(g['lr']))
    m.audio_features = g['feats']; m.audio_targets = g['targs']
    m.model = m.AudioBiLSTM(m.config, seed=0)
    m.model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
    m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate'], max_grad_norm=1e-3, clip_per_group=True,
                           max_grad_value=2e-5, skip_nonfinite=True, count_skipped=False)
    m.criterion = nn.CrossEntropyLoss()
    with contextlib.redirect_stdout(io.StringIO()):
        m.train(1, list(range(17)))
    q.put((rank, {k: v.cpu().numpy() for k, v in m.model.state_dict().items()}, m.optimizer.grad_stats(), m.optimizer.landed_steps()))
    parallel.barrier()
    parallel.destroy_native_comm()
    import torch.distributed as dist
    dist.destroy_process_group()


def test_two_ranks_with_all_three_options_end_with_bit_equal_parameters():
    """Every rank holds the same reduced gradients: the same per-group coefficients, the same skip decision, the same landed count,
    without a collective.  The two ranks share cuda:0 over gloo, as tests/test_clip_gpu.py runs them."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 26000 + os.getpid() % 1000
    procs = [ctx.Process(target=_run_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r, (sd, st, landed)) for r, sd, st, landed in (q.get(timeout=240) for _ in range(2)))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (sd0, st0, l0), (sd1, st1, l1) = res[0], res[1]
    assert st0 == st1 and st0['steps'] == 4 and st0['clipped'] >= 1 and l0 == l1 == 4
    for k in sd0:
        assert sd0[k].tobytes() == sd1[k].tobytes(), k
