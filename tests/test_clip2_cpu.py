"""Value clamp, per-group norms and the landed step count, the parts that need no GPU.

1. The yardstick of tests/test_clip2_gpu.py is pinned: clip2_ref.run against torch on the CPU, three steps (five for the skipping loop),
   Adam and AdamW, wd 0 / 1e-3 / 1e-2 -- clip_grad_norm_ -> clip_grad_value_ -> step(); the per-group loop over two groups with
   different bounds, one of them None; the loop that calls step() only on a finite norm.  Tolerance: test_clip_cpu.py's 1e-6 relative
   on the parameters; NaN positions equal.
2. clip2_ref.clamp at its edge values.
3. The optimizer's host logic against a recording stand-in of the binding (clip2_ref.record_binding2).
4. dep_grad_clip_value and dep_adam_step_opt refuse bad arguments (DEP_ERR_ARG) before any HIP call.
"""
import ctypes as C

import numpy as np
import pytest

import clip2_ref
from optim_rec import ERR_ARG, _Owner, _arrs, _params, lib, name_buffers  # noqa: F401 -- lib is a fixture

torch = pytest.importorskip('torch')

SHAPES = [(7,), (3, 5), (1,), (4, 4), (33,)]
GROUPS = [[0, 2], [1, 3, 4]]
CASES = [(True, 1e-2), (False, 0.0), (False, 1e-3)]          # (AdamW | Adam, weight decay)
LR = 1e-2


def _tensors(seed, steps=3):
    rng = np.random.default_rng(seed)
    P = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    G = [[rng.standard_normal(s).astype(np.float32) for s in SHAPES] for _ in range(steps)]
    return P, G


def _torch_opt(P, wd, decoupled, groups=None):
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in P]
    arg = ps if groups is None else [{'params': [ps[i] for i in idx]} for idx in groups]
    return ps, (torch.optim.AdamW if decoupled else torch.optim.Adam)(arg, lr=LR, weight_decay=wd)


def _close(ref, ps):
    for r, p in zip(ref, ps):
        t = p.detach().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(r), np.isnan(t))
        ok = ~np.isnan(r)
        assert np.abs(r[ok] - t[ok]).max(initial=0.0) <= 1e-6 * np.abs(r[ok]).max(initial=1.0)


# ------------------------------------------------------------------------------------------------ the yardstick against torch
@pytest.mark.parametrize('decoupled,wd', CASES)
@pytest.mark.parametrize('max_norm,c', [(1.0, 0.05), (1e3, 0.5), (None, 0.3)])
def test_yardstick_equals_torch_norm_clip_then_value_clip_then_step(decoupled, wd, max_norm, c):
    P, G = _tensors(3)                                          # norm ~ 8: max_norm 1 clips (|g * coef| ~ 0.12, c = 0.05 binds on most)
    ref = clip2_ref.run(P, G, bounds=[max_norm], max_value=c, lr=LR, wds=[wd], decoupled=decoupled)
    ps, opt = _torch_opt(P, wd, decoupled)
    for gs in G:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        torch.nn.utils.clip_grad_value_(ps, c)
        opt.step()
    _close(ref['P'], ps)


@pytest.mark.parametrize('decoupled,wd', CASES)
def test_yardstick_equals_torch_per_group_loop(decoupled, wd):
    P, G = _tensors(4)
    bounds = [0.5, None]
    ref = clip2_ref.run(P, G, groups=GROUPS, bounds=bounds, lr=LR, wds=[wd, wd], decoupled=decoupled)
    ps, opt = _torch_opt(P, wd, decoupled, GROUPS)
    for k, gs in enumerate(G):
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        for gi, (grp, b) in enumerate(zip(opt.param_groups, bounds)):
            n = float(torch.nn.utils.clip_grad_norm_(grp['params'], float('inf') if b is None else b))
            assert abs(n - ref['steps'][k]['norms'][gi]) <= 1e-6 * n
        opt.step()
    assert ref['steps'][0]['coefs'][0] < 1.0 and ref['steps'][0]['coefs'][1] == 1.0
    _close(ref['P'], ps)


def five_step_gradients(P_shapes, seed):
    """finite / NaN / finite / inf / finite"""
    rng = np.random.default_rng(seed)
    G = [[rng.standard_normal(s).astype(np.float32) for s in P_shapes] for _ in range(5)]
    G[1][3].flat[2] = np.nan
    G[3][0].flat[0] = np.inf
    return G


@pytest.mark.parametrize('decoupled,wd', CASES)
def test_yardstick_equals_torch_loop_that_skips_on_a_nonfinite_norm(decoupled, wd):
    P, _ = _tensors(5)
    G = five_step_gradients(SHAPES, 6)
    ref = clip2_ref.run(P, G, bounds=[1.0], skip_nonfinite=True, count_skipped=False, lr=LR, wds=[wd], decoupled=decoupled)
    assert ref['landed'] == 3 and ref['skipped'] == 2 and [r['t'] for r in ref['steps']] == [1, 1, 2, 2, 3]
    ps, opt = _torch_opt(P, wd, decoupled)
    for gs in G:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        if torch.isfinite(torch.nn.utils.clip_grad_norm_(ps, 1.0)):
            opt.step()
    _close(ref['P'], ps)
    counted = clip2_ref.run(P, G, bounds=[1.0], skip_nonfinite=True, count_skipped=True, lr=LR, wds=[wd], decoupled=decoupled)
    assert max(np.abs(a - b).max() for a, b in zip(counted['P'], ref['P'])) > 1e-4          # the two counts are different optimizers


def test_clamp_edge_values():
    c = np.float32(0.25)
    inside, outside = np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1))
    x = np.array([c, -c, inside, -inside, outside, -outside, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    y = clip2_ref.clamp(x, c)
    want = np.array([c, -c, inside, -inside, c, -c, c, -c, np.nan, 0.0, -0.0], np.float32)
    assert np.array_equal(y[:8], want[:8]) and np.isnan(y[8]) and y[9:].tobytes() == want[9:].tobytes()      # bytes: the zero keeps its sign
    t = torch.from_numpy(x.copy()).clamp_(-float(c), float(c)).numpy()
    assert t.tobytes()[:32] == y.tobytes()[:32] and np.isnan(t[8]) and t[9:].tobytes() == y[9:].tobytes()


# ------------------------------------------------------------------------------------------------ host logic, recording binding
@pytest.fixture()
def rec(monkeypatch):
    return clip2_ref.record_binding2(monkeypatch)


def _two_owner_groups(nn, owners, **second):
    a, b = _Owner(32), _Owner(16)
    name_buffers(owners, a=a, b=b)
    pa = _params(nn, a, [5, 8, 3, 6], dead=(3,))           # offsets 0, 8, 16, 20; the last one is dead (grad None)
    pb = _params(nn, b, [10])
    return [{'params': [pa[0], pa[1]], 'weight_decay': 0.0}, dict({'params': [pa[2], pa[3], pb[0]], 'weight_decay': 1e-5, 'lr': 5e-4}, **second)]


SPANS = [('aG', 0, 16), ('aG', 16, 20), ('bG', 0, 12)]


def test_defaults_call_no_new_entry_point(rec):
    nn, log, owners = rec
    opt = nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    opt.step()
    assert [e[0] for e in log] == ['sqnorm', 'clipped', 'clipped', 'clipped']
    del log[:]
    nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3).step()
    assert [e[0] for e in log] == ['adam'] * 3
    del log[:]
    nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, amsgrad=True).step()
    assert [e[0] for e in log] == ['ext'] * 3
    assert 'groups' not in opt.grad_stats()


@pytest.mark.parametrize('amsgrad', [False, True])
def test_clamp_alone_is_one_new_launch_per_range_and_no_sqnorm(rec, amsgrad):
    nn, log, owners = rec
    opt = nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, max_grad_value=0.25, amsgrad=amsgrad)
    opt.step()
    assert [e[0] for e in log] == ['opt'] * 3 and [e[2] for e in log] == SPANS
    for e in log:
        kw = e[3]
        assert kw['max_grad_value'] == 0.25 and kw['partials'] is None and kw['clip_out'] is None and kw['stats'] is None
        assert kw['ngroups'] == 1 and kw['group'] == 0 and kw['landed_in'] is None and kw['landed_out'] is None
        assert (kw['vmax'] is not None) == amsgrad and kw['step'] == 1


def test_clamp_with_the_global_norm_keeps_the_one_sqnorm(rec):
    nn, log, owners = rec
    opt = nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, max_grad_value=0.25, max_grad_norm=2.0)
    opt.step()
    assert [e[0] for e in log] == ['sqnorm', 'opt', 'opt', 'opt'] and log[0][1] == SPANS
    assert all(e[3]['partials'] is log[0][2] and e[3]['max_norm'] == 2.0 and e[3]['ngroups'] == 1 for e in log[1:])
    assert [e[3]['clip_out'] is not None for e in log[1:]] == [True, False, False]


def test_per_group_is_one_sqnorm_per_group_into_slices_of_one_buffer(rec):
    nn, log, owners = rec
    opt = nn.AdamW(_two_owner_groups(nn, owners, max_grad_norm=None), lr=1e-3, max_grad_norm=0.5, clip_per_group=True, max_grad_value=0.1)
    for step in (1, 2):
        del log[:]
        opt.step()
        assert [e[0] for e in log] == ['sqnorm', 'sqnorm', 'opt', 'opt', 'opt']
        assert log[0][1] == SPANS[:1] and log[1][1] == SPANS[1:]
        s0, s1 = log[0][2], log[1][2]
        assert s0.numel() == s1.numel() == 256 and s0.dtype == torch.float64
        assert s0.untyped_storage().data_ptr() == s1.untyped_storage().data_ptr() and (s0.storage_offset(), s1.storage_offset()) == (0, 256)
        for i, e in enumerate(log[2:]):
            kw = e[3]
            assert e[2] == SPANS[i] and kw['ngroups'] == 2 and kw['group'] == (0 if i == 0 else 1) and kw['group_max_norms'] == [0.5, 0.0]
            assert kw['partials'].untyped_storage().data_ptr() == s0.untyped_storage().data_ptr() and kw['partials'].numel() >= 2 * 256
            assert kw['max_grad_value'] == 0.1 and kw['step'] == step and kw['max_norm'] == 0.0      # the bounds are the list's, nothing else
            for key in ('clip_out', 'stats', 'group_out'):                       # the record pointers go to the first launch only
                assert (kw[key] is not None) == (i == 0), key
    assert [g['last_norm'] for g in opt.grad_stats()['groups']] == [0.0, 0.0]
    # only group 1 holds a gradient: one sqnorm, one group
    for p in opt.param_groups[0]['params']:
        p.live = False
    del log[:]
    opt.step()
    assert [e[0] for e in log] == ['sqnorm', 'opt', 'opt'] and log[0][1] == SPANS[1:]
    # its own bound is None: measured, not clipped -- in the list AND in the scalar a one-group launch may fall back to, not the optimizer's 0.5
    assert all(e[3]['ngroups'] == 1 and e[3]['group'] == 0 and e[3]['group_max_norms'] == [0.0] and e[3]['max_norm'] == 0.0 for e in log[1:])
    assert opt.grad_stats()['groups'][0] == {'last_norm': None, 'last_coef': None}


@pytest.mark.parametrize('own,default,want', [(0.05, None, 0.05), (0.05, 0.5, 0.05), (None, 0.5, 0.0), ('absent', 0.5, 0.5)])
def test_one_active_group_is_clipped_against_its_own_bound(rec, own, default, want):
    nn, log, owners = rec
    a = _Owner(16)
    name_buffers(owners, a=a)
    grp = {'params': _params(nn, a, [5, 8])}
    if own != 'absent':
        grp['max_grad_norm'] = own
    opt = nn.Adam([grp], max_grad_norm=default, clip_per_group=True, skip_nonfinite=True)
    opt.step()
    assert [e[0] for e in log] == ['sqnorm', 'opt']
    kw = log[1][3]
    assert kw['ngroups'] == 1 and kw['group_max_norms'] == [want] and kw['max_norm'] == want


def test_landed_buffer_is_shared_by_a_step_and_the_parity_flips(rec):
    nn, log, owners = rec
    opt = nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, skip_nonfinite=True, count_skipped=False)
    seen = []
    for step in (1, 2, 3):
        del log[:]
        opt.step()
        assert [e[0] for e in log] == ['sqnorm', 'opt', 'opt', 'opt']
        ins = [e[3]['landed_in'] for e in log[1:]]
        outs = [e[3]['landed_out'] for e in log[1:]]
        assert all(t.dtype == torch.int32 and t.numel() == 1 and t.data_ptr() == ins[0].data_ptr() for t in ins)
        assert outs[0] is not None and outs[1] is None and outs[2] is None
        assert outs[0].untyped_storage().data_ptr() == ins[0].untyped_storage().data_ptr() and outs[0].data_ptr() != ins[0].data_ptr()
        assert all(e[3]['skip_nonfinite'] is True and e[3]['step'] == step for e in log[1:])
        seen.append((ins[0].storage_offset(), outs[0].storage_offset()))
    assert seen == [(0, 1), (1, 0), (0, 1)]
    # a step that launches nothing does not turn the two words
    for g in opt.param_groups:
        for p in g['params']:
            p.owner._grad_ready = False
    del log[:]
    opt.step()
    assert log == [] and opt._landed_at == 1
    assert opt.landed_steps() == 0                                              # the stand-in launches nothing


def test_accumulation_runs_the_per_group_sqnorms_at_the_boundary_on_one_rank(rec):
    nn, log, owners = rec
    opt = nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, max_grad_norm=0.5, clip_per_group=True, accumulate_steps=2,
                   skip_nonfinite=True, count_skipped=False)
    opt.step()
    assert [e[0] for e in log] == ['accum'] and log[0][5] is None
    del log[:]
    opt.step()
    assert [e[0] for e in log] == ['accum', 'sqnorm', 'sqnorm', 'opt', 'opt', 'opt']
    assert log[0][5] is None                                                    # the accumulate launch's fused partials are not asked for
    names = {a.untyped_storage().data_ptr(): k for k, a in (('aA', opt._accum[id(opt.param_groups[0]['params'][0].owner)]),
                                                             ('bA', opt._accum[id(opt.param_groups[1]['params'][2].owner)]))}
    owners.update(names)
    assert log[1][1] == [('aA', 0, 16)] and log[2][1] == [('aA', 16, 20), ('bA', 0, 12)]
    assert [e[2] for e in log[3:]] == [('aA', 0, 16), ('aA', 16, 20), ('bA', 0, 12)] and all(e[3]['step'] == 1 for e in log[3:])
    # the global norm with the clamp still takes the accumulate launch's partials on one rank
    del log[:]
    opt = nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, max_grad_norm=0.5, max_grad_value=0.1, accumulate_steps=2)
    opt.step(); opt.step()
    assert [e[0] for e in log] == ['accum', 'accum', 'opt', 'opt', 'opt'] and log[1][5] is not None
    assert all(e[3]['partials'] is log[1][5] for e in log[2:])


def test_errors(rec):
    nn, log, owners = rec
    mk = lambda **second: _two_owner_groups(nn, owners, **second)
    for bad in (0.0, -1.0, float('nan'), float('inf'), True, '0.5'):
        with pytest.raises(ValueError):
            nn.Adam(mk(), max_grad_value=bad)
        with pytest.raises(ValueError):
            nn.clip_grad_value_(mk()[0]['params'], bad)
    with pytest.raises(ValueError):
        nn.Adam(mk(max_grad_norm=1.0), max_grad_norm=2.0)                        # a group's bound without clip_per_group
    with pytest.raises(ValueError):
        nn.Adam(mk(max_grad_norm=-1.0), clip_per_group=True)
    with pytest.raises(ValueError):
        nn.Adam(mk(max_grad_norm=float('nan')), clip_per_group=True)
    with pytest.raises(ValueError):
        nn.Adam(mk(), clip_per_group=True)                                       # no bound anywhere, no skip_nonfinite
    nn.Adam(mk(), clip_per_group=True, skip_nonfinite=True)
    nn.Adam(mk(max_grad_norm=1.0), clip_per_group=True)
    with pytest.raises(ValueError):
        nn.Adam(mk(), count_skipped=False)
    with pytest.raises(ValueError):
        nn.Adam(mk(), count_skipped=False, max_grad_norm=1.0)
    with pytest.raises(nn.L.DepError):
        nn.Adam(mk(), max_grad_norm=1.0).landed_steps()
    # nine groups with a gradient
    o = _Owner(9 * 8)
    name_buffers(owners, c=o)
    ps = _params(nn, o, [4] * 18, dead=tuple(range(1, 18, 2)))
    live = [p for p in ps if p.live]
    opt = nn.Adam([{'params': [p]} for p in live], max_grad_norm=1.0, clip_per_group=True)
    with pytest.raises(nn.L.DepError):
        opt.step()
    nn.Adam([{'params': [p]} for p in live[:8]], max_grad_norm=1.0, clip_per_group=True).step()
    # seventeen ranges for the function, and in one group of a per-group optimizer (sixteen pass; the global limit does not apply per group)
    o = _Owner(17 * 8)
    name_buffers(owners, d=o)
    ps = _params(nn, o, [4] * 34, dead=tuple(range(1, 34, 2)))
    live = [p for p in ps if p.live]
    with pytest.raises(nn.L.DepError, match='per group'):
        nn.Adam([{'params': live[:1]}, {'params': live}], max_grad_norm=1.0, clip_per_group=True).step()
    del log[:]
    nn.Adam([{'params': live[:16]}, {'params': live[16:]}], max_grad_norm=1.0, clip_per_group=True).step()
    assert [e[0] for e in log] == ['sqnorm'] * 2 + ['opt'] * 17
    with pytest.raises(nn.L.DepError):
        nn.clip_grad_value_(ps, 1.0)


def test_clip_grad_value_function_covers_the_merged_ranges(rec):
    nn, log, owners = rec
    groups = _two_owner_groups(nn, owners)
    params = groups[0]['params'] + groups[1]['params']
    assert nn.clip_grad_value_(params, 0.5) is None
    assert log == [('value', [('aG', 0, 20), ('bG', 0, 12)], 0.5)]
    for p in params:
        p.owner._grad_ready = False
    del log[:]
    nn.clip_grad_value_(params, 0.5)
    assert log == []


def test_state_dict_round_trip_with_and_without_landed(rec):
    nn, log, owners = rec
    mk = lambda **kw: nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, skip_nonfinite=True, **kw)
    a = mk(count_skipped=False)
    a.step(); a.step()
    a._clip2[2][a._landed_at] = 2                                               # what the launches would have left
    sd = a.state_dict()
    assert sd['landed'] == 2 and sd['step'] == 2
    b = mk(count_skipped=False)
    b.load_state_dict(sd)
    assert b.landed_steps() == 2 and b._step == 2 and b._clip2[2].tolist() == [2, 2]
    assert b.state_dict()['landed'] == 2
    c = mk()
    c.step()
    sdc = c.state_dict()
    assert 'landed' not in sdc
    mk().load_state_dict(sdc)
    with pytest.raises(ValueError, match='count_skipped'):
        c.load_state_dict(sd)
    with pytest.raises(ValueError, match='count_skipped'):
        b.load_state_dict(sdc)


def test_optim_options_keys():
    from icassp2022_depression_amd import _common
    cfg = {'learning_rate': 1e-3}
    assert _common.optim_options(cfg) == {}
    assert _common.optim_options(dict(cfg, max_grad_value=None, clip_per_group=False, skip_nonfinite=False, count_skipped=True)) == {}
    assert _common.optim_options(dict(cfg, max_grad_value=1, clip_per_group=True, skip_nonfinite=True, count_skipped=False)) == \
        {'max_grad_value': 1.0, 'clip_per_group': True, 'skip_nonfinite': True, 'count_skipped': False}
    for bad in (dict(max_grad_value=0), dict(max_grad_value=float('nan')), dict(max_grad_value=True), dict(max_grad_value='1'),
                dict(clip_per_group=1), dict(skip_nonfinite='yes'), dict(count_skipped=0), dict(count_skipped=False)):
        with pytest.raises(ValueError):
            _common.optim_options(dict(cfg, **bad))
    assert 'get_param_group' in _common.optim_options.__doc__


# ------------------------------------------------------------------------------------------------ argument refusals
def test_new_entry_points_refuse_bad_arguments(lib):
    from icassp2022_depression_amd import _lib
    ok, ok2 = 0x1000, 0x2000                                          # never dereferenced on the host: the checks come first
    bufs, cnts = _arrs([ok], [8])
    assert lib.dep_grad_clip_value(None, cnts, 1, 1.0, None) == ERR_ARG
    assert lib.dep_grad_clip_value(bufs, None, 1, 1.0, None) == ERR_ARG
    assert lib.dep_grad_clip_value(bufs, cnts, 0, 1.0, None) == ERR_ARG
    b17, c17 = _arrs([ok] * 17, [4] * 17)
    assert lib.dep_grad_clip_value(b17, c17, 17, 1.0, None) == ERR_ARG
    b2, c2 = _arrs([ok, None], [4, 4])
    assert lib.dep_grad_clip_value(b2, c2, 2, 1.0, None) == ERR_ARG
    b2, c2 = _arrs([ok, ok], [4, 0])
    assert lib.dep_grad_clip_value(b2, c2, 2, 1.0, None) == ERR_ARG
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert lib.dep_grad_clip_value(bufs, cnts, 1, bad, None) == ERR_ARG
    assert b'bad argument' in lib.dep_last_error()

    two = (C.c_float * 2)(1.0, 2.0)

    def step(p=ok, g=ok, m=ok, v=ok, n=8, step=1, partials=ok, max_norm=1.0, skip=1, c=0.5, ngroups=1, group=0, bounds=None,
             group_out=None, landed_in=None, landed_out=None):
        opt = _lib.AdamOpt(c, ngroups, group, bounds, group_out, landed_in, landed_out)
        return lib.dep_adam_step_opt(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, step, None, partials, max_norm, skip, None, None,
                                     C.byref(opt), None)
    nan2 = (C.c_float * 2)(1.0, float('nan'))
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(step=0), dict(c=-1.0), dict(c=float('nan')),
               dict(c=float('inf')), dict(ngroups=0), dict(ngroups=9, bounds=two), dict(ngroups=2, group=2, bounds=two),
               dict(group=-1), dict(group=1), dict(ngroups=2, bounds=None), dict(ngroups=2, bounds=two, partials=None, skip=0),
               dict(ngroups=2, bounds=nan2), dict(max_norm=float('nan')), dict(group_out=ok2, partials=None, skip=0),
               dict(landed_in=ok2, skip=0), dict(landed_in=ok2, partials=None), dict(landed_out=ok2),
               dict(landed_in=ok2, landed_out=ok2)):
        assert step(**kw) == ERR_ARG, kw
    # everything off is dep_adam_step_ext, whose own checks answer
    off = _lib.AdamOpt(0.0, 1, 0, None, None, None, None)
    assert lib.dep_adam_step_opt(None, ok, ok, ok, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, None, None, 0.0, 0, None, None, C.byref(off), None) == ERR_ARG
    assert lib.dep_adam_step_opt(ok, ok, ok, ok, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, None, None, 0.0, 0, None, None, None, None) == ERR_ARG
