"""Global-norm gradient clipping, the parts that need no GPU.

1. The yardstick of tests/test_clip_gpu.py is pinned: clip_ref.clipped_adam_steps (numpy fp64: S = sum g^2, torch's coefficient
   formula with ONE rounding to fp32, oracle.ref_numpy.adam_step on g * coef) against torch.nn.utils.clip_grad_norm_ +
   torch.optim.AdamW / Adam on the CPU, three steps, norms below, at and far above max_norm.  Tolerance: the fp32 rounding of the
   coefficient and of torch's fp32 update -- parameters within 1e-6 relative.
2. The three entry points refuse bad arguments (DEP_ERR_ARG) before any HIP call.
3. The optimizer's host logic against a recording stand-in of the binding: default construction never calls a new entry point;
   with max_grad_norm set there is exactly one dep_grad_sqnorm per step(), over the ranges of all groups, then one clipped update
   per range.
"""
import numpy as np
import pytest

from clip_ref import clip_coef, clipped_adam_steps
from optim_rec import ERR_ARG, _Owner, _arrs, _params, lib, name_buffers, record_binding  # noqa: F401 -- lib is a fixture

torch = pytest.importorskip('torch')

SHAPES = [(7,), (3, 5), (1,), (4, 4), (33,)]


def _tensors(seed, scale):
    rng = np.random.default_rng(seed)
    P = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    G = [[(scale * rng.standard_normal(s)).astype(np.float32) for s in SHAPES] for _ in range(3)]
    return P, G


def _torch_steps(P, G, max_norm, lr, wd, decoupled):
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in P]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ps, lr=lr, weight_decay=wd)
    norms = []
    for gs in G:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
    return [p.detach().numpy().astype(np.float64) for p in ps], norms


# gradient scale 1 has a norm near 8 over the 62 elements: max_norm 1e3 is far above it (coef = 1), 1e-3 far below (coef ~ 1e-4)
@pytest.mark.parametrize('decoupled,wd', [(True, 1e-2), (False, 0.0), (False, 1e-3)])
@pytest.mark.parametrize('max_norm', [1e3, 1.0, 1e-3, 'at'])
def test_numpy_helper_equals_torch_clip_plus_adam(decoupled, wd, max_norm):
    P, G = _tensors(3, 1.0)
    if max_norm == 'at':                     # the first step's norm itself: the quotient is 1 - 1e-6 / norm, just below the clamp
        max_norm = float(np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in G[0])))
    lr = 1e-2
    ref, coefs, norms = clipped_adam_steps(P, G, max_norm, lr, wd=wd, decoupled=decoupled)
    got, tnorms = _torch_steps(P, G, max_norm, lr, wd, decoupled)
    for n, tn in zip(norms, tnorms):
        assert abs(n - tn) <= 1e-6 * n
    for c, n in zip(coefs, norms):
        assert (c == 1.0) == (max_norm / (n + 1e-6) >= 1.0)
    for r, t in zip(ref, got):
        assert np.abs(r - t).max() <= 1e-6 * np.abs(r).max()


def test_coefficient_formula():
    assert clip_coef(4.0, 1.0) == np.float32(1.0 / (2.0 + 1e-6))
    assert clip_coef(4.0, 100.0) == 1.0
    assert clip_coef(4.0, 0.0) == 1.0 and clip_coef(4.0, float('inf')) == 1.0        # measure only
    assert clip_coef(float('inf'), 1.0) == 0.0
    assert np.isnan(clip_coef(float('nan'), 1.0))


# ------------------------------------------------------------------------------------------------ argument refusals
def test_entry_points_refuse_bad_arguments(lib):
    assert lib.dep_grad_norm_slots() == 256 and lib.dep_grad_norm_chunk() > 0 and lib.dep_grad_norm_chunk() % 4 == 0
    ok = 0x1000                                                       # never dereferenced on the host: the checks come first
    bufs, cnts = _arrs([ok], [8])
    assert lib.dep_grad_sqnorm(None, cnts, 1, ok, None) == ERR_ARG
    assert lib.dep_grad_sqnorm(bufs, None, 1, ok, None) == ERR_ARG
    assert lib.dep_grad_sqnorm(bufs, cnts, 1, None, None) == ERR_ARG
    assert lib.dep_grad_sqnorm(bufs, cnts, 0, ok, None) == ERR_ARG
    b17, c17 = _arrs([ok] * 17, [4] * 17)
    assert lib.dep_grad_sqnorm(b17, c17, 17, ok, None) == ERR_ARG
    assert b'bad argument' in lib.dep_last_error()
    for bad in (0, -3):
        b2, c2 = _arrs([ok, ok], [4, bad])
        assert lib.dep_grad_sqnorm(b2, c2, 2, ok, None) == ERR_ARG
        assert lib.dep_grad_clip_scale(b2, c2, 2, ok, 1.0, None, None) == ERR_ARG
    b2, c2 = _arrs([ok, None], [4, 4])
    assert lib.dep_grad_sqnorm(b2, c2, 2, ok, None) == ERR_ARG
    assert lib.dep_grad_clip_scale(b2, c2, 2, ok, 1.0, None, None) == ERR_ARG
    assert lib.dep_grad_clip_scale(bufs, cnts, 1, None, 1.0, None, None) == ERR_ARG
    assert lib.dep_grad_clip_scale(None, cnts, 1, ok, 1.0, None, None) == ERR_ARG
    assert lib.dep_grad_clip_scale(bufs, cnts, 0, ok, 1.0, None, None) == ERR_ARG
    assert lib.dep_grad_clip_scale(b17, c17, 17, ok, 1.0, None, None) == ERR_ARG
    assert lib.dep_grad_clip_scale(bufs, cnts, 1, ok, float('nan'), None, None) == ERR_ARG

    def adam(p=ok, g=ok, m=ok, v=ok, n=8, step=1, partials=ok, max_norm=1.0):
        return lib.dep_adam_step_clipped(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, step, partials, max_norm, 0, None, None, None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-1), dict(step=0), dict(partials=None),
               dict(max_norm=float('nan'))):
        assert adam(**kw) == ERR_ARG, kw


# ------------------------------------------------------------------------------------------------ host logic, recording binding
@pytest.fixture()
def rec(monkeypatch):
    return record_binding(monkeypatch, adam_logs_p=False)


def _two_owner_groups(nn, owners):
    a, b = _Owner(32), _Owner(16)
    name_buffers(owners, a=a, b=b)
    pa = _params(nn, a, [5, 8, 3, 6], dead=(3,))           # offsets 0, 8, 16, 20; the last one is dead (grad None)
    pb = _params(nn, b, [10])
    groups = [{'params': [pa[0], pa[1]], 'weight_decay': 0.0}, {'params': [pa[2], pa[3], pb[0]], 'weight_decay': 1e-5, 'lr': 5e-4}]
    return groups


def test_default_optimizer_never_calls_a_new_entry_point(rec):
    nn, log, owners = rec
    opt = nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    opt.step(); opt.step()
    assert [e[0] for e in log] == ['adam'] * 6
    assert [e[1] for e in log[:3]] == [('aG', 0, 16), ('aG', 16, 20), ('bG', 0, 12)]
    assert log[0][2:] == (1e-3, 0.9, 0.999, 1e-8, 0.0, True, 1) and log[5][2:] == (5e-4, 0.9, 0.999, 1e-8, 1e-5, True, 2)
    assert opt.grad_stats()['steps'] == 0


@pytest.mark.parametrize('kw', [dict(max_grad_norm=0.5), dict(max_grad_norm=0.5, skip_nonfinite=True), dict(skip_nonfinite=True)])
def test_clipped_step_is_one_sqnorm_over_all_groups_then_one_update_per_range(rec, kw):
    nn, log, owners = rec
    opt = nn.AdamW(_two_owner_groups(nn, owners), lr=1e-3, **kw)
    for step in (1, 2):
        del log[:]
        opt.step()
        assert [e[0] for e in log] == ['sqnorm', 'clipped', 'clipped', 'clipped']
        spans = [('aG', 0, 16), ('aG', 16, 20), ('bG', 0, 12)]          # the dead parameter (offset 20..28) is outside
        assert log[0][1] == spans
        partials = log[0][2]
        assert partials.dtype == torch.float64 and partials.numel() == 256
        for i, e in enumerate(log[1:]):
            assert e[2] == spans[i] and e[1] == (spans[i][0][0] + 'P',) + spans[i][1:]
            lr, b1, b2, eps, wd, dec, st, part, mx, skip, clip_out, stats = e[3:]
            assert (lr, wd) == ((1e-3, 0.0) if i == 0 else (5e-4, 1e-5)) and dec is True and st == step
            assert part is partials and mx == kw.get('max_grad_norm', 0.0) and skip == kw.get('skip_nonfinite', False)
            assert (clip_out is not None) == (i == 0) and (stats is not None) == (i == 0)     # the record is updated once per step
    # a parameter without a gradient anywhere: nothing to clip, nothing launched
    for g in opt.param_groups:
        for p in g['params']:
            p.owner._grad_ready = False
    del log[:]
    opt.step()
    assert log == []


def test_clip_grad_norm_function_covers_the_merged_ranges(rec):
    nn, log, owners = rec
    groups = _two_owner_groups(nn, owners)
    params = groups[0]['params'] + groups[1]['params']
    r = nn.clip_grad_norm_(params, 2.0)
    assert [e[0] for e in log] == ['sqnorm', 'scale']
    assert log[0][1] == [('aG', 0, 20), ('bG', 0, 12)]                 # contiguous runs merge across the groups
    assert log[1][2] is log[0][2] and log[1][3] == 2.0 and log[1][4] is r._out
    for p in params:
        p.owner._grad_ready = False
    del log[:]
    assert nn.clip_grad_norm_(params, 2.0).item() == 0.0 and log == []


def test_more_ranges_than_one_launch_takes_is_an_error(rec):
    nn, log, owners = rec
    o = _Owner(17 * 8)
    name_buffers(owners, **{'': o})
    ps = _params(nn, o, [4] * 34, dead=tuple(range(1, 34, 2)))          # 17 live tensors, none adjacent to another
    with pytest.raises(nn.L.DepError):
        nn.Adam(ps, max_grad_norm=1.0).step()
    with pytest.raises(ValueError):
        nn.Adam(ps, max_grad_norm=-1.0)
