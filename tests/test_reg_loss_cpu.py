"""Regression criteria with a parameter and sample weights (dep_head_loss_reg): the parts that need no GPU.

1. The yardstick of tests/test_reg_loss_gpu.py is pinned: reg_loss_ref.reg_loss (float64 numpy) against
   torch.nn.functional.{l1,smooth_l1,huber,mse}_loss in float64, values and autograd gradients, with d exactly at plus and minus the
   knee and at 0, z exactly 0 and negative under ReLU, beta = 0, and row weights (built from reduction='none').  Bound 1e-12: float64
   rounding of O(1) values summed over at most 37 x 16 elements, six orders below the fp32 kernel's tolerance.
2. The numpy / config helpers of the training loops (balanced_group_weight, reg_options, reg_criterion, sample_row_weight).
3. The criteria's construction-time validation (no device is touched).
4. dep_head_loss_reg / dep_row_weight_sum refuse bad arguments (DEP_ERR_ARG) before any HIP call.
"""
import numpy as np
import pytest

import reg_loss_ref
from optim_rec import ERR_ARG, lib  # noqa: F401 -- lib is a fixture

torch = pytest.importorskip('torch')
Fn = torch.nn.functional

REG_L1, REG_SMOOTHL1, REG_HUBER, REG_MSE = 0, 1, 2, 3
CASES = [('l1', 0.0), ('smooth_l1', 0.0), ('smooth_l1', 0.5), ('smooth_l1', 1.0), ('smooth_l1', 2.0), ('huber', 0.5), ('huber', 1.0),
         ('huber', 2.0), ('mse', 0.0)]


def torch_elementwise(o, t, form, param):
    if form == 'l1':
        return Fn.l1_loss(o, t, reduction='none')
    if form == 'smooth_l1':
        return Fn.smooth_l1_loss(o, t, reduction='none', beta=param)
    if form == 'huber':
        return Fn.huber_loss(o, t, reduction='none', delta=param)
    return Fn.mse_loss(o, t, reduction='none')


def torch_mean(o, t, form, param):
    if form == 'l1':
        return Fn.l1_loss(o, t)
    if form == 'smooth_l1':
        return Fn.smooth_l1_loss(o, t, beta=param)
    if form == 'huber':
        return Fn.huber_loss(o, t, delta=param)
    return Fn.mse_loss(o, t)


@pytest.mark.parametrize('weights', ['none', 'random', 'zero_rows'])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('form,param', CASES)
@pytest.mark.parametrize('B,C', [(1, 1), (6, 1), (37, 16)])
def test_reference_equals_torch_in_float64(B, C, form, param, relu, weights):
    rng = np.random.default_rng(1000 * B + 10 * C + int(10 * param))
    z, t = reg_loss_ref.inputs_with_edges(rng, B, C, param)
    w = None if weights == 'none' else rng.uniform(0.2, 3.0, B)
    if weights == 'zero_rows':
        w[::3] = 0.0
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t, dtype=torch.float64)
    o = torch.relu(zt) if relu else zt
    if w is None:
        lt = torch_mean(o, tt, form, param)                                        # torch's own mean
    else:
        wt = torch.tensor(w, dtype=torch.float64)
        lt = (wt * torch_elementwise(o, tt, form, param).sum(1)).sum() / (C * wt.sum())
    if w is not None and w.sum() == 0:
        out, rows, loss, dz = reg_loss_ref.reg_loss(z, t, form, param, relu, w)     # B = 1 with its one row ignored: 0 / 0 on both sides
        assert np.isnan(loss) and np.isnan(float(lt.detach())) and np.all(rows == 0.0) and np.all(dz == 0.0)
        return
    lt.backward()
    out, rows, loss, dz = reg_loss_ref.reg_loss(z, t, form, param, relu, w)
    assert abs(loss - float(lt.detach())) <= 1e-12, (form, loss, float(lt.detach()))
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12
    assert np.array_equal(out, o.detach().numpy())
    want_rows = torch_elementwise(o, tt, form, param).sum(1).detach().numpy() * (1.0 if w is None else w)
    assert np.abs(rows - want_rows).max() <= 1e-12
    if w is not None:
        assert np.all(rows[w == 0] == 0.0) and np.all(dz[w == 0] == 0.0)


def test_reference_edges_have_the_stated_values():
    """The knees by hand: at |d| == knee the linear branch (torch's `a < knee` is false), sgn(0) = 0, ReLU passes nothing at z <= 0."""
    z = np.array([[2.5], [1.25], [0.75], [0.0], [-1.5]]); t = np.array([[2.0], [1.75], [0.75], [0.5], [0.25]])      # d = .5, -.5, 0, -.5, -.25
    _, rows, _, dz = reg_loss_ref.reg_loss(z, t, 'smooth_l1', 0.5, True, den=1.0)
    assert rows.tolist() == [0.25, 0.25, 0.0, 0.25, 0.0625] and dz.reshape(-1).tolist() == [1.0, -1.0, 0.0, 0.0, 0.0]
    _, rows, _, dz = reg_loss_ref.reg_loss(z, t, 'huber', 0.5, True, den=1.0)
    assert rows.tolist() == [0.125, 0.125, 0.0, 0.125, 0.03125] and dz.reshape(-1).tolist() == [0.5, -0.5, 0.0, 0.0, 0.0]
    _, rows, _, dz = reg_loss_ref.reg_loss(z, t, 'smooth_l1', 0.0, False, den=1.0)
    assert rows.tolist() == [0.5, 0.5, 0.0, 0.5, 1.75] and dz.reshape(-1).tolist() == [1.0, -1.0, 0.0, -1.0, -1.0]
    _, rows, _, dz = reg_loss_ref.reg_loss(z, t, 'mse', 0.0, False, den=1.0)
    assert rows.tolist() == [0.25, 0.25, 0.0, 0.25, 3.0625] and dz.reshape(-1).tolist() == [1.0, -1.0, 0.0, -1.0, -3.5]


def test_ignored_rows_are_selected_not_multiplied():
    z = np.array([[1.0, 2.0], [0.5, -1.0], [3.0, 0.25]]); t = np.array([[0.5, 1.0], [np.nan, np.nan], [1.0, 1.0]])
    w = np.array([2.0, 0.0, 0.5])
    for form, param in CASES:
        out, rows, loss, dz = reg_loss_ref.reg_loss(z, t, form, param, True, w)
        assert rows[1] == 0.0 and np.all(dz[1] == 0.0) and np.isfinite(loss) and np.isfinite(dz).all()
        assert np.array_equal(out, np.maximum(z, 0.0))
        live = [0, 2]
        _, _, loss_live, dz_live = reg_loss_ref.reg_loss(z[live], t[live], form, param, True, w[live])
        assert abs(loss - loss_live) <= 1e-15 and np.abs(dz[live] - dz_live).max() <= 1e-15
    assert np.isnan(reg_loss_ref.reg_loss(z, t, 'mse', 0.0, True, np.zeros(3))[2])


def test_reference_with_an_explicit_denominator_sums_over_shards():
    rng = np.random.default_rng(7)
    B, C = 11, 3
    z = rng.standard_normal((B, C)) * 2; t = rng.uniform(-1, 3, (B, C)); w = rng.uniform(0.2, 3.0, B); w[4] = 0.0
    for form, param in CASES:
        _, _, loss, dz = reg_loss_ref.reg_loss(z, t, form, param, True, w)
        den = reg_loss_ref.denominator(B, C, w)
        parts = [reg_loss_ref.reg_loss(z[a:b], t[a:b], form, param, True, w[a:b], den=den) for a, b in ((0, 4), (4, 8), (8, 11))]
        assert abs(sum(p[2] for p in parts) - loss) <= 1e-14
        assert np.abs(np.concatenate([p[3] for p in parts]) - dz).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ helpers
def test_balanced_group_weight():
    from icassp2022_depression_amd._common import balanced_group_weight
    w = balanced_group_weight(([3, 9, 4], [1, 2, 5, 6, 7, 8, 0]))                   # 3 depressed, 7 non-depressed rows
    assert w.dtype == np.float64 and w.shape == (10,)
    assert np.allclose(w, [10 / (2 * 3)] * 3 + [10 / (2 * 7)] * 7, rtol=1e-15, atol=0)
    assert abs(w.sum() - 10.0) < 1e-12 and abs(w[:3].sum() - w[3:].sum()) < 1e-12   # the weighted row count stays n; the groups weigh the same
    assert balanced_group_weight(([1], [2])).tolist() == [1.0, 1.0]
    assert balanced_group_weight((np.arange(4), np.arange(4))).tolist() == [1.0] * 8
    for bad in (([], [1, 2]), ([1], []), ()):
        with pytest.raises(ValueError):
            balanced_group_weight(bad)


def test_script_config_readers():
    from icassp2022_depression_amd import _common, nn
    assert _common.reg_options({}) == {}
    assert _common.reg_options({'loss': None, 'loss_beta': None, 'loss_delta': None, 'sample_weights': None}) == {}
    assert _common.reg_options({'loss': 'mse'}) == {'loss': 'mse', 'beta': 1.0, 'delta': 1.0}
    assert _common.reg_options({'loss': 'smooth_l1', 'loss_beta': 0.5}) == {'loss': 'smooth_l1', 'beta': 0.5, 'delta': 1.0}
    assert _common.reg_options({'loss': 'huber', 'loss_delta': 2}) == {'loss': 'huber', 'beta': 1.0, 'delta': 2.0}
    for bad in ({'loss': 'l2'}, {'loss': 'MSE'}, {'loss_beta': 0.5}, {'loss_delta': 2.0}):
        with pytest.raises(ValueError):
            _common.reg_options(bad)
    # the criterion a script builds: its own when the key is absent
    assert type(_common.reg_criterion({}, nn.L1Loss)) is nn.L1Loss
    sl1 = _common.reg_criterion({'loss': None}, nn.SmoothL1Loss)
    assert type(sl1) is nn.SmoothL1Loss and sl1.reg_options.neutral and sl1.reg_options.param == 1.0
    c = _common.reg_criterion({'loss': 'smooth_l1', 'loss_beta': 0.5}, nn.L1Loss)
    assert type(c) is nn.SmoothL1Loss and c.reg_options.param == 0.5 and not c.reg_options.neutral
    c = _common.reg_criterion({'loss': 'huber', 'loss_delta': 2.0}, nn.L1Loss)
    assert type(c) is nn.HuberLoss and c.reg_options.param == 2.0
    assert type(_common.reg_criterion({'loss': 'mse'}, nn.L1Loss)) is nn.MSELoss
    assert type(_common.reg_criterion({'loss': 'l1'}, nn.SmoothL1Loss)) is nn.L1Loss
    with pytest.raises(ValueError):
        _common.reg_criterion({'loss': 'huber', 'loss_delta': 0.0}, nn.L1Loss)
    # sample_weights
    groups = ([0, 1], [2, 3, 4, 5])
    assert _common.sample_row_weight({}, groups) is None and _common.sample_row_weight({'sample_weights': None}, groups) is None
    assert np.allclose(_common.sample_row_weight({'sample_weights': 'balanced'}, groups), [1.5, 1.5, 0.75, 0.75, 0.75, 0.75])
    with pytest.raises(ValueError):
        _common.sample_row_weight({'sample_weights': 'inverse'}, groups)


def test_criterion_validation_needs_no_device():
    from icassp2022_depression_amd import models, nn
    assert nn.L1Loss().reg_options.neutral and nn.SmoothL1Loss().reg_options.neutral
    assert not nn.SmoothL1Loss(beta=0.0).reg_options.neutral and not nn.HuberLoss().reg_options.neutral
    assert not nn.MSELoss().reg_options.neutral
    assert nn.HuberLoss().reg_options.param == 1.0 and nn.HuberLoss(delta=0.25).reg_options.param == 0.25
    for make in (lambda: nn.SmoothL1Loss(beta=-0.1), lambda: nn.SmoothL1Loss(beta=float('nan')), lambda: nn.HuberLoss(delta=0.0),
                 lambda: nn.HuberLoss(delta=-1.0), lambda: nn.HuberLoss(delta=float('nan')), lambda: nn.L1Loss(reduction='sum'),
                 lambda: nn.SmoothL1Loss(reduction='none'), lambda: nn.HuberLoss(reduction='sum'), lambda: nn.MSELoss(reduction='none'),
                 lambda: models.MyLoss('reg', loss='l2'), lambda: models.MyLoss('reg', loss='huber', delta=0.0),
                 lambda: models.MyLoss('reg', loss='smooth_l1', beta=-1.0), lambda: models.MyLoss('clf', loss='mse'),
                 lambda: models.MyLoss('reg', label_smoothing=0.1)):
        with pytest.raises(ValueError):
            make()
    assert models.MyLoss('reg').reg_options.neutral and models.MyLoss('reg', loss='mse').reg_options.loss == 'mse'
    # host-side row weights are validated like host labels are
    cpu = torch.device('cpu')
    w_dev, w_host = nn.RegOptions.rows([0.5, 0.0, 2.0], 3, cpu)
    assert w_dev.dtype == torch.float32 and w_dev.tolist() == [0.5, 0.0, 2.0] and w_host.dtype == np.float64
    assert nn.RegOptions.rows(None, 3, cpu) == (None, None)
    assert nn.RegOptions.rows(torch.tensor([1.0, 2.0]), 2, cpu)[1].tolist() == [1.0, 2.0]
    for bad in ([1.0, 2.0], [1.0, -2.0, 1.0], [1.0, float('nan'), 1.0], [1.0, float('inf'), 1.0], np.ones((2, 2))):
        with pytest.raises(ValueError):
            nn.RegOptions.rows(bad, 3, cpu)


# ------------------------------------------------------------------------------------------------ argument refusals
def test_entry_points_refuse_bad_arguments(lib):
    ok = 0x1000                                                       # never dereferenced on the host: the checks come first

    def reg(form=REG_SMOOTHL1, relu=1, param=1.0, z=ok, target=ok, rw=None, out=None, rows=ok, dz=ok, B=4, C=3, norm=12.0, norm_dev=None):
        return lib.dep_head_loss_reg(form, relu, param, z, target, rw, out, rows, dz, B, C, norm, norm_dev, None)
    for kw in (dict(form=4), dict(form=-1), dict(form=0x100), dict(relu=2), dict(relu=-1), dict(param=float('nan')), dict(param=-0.5),
               dict(form=REG_L1, param=-1.0), dict(form=REG_MSE, param=float('nan')), dict(form=REG_HUBER, param=0.0),
               dict(form=REG_HUBER, param=-2.0), dict(z=None), dict(B=0), dict(B=-3), dict(C=0), dict(C=17),
               dict(norm=0.0), dict(norm=-1.0), dict(norm=float('nan')),
               dict(target=None), dict(target=None, dz=None), dict(target=None, rows=None)):
        assert reg(**kw) == ERR_ARG, kw
        assert b'bad argument' in lib.dep_last_error()
    ws = lib.dep_row_weight_sum
    assert ws(None, 4, 3.0, ok, None) == ERR_ARG
    assert ws(ok, 4, 3.0, None, None) == ERR_ARG
    assert ws(ok, 0, 3.0, ok, None) == ERR_ARG
    assert ws(ok, 4, 0.0, ok, None) == ERR_ARG
    assert ws(ok, 4, float('nan'), ok, None) == ERR_ARG


def test_binding_lists_the_new_entry_points(lib):
    from icassp2022_depression_amd import _lib
    for name in ('dep_head_loss_reg', 'dep_row_weight_sum'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert callable(_lib.head_loss_reg) and callable(_lib.row_weight_sum)
    assert (_lib.REG_L1, _lib.REG_SMOOTHL1, _lib.REG_HUBER, _lib.REG_MSE) == (REG_L1, REG_SMOOTHL1, REG_HUBER, REG_MSE)
