"""Regression criteria with a parameter and sample weights, on the device: dep_head_loss_reg / dep_row_weight_sum, nn.L1Loss /
SmoothL1Loss(beta) / HuberLoss(delta) / MSELoss with `weight=`, the regression fusion loss, and the declared denominators of the
training loops (accumulation, data parallelism, the scripts' config).

Yardstick: reg_loss_ref.reg_loss (float64 numpy, pinned to torch in tests/test_reg_loss_cpu.py), evaluated on the float32-rounded
inputs the kernel is given.  Tolerances are the ones tests/test_weighted_loss_gpu.py and tests/test_small_kernels_gpu.py apply to the
head losses -- out bit-equal to fp32 max(z, 0), per-row losses 1e-6 max(1, max |rows|), dz relerr < 1e-5, loss 1e-6 max(1, |loss|),
the device denominator 1e-6 relative; the loops are held to tests/test_accum_gpu.py's bars against one big batch (parameters
2e-5 + 1e-4 max|v|, gradients relerr 1e-3, summed loss 1e-4) and to tests/test_dp_gpu.py's 2e-6 + 1e-5 max|v| against one process.
Run on the MI355X box:  python -m pytest tests/test_reg_loss_gpu.py -m gpu -q"""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

import reg_loss_ref
from conftest import ROOT, load_golden

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from icassp2022_depression_amd import _common, _lib as L, models, nn, parallel
    from icassp2022_depression_amd import audio_bilstm_perm, text_bilstm_perm
    DEV = torch.device('cuda:0')

F32 = np.float32
# (reference form, parameter): L1; SmoothL1 with beta in {0, 0.5, 1, 2}; Huber with delta in {0.5, 2}; MSE
CASES = [('l1', 0.0), ('smooth_l1', 0.0), ('smooth_l1', 0.5), ('smooth_l1', 1.0), ('smooth_l1', 2.0), ('huber', 0.5), ('huber', 2.0), ('mse', 0.0)]
FORM = {'l1': 'REG_L1', 'smooth_l1': 'REG_SMOOTHL1', 'huber': 'REG_HUBER', 'mse': 'REG_MSE'}


def r32(a):
    """float64 holding float32 values: what the kernel is given."""
    return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def buffers(B, C):
    return (torch.full((B, C), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV), torch.full((B, C), 7.0, device=DEV),
            torch.full((1,), float('nan'), device=DEV))


def row_weights(how, B, rng):
    """none / uniform in [0.2, 3] / every third row exactly 0 (from row 2 on, so that a one-row batch keeps its live row)."""
    if how == 'none':
        return None
    w = r32(rng.uniform(0.2, 3.0, B))
    if how == 'ignored':
        w[2::3] = 0.0
    return w


def check_against_reference(tag, z, relu, out, rows, dz, loss, ref, w):
    _, rows_ref, loss_ref_, dz_ref = ref
    got_loss = host(loss)[0]
    print('%s: rows %.3g (of %.3g)  dz relerr %.3g  loss %.9g (ref %.9g)' % (
        tag, np.abs(host(rows) - rows_ref).max(), np.abs(rows_ref).max(), relerr(host(dz), dz_ref), got_loss, loss_ref_))
    want_out = np.maximum(z.astype(F32), F32(0)) if relu else z.astype(F32)
    assert np.array_equal(out.cpu().numpy(), want_out), tag                                   # bit for bit, ignored rows included
    assert np.abs(host(rows) - rows_ref).max() < 1e-6 * max(1.0, np.abs(rows_ref).max()), tag
    assert relerr(host(dz), dz_ref) < 1e-5, tag
    assert abs(got_loss - loss_ref_) < 1e-6 * max(1.0, abs(loss_ref_)), tag
    if w is not None:
        ign = w == 0.0
        assert np.all(host(rows)[ign] == 0.0) and np.all(host(dz)[ign] == 0.0), tag            # exactly zero, although the targets are NaN


# ------------------------------------------------------------------------------------------------ kernel parity
# the block is 128 rows: one row, one short of / exactly / one past a block, several blocks; C = 1, 3, 16 (the most a row holds)
GRID = [(1, 1), (127, 3), (128, 16), (129, 1), (300, 16)]


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('B,C', GRID)
def test_kernel_against_the_reference(B, C, relu):
    for form, param in CASES:
        rng = np.random.default_rng(100 * B + C + 7 * relu)
        z, t = reg_loss_ref.inputs_with_edges(rng, B, C, param)
        z, t = r32(z), r32(t)
        zd = dev(z)
        for how in ('none', 'uniform', 'ignored'):
            w = row_weights(how, B, rng)
            tt = t.copy()
            if how == 'ignored':
                tt[w == 0.0] = np.nan                                 # an ignored row's target holds anything
            td = dev(tt); wd = None if w is None else dev(w)
            ref = reg_loss_ref.reg_loss(z, tt, form, param, bool(relu), w)
            den_ref = reg_loss_ref.denominator(B, C, w)
            assert den_ref > 0 and np.isfinite(ref[2]) and np.isfinite(ref[3]).all()
            tag = '%s(%g) B=%d C=%d relu=%d w=%s' % (form, param, B, C, relu, how)
            f = getattr(L, FORM[form])
            # (a) the host norm
            norm = float(F32(den_ref))
            out, rows, dz, loss = buffers(B, C)
            L.head_loss_reg(f, relu, param, zd, td, out, rows, dz, norm, wd)
            L.reduce_loss(rows, norm, loss)
            check_against_reference(tag + ' host norm', z, relu, out, rows, dz, loss, ref, w)
            # (b) the denominator summed on the device, read through norm_dev
            if w is None:
                continue
            den = torch.full((1,), float('nan'), device=DEV)
            L.row_weight_sum(wd, C, den)
            assert abs(host(den)[0] - den_ref) <= 1e-6 * den_ref, tag       # <= 2 terms per thread + a 64-lane and a 4-wave tree + the scale
            out, rows, dz, loss = buffers(B, C)
            L.head_loss_reg(f, relu, param, zd, td, out, rows, dz, den, wd)
            L.reduce_loss_by(rows, den, loss)
            check_against_reference(tag + ' device norm', z, relu, out, rows, dz, loss, ref, w)


def test_pure_forward_writes_out_only():
    z = r32(np.random.default_rng(1).standard_normal((5, 3)) * 2)
    out, rows, dz, _ = buffers(5, 3)
    L.head_loss_reg(L.REG_MSE, 1, 0.0, dev(z), None, out, None, None, 15.0)
    assert np.array_equal(out.cpu().numpy(), np.maximum(z.astype(F32), F32(0)))
    assert torch.all(rows == 7.0) and torch.all(dz == 7.0)


@pytest.mark.parametrize('old,form,relu', [('LOSS_L1_RELU', 'REG_L1', 1), ('LOSS_SMOOTHL1_RELU', 'REG_SMOOTHL1', 1),
                                           ('LOSS_SMOOTHL1', 'REG_SMOOTHL1', 0)])
@pytest.mark.parametrize('B,C', GRID)
def test_neutral_case_is_bit_identical_to_dep_head_loss(B, C, old, form, relu):
    rng = np.random.default_rng(7 * B + C)
    z, t = reg_loss_ref.inputs_with_edges(rng, B, C, 1.0)
    zd, td = dev(z), dev(t)
    for norm in (float(B * C), 3.0 * B * C):                          # the batch's own count, and a declared global one
        out0, rows0, dz0, loss0 = buffers(B, C)
        L.head_loss(getattr(L, old), zd, td, out0, rows0, dz0, norm)
        L.reduce_loss(rows0, norm, loss0)
        out1, rows1, dz1, loss1 = buffers(B, C)
        L.head_loss_reg(getattr(L, form), relu, 1.0, zd, td, out1, rows1, dz1, norm)
        L.reduce_loss(rows1, norm, loss1)
        assert torch.equal(out1, out0) and torch.equal(rows1, rows0) and torch.equal(dz1, dz0) and torch.equal(loss1, loss0)
    # unit weights summed on the device give exactly B * C: the same bits again
    den = torch.full((1,), float('nan'), device=DEV)
    ones = torch.ones(B, device=DEV)
    L.row_weight_sum(ones, C, den)
    assert host(den)[0] == float(B * C)
    out0, rows0, dz0, loss0 = buffers(B, C)
    L.head_loss(getattr(L, old), zd, td, out0, rows0, dz0, float(B * C))
    L.reduce_loss(rows0, float(B * C), loss0)
    out2, rows2, dz2, loss2 = buffers(B, C)
    L.head_loss_reg(getattr(L, form), relu, 1.0, zd, td, out2, rows2, dz2, den, ones)
    L.reduce_loss_by(rows2, den, loss2)
    assert torch.equal(out2, out0) and torch.equal(rows2, rows0) and torch.equal(dz2, dz0) and torch.equal(loss2, loss0)


def test_all_rows_weight_zero_gives_nan():
    B, C = 3, 2
    rng = np.random.default_rng(0)
    zd = dev(rng.standard_normal((B, C))); td = dev(rng.standard_normal((B, C)))
    wd = torch.zeros(B, device=DEV)
    den = torch.full((1,), 5.0, device=DEV)
    L.row_weight_sum(wd, C, den)
    assert host(den)[0] == 0.0
    out, rows, dz, loss = buffers(B, C)
    L.head_loss_reg(L.REG_MSE, 1, 0.0, zd, td, out, rows, dz, den, wd)
    L.reduce_loss_by(rows, den, loss)
    assert np.isnan(host(loss)[0]) and np.all(host(rows) == 0.0) and np.all(host(dz) == 0.0)


# ------------------------------------------------------------------------------------------------ nn level
def _kernels_logged(fn):
    torch.cuda.synchronize()
    L.order_log_enable(True)
    try:
        res = fn(); torch.cuda.synchronize()
        log = L.order_log_read(reset=True)
    finally:
        L.order_log_enable(False)
    return res, [e[2:] for e in log if e.startswith('K ')]


def _order_logged(fn):
    """(result, the whole enqueue-order log: kernels, collectives and host notes)."""
    torch.cuda.synchronize()
    L.order_log_enable(True)
    try:
        res = fn(); torch.cuda.synchronize()
        log = L.order_log_read(reset=True)
    finally:
        L.order_log_enable(False)
    return res, log


def _regressor(name):
    """A tiny AudioGRU('reg') / TextBiLSTM('reg'): T = 6, F = 8, H = 16, B = 5."""
    mod, cls = {'audio': (audio_bilstm_perm, 'AudioBiLSTM'), 'text': (text_bilstm_perm, 'TextBiLSTM')}[name]
    cfg = dict(mod.config); cfg.update(embedding_size=8, hidden_dims=16, dropout=0.0)
    model = getattr(mod, cls)(cfg, seed=3)
    assert isinstance(model, models.AudioGRU if name == 'audio' else models.TextBiLSTM) and model.variant == 'reg'
    model.train()
    x = np.random.default_rng(5).standard_normal((5, 6, 8)).astype(np.float32)
    return model, x


def _criteria():
    return [(nn.L1Loss(), 'l1', 0.0), (nn.SmoothL1Loss(), 'smooth_l1', 1.0), (nn.SmoothL1Loss(beta=0.5), 'smooth_l1', 0.5),
            (nn.SmoothL1Loss(beta=0.0), 'smooth_l1', 0.0), (nn.HuberLoss(), 'huber', 1.0), (nn.HuberLoss(delta=0.25), 'huber', 0.25),
            (nn.MSELoss(), 'mse', 0.0)]


@pytest.mark.parametrize('name', ['audio', 'text'])
def test_criteria_through_a_model_against_the_reference(name):
    model, x = _regressor(name)
    y = np.array([0.05, 0.3, 0.0, 1.5, 0.2])                          # near the tiny model's outputs: both sides of every knee occur
    w = np.array([0.5, 2.0, 0.0, 1.25, 3.0])                          # row 2 is ignored
    for crit, form, param in _criteria():
        for where in ('none', 'host', 'device'):
            weight = {'none': None, 'host': w, 'device': dev(w)}[where]
            output = model(x)
            loss, kernels = _kernels_logged(lambda: crit(output, y.reshape(-1, 1), weight=weight) if weight is not None
                                            else crit(output, y.reshape(-1, 1)))
            if where == 'none' and crit.reg_options.neutral:
                assert kernels == ['head_loss_kernel', 'reduce_loss_kernel'], kernels          # the launches they always enqueued
            elif where == 'device':
                assert kernels == ['row_weight_sum_kernel', 'head_loss_reg_kernel', 'reduce_loss_by_kernel'], kernels   # one launch more, no host read
            else:
                assert kernels == ['head_loss_reg_kernel', 'reduce_loss_kernel'], kernels
            z = host(output._z)
            _, _, loss_want, dz_want = reg_loss_ref.reg_loss(z, r32(y).reshape(-1, 1), form, param, True, None if weight is None else w)
            got = loss.item()
            print('%s %s(%g) %s weights: loss %.9g (ref %.9g), dz relerr %.3g' % (name, form, param, where, got, loss_want,
                                                                                   relerr(host(loss.dz), dz_want)))
            assert abs(got - loss_want) < 1e-6 * max(1.0, abs(loss_want))
            assert relerr(host(loss.dz), dz_want) < 1e-5
            assert np.array_equal(output.numpy(), np.maximum(z, 0.0).astype(F32))
            if weight is not None:
                assert np.all(host(loss.dz)[2] == 0.0)
            loss.backward()                                            # the backward starts from that tensor
            model.check_health()
    # evaluate(): the batch's own denominator, no gradient
    model.eval()
    crit = nn.MSELoss()
    loss = crit(model(x), y.reshape(-1, 1), weight=w)
    want = reg_loss_ref.reg_loss(host(model(x)._z), r32(y).reshape(-1, 1), 'mse', 0.0, True, w)[2]
    assert loss.dz is None and abs(loss.item() - want) < 1e-6 * max(1.0, abs(want))
    model.train()
    with pytest.raises(ValueError):
        crit(model(x), y.reshape(-1, 1), weight=[1.0, 2.0])            # two weights, five rows
    with pytest.raises(ValueError):
        crit(model(x), y.reshape(-1, 1), weight=[1.0, 2.0, -1.0, 1.0, 1.0])


def test_declared_denominators_and_the_data_parallel_refusal(monkeypatch):
    model, x = _regressor('audio')
    y = np.array([0.05, 0.3, 0.0, 1.5, 0.2]).reshape(-1, 1)
    w = np.array([0.5, 2.0, 0.0, 1.25, 3.0])
    crit = nn.HuberLoss(delta=0.25)
    try:
        parallel.set_accumulated_weight(20.0)                          # the 5 rows are a micro-batch of a group whose weights sum to 20
        output = model(x)
        loss = crit(output, y, weight=dev(w))
        want = reg_loss_ref.reg_loss(host(output._z), r32(y), 'huber', 0.25, True, w, den=20.0)
        assert abs(loss.item() - want[2]) < 1e-6 * max(1.0, abs(want[2])) and relerr(host(loss.dz), want[3]) < 1e-5
        parallel.set_accumulated_weight(None)
        model.eval()                                                   # evaluate() never takes a declared weight
        parallel.set_accumulated_weight(20.0)
        want = reg_loss_ref.reg_loss(host(model(x)._z), r32(y), 'huber', 0.25, True, w)[2]
        assert abs(crit(model(x), y, weight=w).item() - want) < 1e-6 * max(1.0, abs(want))
        parallel.set_accumulated_weight(None)
        model.train()
        monkeypatch.setattr(parallel, 'world_size', lambda: 2)
        with pytest.raises(L.DepError) as e:
            crit(model(x), y, weight=w)                                # weights, two ranks, nothing declared
        assert 'parallel.set_global_weight' in str(e.value) and 'row_weight=' in str(e.value)
    finally:
        parallel.set_accumulated_weight(None); parallel.set_global_weight(None)


def test_default_criteria_enqueue_what_they_did():
    class OldL1(nn._HeadLoss):                                         # the path the two criteria took before they had arguments
        kind = L.LOSS_L1_RELU
        target_dtype = 'float'

    class OldSmoothL1(nn._HeadLoss):
        kind = L.LOSS_SMOOTHL1_RELU
        target_dtype = 'float'

    model, x = _regressor('audio')
    y = np.array([0.05, 0.3, 0.0, 1.5, 0.2]).reshape(-1, 1)
    output = model(x)
    nn.MSELoss()(output, y, weight=[1.0] * 5)                          # a weighted criterion ran in the same process
    for Old, new in ((OldL1, nn.L1Loss), (OldSmoothL1, nn.SmoothL1Loss)):
        a, log_old = _kernels_logged(lambda: Old()(output, y))
        b, log_new = _kernels_logged(lambda: new()(output, y))
        assert log_new == log_old == ['head_loss_kernel', 'reduce_loss_kernel']
        assert torch.equal(b._v, a._v) and torch.equal(b.dz, a.dz)
    c, log = _kernels_logged(lambda: nn.SmoothL1Loss(beta=1.0, reduction='mean')(output, y, weight=None))
    assert log == ['head_loss_kernel', 'reduce_loss_kernel']


def _fusion(m):
    g = load_golden('fuse_reg')
    N, T, Fa, Ft, Ha, Ht = [int(v) for v in g['dims']]
    m.config.update(audio_embed_size=Fa, text_embed_size=Ft, audio_hidden_dims=Ha, text_hidden_dims=Ht, dropout=0.0,
                    learning_rate=float(g['lr']))
    model = m.build(seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
    model.eval()
    tf, af = model.pretrained_feature([[g['xa'][i], g['xt'][i]] for i in range(N)])
    model.train()
    return g, model, tf, af, N, Ht


def test_fusion_regression_loss_shares_one_denominator():
    from icassp2022_depression_amd import fuse_net as m
    saved_cfg = dict(m.config)
    try:
        g, model, tf, af, N, Ht = _fusion(m)
        y = np.asarray(g['y'], dtype=np.float64) / 64.0                # scaled towards the halves' outputs: both sides of the knees occur
        w = r32(np.random.default_rng(3).uniform(0.2, 3.0, N)); w[1] = 0.0
        W = dict(model.named_parameters())['fc_final.0.weight'].data
        Cc, D = W.shape
        zt = torch.empty(N, Cc, device=DEV); za = torch.empty(N, Cc, device=DEV)      # the halves' outputs, by the calls the loss makes
        L.gemm(0, 1, N, Cc, Ht, tf, Ht, W, D, zt, Cc)
        L.gemm(0, 1, N, Cc, af.shape[1], af, af.shape[1], W[:, Ht:], D, za, Cc)
        den = reg_loss_ref.denominator(N, Cc, w)
        for kw, form, param in ((dict(loss='mse'), 'mse', 0.0), (dict(loss='huber', delta=0.25), 'huber', 0.25),
                                (dict(loss='smooth_l1', beta=0.5), 'smooth_l1', 0.5), (dict(), 'smooth_l1', 1.0), (dict(loss='l1'), 'l1', 0.0)):
            crit = m.MyLoss(**kw)
            loss, log = _kernels_logged(lambda: crit(tf, af, y, model, weight=w))
            assert [k for k in log if 'loss' in k] == ['head_loss_reg_kernel', 'reduce_loss_kernel'] * 2, log
            rt = reg_loss_ref.reg_loss(host(zt), r32(y).reshape(N, Cc), form, param, False, w, den=den)
            ra = reg_loss_ref.reg_loss(host(za), r32(y).reshape(N, Cc), form, param, False, w, den=den)
            want = rt[2] + ra[2]
            got = loss.item()
            print('fusion %s(%g): loss %.9g (ref %.9g)' % (form, param, got, want))
            assert abs(got - want) < 1e-6 * max(1.0, abs(want))
            dzt, dza = loss.dz_halves
            assert relerr(host(dzt), rt[3]) < 1e-5 and relerr(host(dza), ra[3]) < 1e-5
            assert np.all(host(dzt)[1] == 0.0) and np.all(host(dza)[1] == 0.0)
        loss.backward()
        gW = host(dict(model.named_parameters())['fc_final.0.weight'].grad)
        want_gW = np.concatenate([rt[3].T @ host(tf), ra[3].T @ host(af)], axis=1)
        assert relerr(gW, want_gW) < 1e-4                                            # two small fp32 GEMMs over the checked dz
        # device-resident weights: one launch more for the shared denominator, none per half
        _, log = _kernels_logged(lambda: m.MyLoss(loss='mse')(tf, af, y, model, weight=dev(w)))
        assert [k for k in log if 'loss' in k or 'weight' in k] == ['row_weight_sum_kernel'] + ['head_loss_reg_kernel', 'reduce_loss_by_kernel'] * 2
        # a form without weights takes the element count, as the default does
        loss = m.MyLoss(loss='mse')(tf, af, y, model)
        want = sum(reg_loss_ref.reg_loss(host(zh), r32(y).reshape(N, Cc), 'mse', 0.0, False)[2] for zh in (zt, za))
        assert abs(loss.item() - want) < 1e-6 * max(1.0, abs(want))
        # defaults without a weight: the launches the loss always enqueued, and their bits
        old = models.MyLoss('reg')
        a, log_a = _kernels_logged(lambda: old(tf, af, y, model))
        b, log_b = _kernels_logged(lambda: m.MyLoss()(tf, af, y, model))
        assert log_a == log_b and [k for k in log_b if 'loss' in k] == ['head_loss_kernel', 'reduce_loss_kernel'] * 2
        assert torch.equal(a._v, b._v) and torch.equal(a.dz_halves[0], b.dz_halves[0]) and torch.equal(a.dz_halves[1], b.dz_halves[1])
        with pytest.raises(ValueError):
            models.MyLoss('clf')(tf, af, np.zeros(N, dtype=np.int64), model, weight=w)
    finally:
        m.config.clear(); m.config.update(saved_cfg)


# ------------------------------------------------------------------------------------------------ training loops
DEP, NON = [0, 1, 2, 3], [4, 5, 6, 7, 8, 9, 10]                        # 4 against 7 rows: balanced weights 11/8 and 11/14


def _live_start(g):
    """The fixture's parameters with the output bias lifted by 1.  As recorded, every pre-activation of the fixture's model is
    negative: the ReLU passes no gradient and no parameter ever moves (its 'after' equals its 'sd'), which would make every comparison
    of two training runs vacuous.  Lifted, the outputs are 0.8 .. 0.95 against targets of 30 .. 70."""
    sd = {k: v.copy() for k, v in g['sd'].items()}
    sd['fc_audio.4.bias'] = sd['fc_audio.4.bias'] + np.float32(1.0)
    return sd


def _audio_fixture(m, **cfg):
    g = load_golden('audio_reg_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, learning_rate=float(g['lr']), **cfg)
    m.audio_features = g['feats']; m.audio_targets = g['targs']
    model = m.AudioBiLSTM(m.config, seed=0)
    g['start'] = _live_start(g)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g['start'].items()})
    m.train_dep_idxs = list(DEP); m.train_non_idxs = list(NON)
    return g, model


def test_accumulated_balanced_mse_epoch_equals_one_big_weighted_batch():
    """audio_bilstm_perm with loss='mse', sample_weights='balanced', accum_steps=2: 11 rows as micro-batches of 6 and 5 accumulated into
    ONE update, every criterion dividing by the declared weight of the 11 rows, against one 11-row step of a plain optimizer whose
    criterion sums its own denominator from host weights."""
    m = audio_bilstm_perm
    saved_cfg = dict(m.config)
    try:
        g, m.model = _audio_fixture(m, batch_size=6, accum_steps=2, loss='mse', sample_weights='balanced')
        m.optimizer = nn.Adam(m.model.parameters(), lr=m.config['learning_rate'], accumulate_steps=2)
        m.criterion = _common.reg_criterion(m.config, nn.L1Loss)
        assert type(m.criterion) is nn.MSELoss
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            m.train(1)
        assert m.optimizer._step == 1 and m.optimizer.pending == 0
        assert parallel.loss_weight() is None and parallel._global_weight[0] is None            # nothing stays declared
        total = float(out.getvalue().split('Loss:')[1].split()[0])
        # the big batch
        _, big = _audio_fixture(m)
        opt = nn.Adam(big.parameters(), lr=m.config['learning_rate'])
        big.train()
        idx = DEP + NON
        w = np.array([11 / 8] * 4 + [11 / 14] * 7)
        assert np.allclose(_common.sample_row_weight(m.config, (DEP, NON)), w, rtol=1e-15, atol=0)
        loss = nn.MSELoss()(big(m.audio_features[idx]), np.asarray(m.audio_targets)[idx].reshape(-1, 1), weight=w)
        loss.backward()
        grads = {k: host(p.grad).copy() for k, p in big.named_parameters() if p.grad is not None}
        opt.step()
        assert len(grads) >= 10
        for k, p in m.model.named_parameters():
            if k in grads:
                e = relerr(host(m.optimizer.accumulated_grad(p)), grads[k])
                assert e < 1e-3, (k, e)
        sd, sd_big = m.model.state_dict(), big.state_dict()
        moved = 0.0
        for k in sd:
            v = host(sd_big[k])
            assert np.abs(host(sd[k]) - v).max() < 2e-5 + 1e-4 * np.abs(v).max(), k
            if sd[k].dtype.is_floating_point:
                moved = max(moved, np.abs(v - g['start'][k]).max())
        assert moved > 1e-4                                                                   # the update is Adam's first: about lr = 1e-3 per weight
        print('summed micro-losses %.6f, big batch %.6f' % (total, loss.item()))
        assert abs(total - loss.item()) < 1e-4 * max(1.0, abs(loss.item()))                   # the micro-losses sum to the big batch's
    finally:
        m.config.clear(); m.config.update(saved_cfg)
        parallel.set_accumulated_weight(None); parallel.set_global_weight(None); parallel.set_accumulated_count(None)


def test_script_with_all_keys_absent_enqueues_what_it_did():
    """audio_bilstm_perm.train() with none of the new config keys, against the loop as it was written before they existed (spelled out
    here: no helper of the new ones is called, the criterion is _HeadLoss's call): the same enqueue-order log, the same state_dict bits."""
    m = audio_bilstm_perm
    saved_cfg = dict(m.config)

    class OldL1(nn._HeadLoss):
        kind = L.LOSS_L1_RELU
        target_dtype = 'float'

    def old_train(model, optimizer, criterion):
        model.train()
        idx = list(m.train_dep_idxs) + list(m.train_non_idxs)
        pred_dev = _common.prediction_buffer(len(idx), model.device)
        Y_train = m.audio_targets[idx]
        Y_dev = _common.device_labels(Y_train, model.device)
        feed = _common.FeatureFeeder(m.audio_features, idx, model.device, role='audio_features')

        def step(a, b, then):
            output = model(feed.rows(a, b, then=then))
            return criterion(output, Y_dev[a:b].view(-1, 1)), output

        def after_step(a, b, output):
            _common.store_predictions(pred_dev, a, output)
        total = _common.train_epoch(model, optimizer, len(idx), m.config['batch_size'], step, after_step)
        return total, _common.epoch_mae_rmse(Y_train, pred_dev)[0]
    try:
        runs = []
        for which in ('old', 'new', 'old', 'new'):                    # each twice: the first pair also warms the feature cache up
            g, model = _audio_fixture(m, batch_size=4)
            assert not any(k in m.config for k in ('loss', 'loss_beta', 'loss_delta', 'sample_weights'))
            opt = nn.Adam(model.parameters(), lr=m.config['learning_rate'])
            if which == 'old':
                (_, mae), log = _order_logged(lambda: old_train(model, opt, OldL1()))
            else:
                m.model, m.optimizer = model, opt
                m.criterion = _common.reg_criterion(m.config, nn.L1Loss)
                assert type(m.criterion) is nn.L1Loss
                mae, log = _order_logged(lambda: quiet(m.train, 1))
            runs.append((log, {k: v.clone() for k, v in model.state_dict().items()}, mae))
        (log_old, sd_old, mae_old), (log_new, sd_new, mae_new) = runs[2], runs[3]
        assert len(log_old) > 20 and log_new == log_old
        assert not any('head_loss_reg' in k or 'row_weight_sum' in k or 'reduce_loss_by' in k for k in log_new)
        assert mae_new == mae_old
        for k in sd_old:
            assert torch.equal(sd_new[k], sd_old[k]), k
        assert max(np.abs(host(sd_new[k]) - g['start'][k]).max() for k in sd_new if sd_new[k].dtype.is_floating_point) > 1e-4    # and they moved
    finally:
        m.config.clear(); m.config.update(saved_cfg)


# ------------------------------------------------------------------------------------------------ data parallel
def _run_rank(rank, world, port, q):
    # gloo: the ranks share cuda:0 (as tests/test_dp_gpu.py runs them)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    sys.path.insert(0, ROOT)
    from icassp2022_depression_amd import _common, audio_bilstm_perm as m, nn, parallel
    if world > 1:
        parallel.init_from_env('gloo')
    g = load_golden('audio_reg_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, batch_size=3, accum_steps=2, learning_rate=float(g['lr']),
                    loss='mse', sample_weights='balanced')
    m.audio_features = g['feats']; m.audio_targets = g['targs']
    m.model = m.AudioBiLSTM(m.config, seed=0)
    m.model.load_state_dict({k: torch.from_numpy(v) for k, v in _live_start(g).items()})
    m.optimizer = nn.Adam(m.model.parameters(), lr=m.config['learning_rate'], accumulate_steps=2)
    m.criterion = _common.reg_criterion(m.config, nn.L1Loss)
    m.train_dep_idxs = [0, 1, 2, 3]; m.train_non_idxs = [4, 5, 6, 7, 8, 9, 10, 11, 12]      # 13 rows: 3, 3 | 3, 3 | 1 -- rank 1 owns no row of the tail
    with contextlib.redirect_stdout(io.StringIO()):
        mae1 = m.train(1); mae2 = m.train(2)
    if rank == 0:
        q.put(({k: v.cpu().numpy() for k, v in m.model.state_dict().items()}, (float(mae1), float(mae2)), type(m.criterion).__name__,
               int(m.optimizer._step), parallel.loss_weight()))
    if world > 1:
        parallel.barrier()
        import torch.distributed as dist
        dist.destroy_process_group()


def _spawn(world, port):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
def test_two_rank_balanced_mse_training_equals_single_process():
    port = 25100 + os.getpid() % 500
    sd1, mae1, crit1, steps1, left1 = _spawn(1, port)
    sd2, mae2, crit2, steps2, left2 = _spawn(2, port + 2)
    assert crit1 == crit2 == 'MSELoss' and steps1 == steps2 == 6 and left1 is None and left2 is None
    assert np.allclose(mae1, mae2, rtol=0, atol=1e-4), (mae1, mae2)
    start = _live_start(load_golden('audio_reg_train_eval'))
    moved = 0.0
    for k in sd1:
        assert np.abs(sd1[k] - sd2[k]).max() < 2e-6 + 1e-5 * np.abs(sd1[k]).max(), k
        if sd1[k].dtype.kind == 'f':
            moved = max(moved, np.abs(sd1[k] - start[k]).max())
    assert moved > 1e-4                                                # six Adam updates at lr = 1e-3
