"""Class weights, label smoothing and ignore_index in the fused CE losses: the parts that need no GPU.

1. The yardstick of tests/test_weighted_loss_gpu.py is pinned: loss_ref.weighted_ce (float64 numpy) against
   torch.nn.functional.cross_entropy in float64, loss and gradient, for both kinds (the input is z, or softmax(z) for the double
   softmax).  Bound 1e-12: float64 rounding with four orders of margin over the 4.4e-16 measured for the formulas, six orders below
   the fp32 kernel's tolerance.
2. The two numpy helpers of the training loops (class_row_weight, balanced_class_weight) and the script config reader.
3. parallel.loss_weight()'s priority, and train_epoch's declarations with a recording criterion.
4. dep_head_loss_ce / dep_ce_weight_sum / dep_reduce_loss_by refuse bad arguments (DEP_ERR_ARG) before any HIP call.
"""
import numpy as np
import pytest

import loss_ref
from optim_rec import ERR_ARG, lib  # noqa: F401 -- lib is a fixture

torch = pytest.importorskip('torch')

KIND_LOGITS, KIND_ON_SOFTMAX, KIND_L1_RELU, LABELS_I64 = 3, 0, 1, 0x100


# ------------------------------------------------------------------------------------------------ the reference against torch
def _weights(how, C, rng):
    if how == 'none':
        return None
    w = rng.uniform(0.2, 3.0, C)
    if how == 'zero':
        w[C - 1] = 0.0
    return w


def _labels(ignored, B, C, rng):
    y = rng.integers(0, C, B)
    if ignored == 'some':
        y[::3] = -100
    elif ignored == 'all':
        y[:] = -100
    return y


@pytest.mark.parametrize('ignored', ['none', 'some', 'all'])
@pytest.mark.parametrize('how', ['none', 'random', 'zero'])
@pytest.mark.parametrize('eps', [0.0, 0.1, 0.5])
@pytest.mark.parametrize('C', [2, 3, 16])
@pytest.mark.parametrize('B', [1, 37])
def test_reference_equals_torch_cross_entropy_in_float64(B, C, eps, how, ignored):
    rng = np.random.default_rng(1000 * B + 10 * C + int(10 * eps))
    z = rng.standard_normal((B, C)) * 2
    w = _weights(how, C, rng)
    y = _labels(ignored, B, C, rng)
    for kind in loss_ref.KINDS:
        zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        a = zt if kind == 'logits' else torch.softmax(zt, dim=1)
        lt = torch.nn.functional.cross_entropy(a, torch.from_numpy(y), weight=None if w is None else torch.tensor(w, dtype=torch.float64),
                                               label_smoothing=eps, ignore_index=-100)
        lt.backward()
        out, rows, loss, dz = loss_ref.weighted_ce(z, y, kind, w, eps, -100)
        want_loss, want_dz = float(lt.detach()), zt.grad.numpy()
        if loss_ref.denominator(y, w) == 0:
            # den = 0.  No live row: 0 / 0, NaN on both sides.  (B = 1 can also draw the one class of weight 0: a live row over a zero
            # denominator is not finite on either side, and nothing more is claimed for it.)
            if not (y != -100).any():
                assert np.allclose(loss, want_loss, equal_nan=True) and np.isnan(loss)
            assert not np.isfinite(loss) and not np.isfinite(want_loss)
            continue
        assert abs(loss - want_loss) <= 1e-12, (kind, loss, want_loss)
        assert np.abs(dz - want_dz).max() <= 1e-12, kind
        assert np.abs(out - torch.softmax(zt, 1).detach().numpy()).max() <= 1e-15
        assert np.all(rows[y == -100] == 0.0) and np.all(dz[y == -100] == 0.0)


def test_reference_with_an_explicit_denominator_sums_over_shards():
    rng = np.random.default_rng(7)
    B, C = 11, 3
    z = rng.standard_normal((B, C)); y = rng.integers(0, C, B); y[4] = -100
    w = np.array([0.5, 2.0, 1.25])
    for kind in loss_ref.KINDS:
        _, _, loss, dz = loss_ref.weighted_ce(z, y, kind, w, 0.1)
        den = loss_ref.denominator(y, w)
        parts = [loss_ref.weighted_ce(z[a:b], y[a:b], kind, w, 0.1, den=den) for a, b in ((0, 4), (4, 8), (8, 11))]
        assert abs(sum(p[2] for p in parts) - loss) <= 1e-14
        assert np.abs(np.concatenate([p[3] for p in parts]) - dz).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ numpy helpers
def test_class_row_weight():
    from icassp2022_depression_amd._common import class_row_weight
    got = class_row_weight([0, 1, -100, 1, 2], [0.5, 2.0, 3.0])
    assert got.dtype == np.float64 and got.tolist() == [0.5, 2.0, 0.0, 2.0, 3.0]
    assert class_row_weight([7, 1, 0], [1.0, 4.0], ignore_index=7).tolist() == [0.0, 4.0, 1.0]
    assert class_row_weight([], [1.0, 2.0]).tolist() == []
    assert class_row_weight([-100, -100], [1.0, 2.0]).tolist() == [0.0, 0.0]
    with pytest.raises(IndexError):
        class_row_weight([0, 2], [1.0, 2.0])
    with pytest.raises(IndexError):
        class_row_weight([0, -1], [1.0, 2.0])


def test_balanced_class_weight():
    from icassp2022_depression_amd._common import balanced_class_weight, class_row_weight
    y = [0, 0, 0, 1, -100, 0, 1, 0]                    # 7 live rows: 5 of class 0, 2 of class 1
    w = balanced_class_weight(y, 2)
    assert np.allclose(w, [7 / (2 * 5), 7 / (2 * 2)], rtol=1e-15, atol=0)
    assert abs(class_row_weight(y, w).sum() - 7.0) < 1e-12     # the balanced weights keep the weighted row count at n_live
    assert np.allclose(balanced_class_weight([2, 1, 0], 3), [1 / 3 * 3, 1.0, 1.0])
    with pytest.raises(ValueError):
        balanced_class_weight([0, 0, 2], 3)            # no row of class 1
    with pytest.raises(ValueError):
        balanced_class_weight([-100, 0], 2)            # class 1 only in an ignored row
    with pytest.raises(IndexError):
        balanced_class_weight([0, 1, 2], 2)


def test_script_config_reader():
    from icassp2022_depression_amd import _common
    y = np.array([0, 0, 0, 1])
    assert _common.ce_options({'num_classes': 2}, y) == {}
    assert _common.ce_options({'num_classes': 2, 'class_weights': None, 'label_smoothing': 0.0}, y) == {}
    o = _common.ce_options({'num_classes': 2, 'class_weights': [0.5, 2.0]}, y)
    assert o == {'weight': [0.5, 2.0], 'label_smoothing': 0.0}
    o = _common.ce_options({'num_classes': 2, 'class_weights': 'balanced', 'label_smoothing': 0.1}, y)
    assert np.allclose(o['weight'], [4 / 6, 2.0]) and o['label_smoothing'] == 0.1
    assert _common.ce_options({'num_classes': 2, 'label_smoothing': 0.2}, y) == {'weight': None, 'label_smoothing': 0.2}
    with pytest.raises(ValueError):
        _common.ce_options({'num_classes': 2, 'class_weights': [1.0, 2.0, 3.0]}, y)
    with pytest.raises(ValueError):
        _common.ce_options({'num_classes': 2, 'class_weights': 'inverse'}, y)

    class Plain:
        pass
    assert _common.criterion_row_weight(Plain(), y) is None      # a criterion without options: counts only


def test_option_validation_needs_no_device():
    from icassp2022_depression_amd import nn
    o = nn.CEOptions()
    assert not o.active and o.ignore_index == -100 and o.label_smoothing == 0.0 and o.weight is None
    assert nn.CEOptions(label_smoothing=0.1).active and nn.CEOptions(ignore_index=3).active
    for kw in (dict(reduction='sum'), dict(reduction='none'), dict(label_smoothing=-0.1), dict(label_smoothing=1.0),
               dict(label_smoothing=float('nan')), dict(weight=[1.0, -2.0]), dict(weight=[]), dict(weight=[1.0, float('inf')]),
               dict(ignore_index=1.5)):
        with pytest.raises(ValueError):
            nn.CEOptions(**kw)
        with pytest.raises(ValueError):
            nn.CrossEntropyLoss(**kw)
    assert nn.CEOptions(label_smoothing=0.1).row_weight([1, -100, 0]).tolist() == [1.0, 0.0, 1.0]
    t = torch.tensor([0, -100, 1])
    nn._check_labels(t, 2, -100)                                  # an ignored label is not out of range
    with pytest.raises(IndexError):
        nn._check_labels(t, 2)
    with pytest.raises(IndexError):
        nn._check_labels(torch.tensor([0, -100, 2]), 2, -100)


# ------------------------------------------------------------------------------------------------ declared denominators
def test_loss_weight_priority(monkeypatch):
    from icassp2022_depression_amd import parallel
    try:
        assert parallel.loss_weight() is None
        parallel.set_global_weight(12.5)
        assert parallel.loss_weight() is None                     # one rank: a global weight is not consulted
        monkeypatch.setattr(parallel, 'world_size', lambda: 2)
        assert parallel.loss_weight() == 12.5
        parallel.set_accumulated_weight(40.0)
        assert parallel.loss_weight() == 40.0                     # accumulated over global
        parallel.set_global_weight(None)
        assert parallel.loss_weight() == 40.0
        monkeypatch.setattr(parallel, 'world_size', lambda: 1)
        assert parallel.loss_weight() == 40.0                     # ... on one rank too
        parallel.set_accumulated_weight(None)
        assert parallel.loss_weight() is None
        parallel.set_global_weight(3)
        parallel.set_global_weight(None)
        monkeypatch.setattr(parallel, 'world_size', lambda: 2)
        assert parallel.loss_weight() is None                     # None clears
        assert parallel.loss_count(5) == 5                        # the counts are a protocol of their own
    finally:
        parallel.set_accumulated_weight(None); parallel.set_global_weight(None)


class _Model:
    device = torch.device('cpu')


def _recording_loop(monkeypatch, accumulate_steps, row_weight, n_rows=11, batch=4):
    from icassp2022_depression_amd import _common, nn, parallel
    log = []
    for name in ('set_global_weight', 'set_accumulated_weight'):
        real = getattr(parallel, name)
        monkeypatch.setattr(parallel, name, lambda w, name=name, real=real: (log.append((name, w)), real(w))[1])

    class Opt:
        def zero_grad(self):
            pass

        def step(self):
            pass

        def flush(self):
            log.append(('flush',))
    Opt.accumulate_steps = accumulate_steps

    def criterion(a, b):
        log.append(('criterion', a, b, parallel._global_weight[0], parallel._accum_weight[0], parallel.loss_weight()))
        return nn.Loss(torch.tensor([1.0]), lambda: None)

    def step(a, b, then):
        return criterion(a, b), None

    total = _common.train_epoch(_Model(), Opt(), n_rows, batch, step, row_weight=row_weight)
    assert total == float(len(range(0, n_rows, batch)))
    assert parallel._global_weight[0] is None and parallel._accum_weight[0] is None and parallel.loss_weight() is None
    return log


@pytest.mark.parametrize('K', [1, 3])
def test_train_epoch_declares_the_row_weight_sums(monkeypatch, K):
    rw = np.array([0.5, 2.0, 0.0, 2.0, 0.5, 0.5, 2.0, 2.0, 0.0, 0.5, 2.0])          # 11 rows, batch 4: 4 + 4 + 3 (ragged)
    sums = [rw[0:4].sum(), rw[4:8].sum(), rw[8:11].sum()]
    log = _recording_loop(monkeypatch, K, rw)
    crit = [e for e in log if e[0] == 'criterion']
    assert [(e[1], e[2]) for e in crit] == [(0, 4), (4, 8), (8, 11)]
    assert [e[3] for e in crit] == sums                                             # each global mini-batch's sum, in front of its criterion
    if K == 1:
        assert [e[4] for e in crit] == [None] * 3 and [e[5] for e in crit] == [None] * 3      # one rank: the criterion sums its own
        assert [e for e in log if e[0] != 'criterion'] == [('set_global_weight', s) for s in sums] + \
            [('set_accumulated_weight', None), ('set_global_weight', None)]
    else:
        assert [e[4] for e in crit] == [rw.sum()] * 3 and [e[5] for e in crit] == [rw.sum()] * 3   # one group of three: the 11 rows' sum
        assert log[0] == ('set_global_weight', sums[0]) and log[1] == ('set_accumulated_weight', rw.sum())
        assert log[-3:] == [('flush',), ('set_accumulated_weight', None), ('set_global_weight', None)]
        assert [e for e in log if e[0] == 'set_accumulated_weight'] == [('set_accumulated_weight', rw.sum()), ('set_accumulated_weight', None)]


def test_train_epoch_cuts_accumulation_groups_at_their_mini_batches(monkeypatch):
    rw = np.arange(1.0, 12.0)                                                       # 11 rows, batch 2, K = 2: groups of 4, 4, 3 rows
    log = _recording_loop(monkeypatch, 2, rw, batch=2)
    acc = [e[1] for e in log if e[0] == 'set_accumulated_weight']
    assert acc == [rw[0:4].sum(), rw[4:8].sum(), rw[8:11].sum(), None]
    crit = [e for e in log if e[0] == 'criterion']
    assert [e[5] for e in crit] == [rw[0:4].sum()] * 2 + [rw[4:8].sum()] * 2 + [rw[8:11].sum()] * 2


def test_train_epoch_without_row_weight_never_calls_the_new_setters(monkeypatch):
    assert _recording_loop(monkeypatch, 1, None) == [('criterion', 0, 4, None, None, None), ('criterion', 4, 8, None, None, None),
                                                    ('criterion', 8, 11, None, None, None)]
    log = _recording_loop(monkeypatch, 3, None)
    assert [e[0] for e in log] == ['criterion'] * 3 + ['flush']
    from icassp2022_depression_amd import _common
    with pytest.raises(ValueError):
        _common.train_epoch(_Model(), None, 11, 4, None, row_weight=np.ones(10))   # one entry per training row


# ------------------------------------------------------------------------------------------------ argument refusals
def test_entry_points_refuse_bad_arguments(lib):
    ok = 0x1000                                                       # never dereferenced on the host: the checks come first

    def ce(kind=KIND_LOGITS, z=ok, target=ok, cw=None, eps=0.0, ignore=-100, out=None, rows=ok, dz=ok, B=4, C=3, norm=4.0, norm_dev=None):
        return lib.dep_head_loss_ce(kind, z, target, cw, eps, ignore, out, rows, dz, B, C, norm, norm_dev, None)
    for kw in (dict(kind=KIND_L1_RELU), dict(kind=2), dict(kind=4), dict(kind=KIND_L1_RELU | LABELS_I64), dict(kind=5), dict(kind=-1),
               dict(C=17), dict(C=0), dict(B=0), dict(eps=-0.1), dict(eps=1.0), dict(eps=float('nan')), dict(z=None),
               dict(norm=0.0), dict(norm=-1.0), dict(norm=float('nan')), dict(target=None)):
        assert ce(**kw) == ERR_ARG, kw
        assert b'bad argument' in lib.dep_last_error()
    ws = lib.dep_ce_weight_sum
    assert ws(None, 0, ok, -100, 4, 3, ok, None) == ERR_ARG
    assert ws(ok, 0, ok, -100, 4, 3, None, None) == ERR_ARG
    assert ws(ok, 1, None, -100, 0, 3, ok, None) == ERR_ARG
    assert ws(ok, 1, None, -100, 4, 17, ok, None) == ERR_ARG
    assert ws(ok, 1, None, -100, 4, 0, ok, None) == ERR_ARG
    rb = lib.dep_reduce_loss_by
    assert rb(None, 4, ok, ok, 0, None) == ERR_ARG
    assert rb(ok, 4, None, ok, 0, None) == ERR_ARG
    assert rb(ok, 4, ok, None, 0, None) == ERR_ARG
    assert rb(ok, 0, ok, ok, 0, None) == ERR_ARG


def test_binding_lists_the_new_entry_points(lib):
    from icassp2022_depression_amd import _lib
    for name in ('dep_head_loss_ce', 'dep_ce_weight_sum', 'dep_reduce_loss_by'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert callable(_lib.head_loss_ce) and callable(_lib.ce_weight_sum) and callable(_lib.reduce_loss_by)
