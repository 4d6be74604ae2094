"""Class weights, label smoothing and ignore_index in the fused CE losses, on the device: dep_head_loss_ce / dep_ce_weight_sum /
dep_reduce_loss_by, nn.CrossEntropyLoss(weight, ignore_index, label_smoothing), the fusion loss, and the declared denominators of the
training loops (accumulation, data parallelism, the scripts' config).

Yardstick: loss_ref.weighted_ce (float64 numpy, pinned to torch in tests/test_weighted_loss_cpu.py).  Tolerances are the ones
tests/test_small_kernels_gpu.py applies to dep_head_loss -- out 1e-6 absolute, dz relerr < 1e-5, loss 1e-6 max(1, |loss|), per-row
losses 1e-6 max(1, max |rows|) -- since the new entry evaluates the same functions of the same magnitudes; the loops are held to
tests/test_accum_gpu.py's bars against one big batch (parameters 2e-5 + 1e-4 max|v|, gradients relerr 1e-3, summed loss 1e-4) and to
tests/test_dp_gpu.py's 2e-6 against one process.
Run on the MI355X box:  python -m pytest tests/test_weighted_loss_gpu.py -m gpu -q"""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

import loss_ref
from conftest import ROOT, load_golden

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L, nn, parallel
    from icassp2022_depression_amd import audio_gru_whole, text_bilstm_whole
    DEV = torch.device('cuda:0')

F32 = np.float32
KINDS = {'logits': 'LOSS_CE_LOGITS', 'on_softmax': 'LOSS_CE_ON_SOFTMAX'}


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


def labels_with_both_ends(rng, B, C):
    y = rng.integers(0, C, B)
    y[-1] = C - 1
    if B > 1:
        y[0] = 0
    return y


def class_weights(how, C, rng):
    """none / random in [0.2, 3] / one weight exactly 0 (class 0: every B > 1 case holds a row of it, and the B = 1 case a live weight)."""
    if how == 'none':
        return None
    w = r32(rng.uniform(0.2, 3.0, C))
    if how == 'zero':
        w[0] = 0.0
    return w


def buffers(B, C):
    return (torch.full((B, C), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV), torch.full((B, C), 7.0, device=DEV),
            torch.full((1,), float('nan'), device=DEV))


def check_against_reference(tag, out, rows, dz, loss, ref, y):
    p, rows_ref, loss_ref_, dz_ref = ref
    got_loss = host(loss)[0]
    print('%s: out %.3g  rows %.3g  dz relerr %.3g  loss %.9g (ref %.9g)' % (
        tag, np.abs(host(out) - p).max(), np.abs(host(rows) - rows_ref).max(), relerr(host(dz), dz_ref), got_loss, loss_ref_))
    assert np.abs(host(out) - p).max() < 1e-6, tag
    assert np.abs(host(rows) - rows_ref).max() < 1e-6 * max(1.0, np.abs(rows_ref).max()), tag
    assert relerr(host(dz), dz_ref) < 1e-5, tag
    assert abs(got_loss - loss_ref_) < 1e-6 * max(1.0, abs(loss_ref_)), tag
    ign = y == -100
    assert np.all(host(rows)[ign] == 0.0) and np.all(host(dz)[ign] == 0.0), tag        # exactly zero, not merely small


# ------------------------------------------------------------------------------------------------ kernel parity
# the block is 128 rows and the class arrays hold 16: one row, one short of / exactly / one past a block, several blocks; C = 2, 3, 16
GRID = [(1, 2), (127, 3), (128, 16), (129, 2), (300, 16)]


@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('B,C', GRID)
def test_kernel_against_the_reference(B, C, kind):
    rng = np.random.default_rng(100 * B + C)
    z = r32(rng.standard_normal((B, C)) * 2)
    zd = dev(z)
    k = getattr(L, KINDS[kind])
    for eps in (0.0, 0.1):
        for how in ('none', 'random', 'zero'):
            for ignore in (False, True):
                w = class_weights(how, C, rng)
                y = labels_with_both_ends(rng, B, C)
                if ignore:
                    y[2::3] = -100                                    # every third row
                wd = None if w is None else dev(w)
                y32 = torch.from_numpy(y.astype(np.int32)).to(DEV); y64 = torch.from_numpy(y.astype(np.int64)).to(DEV)
                ref = loss_ref.weighted_ce(z, y, kind, w, eps, -100)
                den_ref = loss_ref.denominator(y, w)
                assert den_ref > 0
                tag = '%s B=%d C=%d eps=%g w=%s ignore=%s' % (kind, B, C, eps, how, ignore)
                # (a) the host norm
                norm = float(F32(den_ref))
                out, rows, dz, loss = buffers(B, C)
                L.head_loss_ce(k, zd, y32, out, rows, dz, norm, wd, eps, -100)
                L.reduce_loss(rows, norm, loss)
                check_against_reference(tag + ' host norm', out, rows, dz, loss, ref, y)
                out64, rows64, dz64, _ = buffers(B, C)
                L.head_loss_ce(k | L.LOSS_LABELS_I64, zd, y64, out64, rows64, dz64, norm, wd, eps, -100)
                assert torch.equal(out64, out) and torch.equal(rows64, rows) and torch.equal(dz64, dz), tag     # torch.long labels read in place
                # (b) the denominator summed on the device, read through norm_dev
                den = torch.full((1,), float('nan'), device=DEV)
                L.ce_weight_sum(y32, wd, -100, C, den)
                assert abs(host(den)[0] - den_ref) <= 1e-6 * den_ref, tag     # <= 2 terms per thread + a 64-lane and a 4-wave tree: ~10 roundings of 6e-8
                den64 = torch.full((1,), float('nan'), device=DEV)
                L.ce_weight_sum(y64, wd, -100, C, den64)
                assert torch.equal(den64, den), tag
                out, rows, dz, loss = buffers(B, C)
                L.head_loss_ce(k, zd, y32, out, rows, dz, den, wd, eps, -100)
                L.reduce_loss_by(rows, den, loss)
                check_against_reference(tag + ' device norm', out, rows, dz, loss, ref, y)


@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('B,C', [(129, 3), (300, 16)])
def test_neutral_options_are_bit_identical_to_dep_head_loss(B, C, kind):
    rng = np.random.default_rng(7 * B + C)
    zd = dev(rng.standard_normal((B, C)) * 2)
    y = labels_with_both_ends(rng, B, C)
    k = getattr(L, KINDS[kind])
    for yd, wide in ((torch.from_numpy(y.astype(np.int32)).to(DEV), 0), (torch.from_numpy(y.astype(np.int64)).to(DEV), L.LOSS_LABELS_I64)):
        out0, rows0, dz0, loss0 = buffers(B, C)
        L.head_loss(k | wide, zd, yd, out0, rows0, dz0, B)
        L.reduce_loss(rows0, B, loss0)
        out1, rows1, dz1, loss1 = buffers(B, C)
        L.head_loss_ce(k | wide, zd, yd, out1, rows1, dz1, B, None, 0.0, -100)
        L.reduce_loss(rows1, B, loss1)
        assert torch.equal(out1, out0) and torch.equal(rows1, rows0) and torch.equal(dz1, dz0) and torch.equal(loss1, loss0)
        # the count summed on the device is exactly B: the same bits again
        den = torch.full((1,), float('nan'), device=DEV)
        L.ce_weight_sum(yd, None, -100, C, den)
        assert host(den)[0] == float(B)
        out2, rows2, dz2, loss2 = buffers(B, C)
        L.head_loss_ce(k | wide, zd, yd, out2, rows2, dz2, den, None, 0.0, -100)
        L.reduce_loss_by(rows2, den, loss2)
        assert torch.equal(out2, out0) and torch.equal(rows2, rows0) and torch.equal(dz2, dz0) and torch.equal(loss2, loss0)


def test_saturated_logits_stay_finite_with_weights_and_smoothing():
    """Logits 120 apart, as in tests/test_small_kernels_gpu.py::test_saturated_logits_have_exact_outcomes: the softmax is exactly one-hot
    and -log q of the other classes is 120 (CE_LOGITS), large but finite; nothing overflows with weights and eps = 0.1 on top."""
    for zs, ys, w in (([(60, -60), (60, -60), (-60, 60), (-60, 60)], [0, 1, 1, 0], [0.5, 2.0]),
                      ([(-60, 60, -60), (-60, 60, -60), (-60, 60, -60), (60, -60, -60), (-60, -60, 60)], [1, 0, 2, 0, 1], [0.25, 3.0, 1.0])):
        z = np.array(zs, dtype=np.float64); y = np.array(ys); w = np.array(w)
        B, C = z.shape
        zd = dev(z); yd = torch.from_numpy(y.astype(np.int32)).to(DEV); wd = dev(w)
        onehot_max = (z == z.max(1, keepdims=True)).astype(np.float64)
        for kind in KINDS:
            ref = loss_ref.weighted_ce(z, y, kind, w, 0.1)
            norm = float(F32(loss_ref.denominator(y, w)))
            out, rows, dz, loss = buffers(B, C)
            L.head_loss_ce(getattr(L, KINDS[kind]), zd, yd, out, rows, dz, norm, wd, 0.1, -100)
            L.reduce_loss(rows, norm, loss)
            assert np.array_equal(host(out), onehot_max)
            assert np.isfinite(host(rows)).all() and np.isfinite(host(dz)).all() and np.isfinite(host(loss)).all()
            assert np.abs(host(rows) - ref[1]).max() <= 1e-6 * max(1.0, np.abs(ref[1]).max())
            assert relerr(host(dz), ref[3]) < 1e-5


def test_all_rows_ignored_gives_nan():
    B, C = 3, 2
    zd = dev(np.random.default_rng(0).standard_normal((B, C)))
    yd = torch.full((B,), -100, dtype=torch.int64, device=DEV)
    den = torch.full((1,), 5.0, device=DEV)
    L.ce_weight_sum(yd, None, -100, C, den)
    assert host(den)[0] == 0.0
    out, rows, dz, loss = buffers(B, C)
    L.head_loss_ce(L.LOSS_CE_LOGITS | L.LOSS_LABELS_I64, zd, yd, out, rows, dz, den, None, 0.1, -100)
    L.reduce_loss_by(rows, den, loss)
    assert np.isnan(host(loss)[0])


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


def _classifier(name):
    mod, cls = {'audio': (audio_gru_whole, 'AudioBiLSTM'), 'text': (text_bilstm_whole, 'TextBiLSTM')}[name]
    cfg = dict(mod.config); cfg.update(embedding_size=8, hidden_dims=16, dropout=0.0)
    model = getattr(mod, cls)(cfg, seed=3)
    model.train()
    x = np.random.default_rng(5).standard_normal((9, 6, 8)).astype(np.float32)
    return model, x


@pytest.mark.parametrize('name', ['audio', 'text'])
def test_criterion_with_options_against_the_reference(name):
    model, x = _classifier(name)
    w = np.array([0.5, 2.0])
    y = np.array([0, 1, 1, 0, -100, 1, 0, 0, 1])
    crit = nn.CrossEntropyLoss(weight=torch.tensor(w, dtype=torch.float32), label_smoothing=0.1)
    expect = {'host': ['head_loss_ce_kernel<true>', 'reduce_loss_kernel'],
              'device': ['ce_weight_sum_kernel', 'head_loss_ce_kernel<true>', 'reduce_loss_by_kernel']}      # one launch more, no host read
    for where, labels in (('host', torch.from_numpy(y)), ('device', torch.from_numpy(y).to(DEV)), ('host', y.astype(np.int32))):
        output = model(x)
        loss, kernels = _kernels_logged(lambda: crit(output, labels))
        assert kernels == expect[where], kernels
        _, _, loss_want, dz_want = loss_ref.weighted_ce(host(output._z), y, 'on_softmax', w, 0.1, -100)
        got = loss.item()
        print('%s %s labels: loss %.9g (ref %.9g), dz relerr %.3g' % (name, where, got, loss_want, relerr(host(loss.dz), dz_want)))
        assert abs(got - loss_want) < 1e-6 * max(1.0, abs(loss_want))
        assert relerr(host(loss.dz), dz_want) < 1e-5 and np.all(host(loss.dz)[4] == 0.0)
        loss.backward()                                                # the backward starts from that tensor
        model.check_health()
    # evaluate(): the batch's own denominator, no gradient
    model.eval()
    loss = crit(model(x), y)
    assert loss.dz is None and abs(loss.item() - loss_ref.weighted_ce(host(model(x)._z), y, 'on_softmax', w, 0.1)[2]) < 1e-6
    with pytest.raises(ValueError):
        nn.CrossEntropyLoss(weight=[1.0, 2.0, 3.0])(model(x), y)       # three weights, two classes
    with pytest.raises(IndexError):
        crit(model(x), np.array([0, 1, 1, 0, -100, 1, 0, 2, 1]))       # class 2 of 2 is still out of range


def test_default_criterion_enqueues_what_the_unweighted_path_enqueues():
    model, x = _classifier('audio')
    y = np.array([0, 1, 1, 0, 1, 1, 0, 0, 1])

    class Unweighted(nn._HeadLoss):                                    # the path every criterion took before the options existed
        kind = L.LOSS_CE_ON_SOFTMAX
        target_dtype = 'int'

    output = model(x)
    old, log_old = _kernels_logged(lambda: Unweighted()(output, y))
    new, log_new = _kernels_logged(lambda: nn.CrossEntropyLoss()(output, y))
    assert log_new == log_old == ['head_loss_kernel', 'reduce_loss_kernel']
    assert torch.equal(new._v, old._v) and torch.equal(new.dz, old.dz)
    # ... also after a criterion with options ran in the same process
    nn.CrossEntropyLoss(label_smoothing=0.1)(output, y)
    again, log_again = _kernels_logged(lambda: nn.CrossEntropyLoss(weight=None, ignore_index=-100, label_smoothing=0.0)(output, y))
    assert log_again == log_old and torch.equal(again._v, old._v)


def test_fusion_classification_loss_shares_one_denominator():
    from icassp2022_depression_amd import fuse_net_whole as m
    g = load_golden('fuse_clf')
    N, T, Fa, Ft, Ha, Ht = [int(v) for v in g['dims']]
    saved_cfg = dict(m.config)
    try:
        m.config.update(audio_embed_size=Fa, text_embed_size=Ft, audio_hidden_dims=Ha, text_hidden_dims=Ht, dropout=0.0,
                        learning_rate=float(g['lr']))
        model = m.build(seed=0)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
        model.eval()
        tf, af = model.pretrained_feature([[g['xa'][i], g['xt'][i]] for i in range(N)])
        model.train()
        y = np.asarray(g['y']).astype(np.int64).copy()
        assert set(y.tolist()) == {0, 1}
        y[1] = -100
        w = np.array([0.5, 2.0])
        crit = m.MyLoss(weight=w, label_smoothing=0.1)
        loss = crit(tf, af, y, model)
        W = dict(model.named_parameters())['fc_final.0.weight'].data
        Cc, D = W.shape
        zt = torch.empty(N, Cc, device=DEV); za = torch.empty(N, Cc, device=DEV)      # the halves' logits, by the calls the loss makes
        L.gemm(0, 1, N, Cc, Ht, tf, Ht, W, D, zt, Cc)
        L.gemm(0, 1, N, Cc, Ha, af, Ha, W[:, Ht:], D, za, Cc)
        den = loss_ref.denominator(y, w)
        rt = loss_ref.weighted_ce(host(zt), y, 'logits', w, 0.1, den=den)
        ra = loss_ref.weighted_ce(host(za), y, 'logits', w, 0.1, den=den)
        want = rt[2] + ra[2]
        got = loss.item()
        print('fusion: loss %.9g (ref %.9g)' % (got, want))
        assert abs(got - want) < 1e-6 * max(1.0, abs(want))
        dzt, dza = loss.dz_halves
        assert relerr(host(dzt), rt[3]) < 1e-5 and relerr(host(dza), ra[3]) < 1e-5
        assert np.all(host(dzt)[1] == 0.0) and np.all(host(dza)[1] == 0.0)
        loss.backward()
        gW = host(dict(model.named_parameters())['fc_final.0.weight'].grad)
        want_gW = np.concatenate([rt[3].T @ host(tf), ra[3].T @ host(af)], axis=1)
        assert relerr(gW, want_gW) < 1e-4                                            # two small fp32 GEMMs over the checked dz
        # defaults: the launches the loss always enqueued
        _, log = _kernels_logged(lambda: m.MyLoss()(tf, af, np.asarray(g['y']), model))
        assert [k for k in log if 'loss' in k] == ['head_loss_kernel', 'reduce_loss_kernel'] * 2
        with pytest.raises(ValueError):
            from icassp2022_depression_amd import models
            models.MyLoss('reg', label_smoothing=0.1)
    finally:
        m.config.clear(); m.config.update(saved_cfg)


# ------------------------------------------------------------------------------------------------ training loops
def _audio_fixture(m, **cfg):
    g = load_golden('audio_clf_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, learning_rate=float(g['lr']), **cfg)
    m.audio_features = g['feats']; m.audio_targets = g['targs']
    model = m.AudioBiLSTM(m.config, seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
    return g, model


def test_accumulated_weighted_epoch_equals_one_big_batch():
    """11 rows as micro-batches of 4, 4, 3 (ragged) accumulated into ONE update, every criterion dividing by the declared weight of
    the 11 rows, against one 11-row step of a plain optimizer whose criterion sums its own denominator from host labels."""
    m = audio_gru_whole
    saved_cfg = dict(m.config)
    try:
        g, m.model = _audio_fixture(m, batch_size=4, accum_steps=3, class_weights=[0.5, 2.0], label_smoothing=0.1)
        idx = list(range(11))
        assert set(np.asarray(m.audio_targets)[idx].tolist()) == {0, 1}
        m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate'], accumulate_steps=3)
        m.criterion = m.make_criterion(idx)
        assert m.criterion.options.active and m.criterion.options.weight.tolist() == [0.5, 2.0]
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            m.train(1, idx)
        assert m.optimizer._step == 1 and m.optimizer.pending == 0
        assert parallel.loss_weight() is None and parallel._global_weight[0] is None            # nothing stays declared
        total = float(out.getvalue().split('Loss:')[1].split()[0])
        # the big batch
        _, big = _audio_fixture(m)
        opt = nn.AdamW(m.get_param_group(big), lr=m.config['learning_rate'])
        big.train()
        y = np.asarray(m.audio_targets)[idx]
        loss = nn.CrossEntropyLoss(weight=[0.5, 2.0], label_smoothing=0.1)(big(m.audio_features[idx]), torch.from_numpy(y.astype(np.int64)))
        loss.backward()
        grads = {k: host(p.grad).copy() for k, p in big.named_parameters() if p.grad is not None}
        opt.step()
        assert len(grads) >= 10
        for k, p in m.model.named_parameters():
            if k in grads:
                e = relerr(host(m.optimizer.accumulated_grad(p)), grads[k])
                assert e < 1e-3, (k, e)
        sd, sd_big = m.model.state_dict(), big.state_dict()
        for k in sd:
            v = host(sd_big[k])
            assert np.abs(host(sd[k]) - v).max() < 2e-5 + 1e-4 * np.abs(v).max(), k
        assert abs(total - loss.item()) < 1e-4 * max(1.0, abs(loss.item()))                   # the micro-losses sum to the big batch's
    finally:
        m.config.clear(); m.config.update(saved_cfg)
        parallel.set_accumulated_weight(None); parallel.set_global_weight(None); parallel.set_accumulated_count(None)


def test_script_train_equals_a_written_out_loop_on_host_labels():
    """audio_gru_whole.train() (device-resident labels, the denominators its loop declares / dep_ce_weight_sum) against the loop
    written out here, whose criterion sees host labels and sums its own denominator in float64."""
    m = audio_gru_whole
    saved_cfg = dict(m.config)
    try:
        torch.manual_seed(2024)
        g, m.model = _audio_fixture(m, batch_size=4, class_weights=[0.5, 2.0], label_smoothing=0.1)
        idx = list(range(15))                                   # 4, 4, 4, 3
        m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate'])
        m.criterion = m.make_criterion(idx)
        quiet(m.train, 1, idx)
        assert m.optimizer._step == 4
        _, ref = _audio_fixture(m)
        opt = nn.AdamW(m.get_param_group(ref), lr=m.config['learning_rate'])
        crit = nn.CrossEntropyLoss(weight=[0.5, 2.0], label_smoothing=0.1)
        ref.train()
        X, Y = m.audio_features[idx], np.asarray(m.audio_targets)[idx].astype(np.int64)
        for a in range(0, 15, 4):
            opt.zero_grad()
            loss = crit(ref(X[a:a + 4]), torch.from_numpy(Y[a:a + 4]))
            loss.backward()
            opt.step()
        sd, sd_ref = m.model.state_dict(), ref.state_dict()
        moved = 0.0
        for k in sd:
            v = host(sd_ref[k])
            assert np.abs(host(sd[k]) - v).max() < 2e-5 + 1e-4 * np.abs(v).max(), k
            moved = max(moved, np.abs(v - g['sd'][k]).max())
        assert moved > 0
        # defaults: today's criterion, no row weights
        m.config.pop('class_weights'); m.config.pop('label_smoothing')
        plain = m.make_criterion(idx)
        assert type(plain) is nn.CrossEntropyLoss and not plain.options.active
        from icassp2022_depression_amd import _common
        assert _common.criterion_row_weight(plain, Y) is None
    finally:
        m.config.clear(); m.config.update(saved_cfg)


# ------------------------------------------------------------------------------------------------ data parallel
def _run_rank(rank, world, port, q):
    # gloo: the ranks share cuda:0 (as tests/test_dp_gpu.py runs them)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    sys.path.insert(0, ROOT)
    from icassp2022_depression_amd import audio_gru_whole as m, nn, parallel
    if world > 1:
        parallel.init_from_env('gloo')
    g = load_golden('audio_clf_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, batch_size=4, learning_rate=float(g['lr']),
                    class_weights='balanced', label_smoothing=0.1)
    m.audio_features = g['feats']; m.audio_targets = g['targs']
    m.model = m.AudioBiLSTM(m.config, seed=0)
    m.model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
    m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate'])
    idx = list(range(17))                     # batches of 4, 4, 4, 4, 1: rank 1 owns no row of the tail batch
    m.criterion = m.make_criterion(idx)
    with contextlib.redirect_stdout(io.StringIO()):
        m.train(1, idx); m.train(2, idx)
    if rank == 0:
        q.put(({k: v.cpu().numpy() for k, v in m.model.state_dict().items()}, int(m.train_acc),
               m.criterion.options.weight.tolist(), parallel.loss_weight()))
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
def test_two_rank_balanced_training_equals_single_process():
    port = 24100 + os.getpid() % 500
    sd1, acc1, w1, left1 = _spawn(1, port)
    sd2, acc2, w2, left2 = _spawn(2, port + 2)
    y = np.asarray(load_golden('audio_clf_train_eval')['targs'])[:17]
    counts = np.bincount(y.astype(np.int64), minlength=2)
    assert np.allclose(w1, 17 / (2 * counts), rtol=1e-15, atol=0) and w2 == w1 and counts.min() > 0 and counts[0] != counts[1]
    assert left1 is None and left2 is None and acc1 == acc2
    for k in sd1:
        assert np.abs(sd1[k] - sd2[k]).max() < 2e-6, k
