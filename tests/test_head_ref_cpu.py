"""CPU checks of what tests/test_head_forms_gpu.py stands on (tests/head_ref.py): the float64 reference against stock torch, what the case table
reaches, that a lost batch row would show under the bars, and how much of the 5e-6 gradient bar float32 summation in the weight pass's own order
uses up at the largest batches."""
import numpy as np
import pytest

import head_ref as H

torch = pytest.importorskip('torch')


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('C', [0, 1, 5])
@pytest.mark.parametrize('p,first', [(0.0, False), (0.0, True), (0.5, False), (0.5, True)])
def test_reference_is_stock_torch_in_float64(C, p, first):
    B, Hin, H1 = 7, 16, 8
    c = H.Case('pin', B, Hin, H1, C, p, first)
    d = H.inputs(c)
    r = H.reference(c)
    assert (d['m0'] is not None) == (first and p > 0) and (d['m1'] is not None) == (p > 0)
    t = lambda a: torch.from_numpy(H.f64(a))
    ones = lambda m, *s: torch.ones(*s, dtype=torch.float64) if m is None else torch.from_numpy(m)
    x, W1, b1 = t(d['x']).requires_grad_(), t(d['W1']).requires_grad_(), t(d['b1']).requires_grad_()
    a0 = x * ones(d['m0'], B, Hin)
    z1 = torch.nn.functional.linear(a0, W1, b1)
    a1 = torch.relu(z1) * ones(d['m1'], B, H1)
    close = lambda a, b: H.relerr(a, b.detach().numpy()) < 1e-12
    assert close(r['a0'], a0) and close(r['z1'], z1) and close(r['a1'], a1)
    if p > 0:                                                        # the masks are masks: 0 or 1 / (1 - p), both present
        assert set(np.unique(d['m1'])) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    if not C:
        assert r['z2'] is None and 'dW1' not in r
        return
    W2, b2 = t(d['W2']).requires_grad_(), t(d['b2']).requires_grad_()
    z1.retain_grad()
    z2 = torch.nn.functional.linear(a1, W2, b2)
    assert close(r['z2'], z2)
    z2.backward(t(d['dz2']))
    for k, g in (('dz1', z1.grad), ('dW1', W1.grad), ('db1', b1.grad), ('dW2', W2.grad), ('db2', b2.grad), ('dx', x.grad)):
        assert close(r[k], g), k
        assert r[k].any(), k


def test_masks_index_by_row_times_width_plus_column():
    m0, m1 = H.masks(5, 8, 16, 0.3, 77, (9, 11), True)
    flat = H.R.dropout_mask(5 * 16, 0.3, 77, 11).astype(np.float64)
    assert m1[3, 7] == flat[3 * 16 + 7] and (m1.reshape(-1) == flat).all()
    assert (m0.reshape(-1) == H.R.dropout_mask(40, 0.3, 77, 9)).all()
    assert H.masks(5, 8, 16, 0.3, 77, (9, 11), False)[0] is None and H.masks(5, 8, 16, 0.0, 77, (9, 11), True) == (None, None)


# ----------------------------------------------------------------------------- the case table
def test_case_table_reaches_every_instance_and_edge():
    cs = H.CASES
    assert len(set(cs)) == len(cs) and all(H.supported(c.Hin, c.H1, c.C) for c in cs)
    ragged = [c for c in cs if c.B % H.HR]
    assert {H.fwd_instance(c.Hin) for c in ragged} | {H.rows_instance(c.H1) for c in ragged if c.C} | {H.W_INSTANCE} == H.ALL_INSTANCES
    assert len(H.ALL_INSTANCES) == 13
    A = H.section('A')
    assert {(c.Hin, c.H1) for c in A} == set(H.INSTANCE_SHAPES) and len(A) == 24
    assert all(c.B == 5 and c.C == 2 for c in A) and {(c.p, c.first) for c in A} == {(0.0, False), (0.5, True), (0.3, False)}
    Bs = [c for c in H.section('B') if (c.Hin, c.H1, c.C) == (32, 16, 5)]
    assert [c.B for c in Bs] == [1, 3, 4, 5, 8, 9, 15, 16, 17, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2049]
    assert all(c.p == 0.5 and c.first for c in Bs)
    wide = [c for c in H.section('B') if (c.Hin, c.H1, c.C) == (256, 256, 16)]
    assert [c.B for c in wide] == [513, 1025, 2049] and all(c.p == 0 for c in wide)
    Cs = H.section('C')
    assert [c.C for c in Cs] == [0, 1, 3, 4, 5, 15, 16] and all((c.B, c.Hin, c.H1) == (37, 64, 64) for c in Cs)
    assert {(c.Hin, c.H1, c.C, c.B) for c in H.section('D')} == {(32, 16, 5, 5), (32, 16, 5, 1025), (256, 256, 2, 5), (256, 256, 2, 1025)}
    assert not any(H.supported(*s) for s in H.REFUSED)
    assert {s[2] for s in H.REFUSED} >= {17} and {4, 24, 512} <= {s[0] for s in H.REFUSED} & {s[1] for s in H.REFUSED}
    # x, W1, b1 and the masks do not depend on C: the C = 0 run of section C can be held to the C = 5 run's bits
    a, b = H.inputs(Cs[0]), H.inputs(Cs[4])
    assert a['x'] is b['x'] and a['W1'] is b['W1'] and a['seed'] == b['seed'] and a['dz2'] is None and b['dz2'].shape == (37, 5)


def test_weight_pass_geometry():
    """wave_rows / probe_rows restate head.hip's split of the batch; the batch edges of section B are where that split changes."""
    for B in (1, 5, 8, 9, 513, 1024, 1025, 2049):
        rows = H.wave_rows(B)
        assert sorted(r for w in rows for r in w) == list(range(B))
    assert [len(w) for w in H.wave_rows(8)] == [1] * 8 and [len(w) for w in H.wave_rows(9)] == [2, 2, 2, 2, 1, 0, 0, 0]
    assert [len(w) for w in H.wave_rows(1025)] == [129] + [128] * 7 and H.wave_rows(1025)[0][-1] == 1024        # a last round of one row: wave 0's
    assert H.wave_rows(2049)[0][126:130] == [126, 127, 1024, 1025] and H.wave_rows(2049)[0][-3:] == [1150, 1151, 2048]
    assert H.wave_rows(2049)[7][-1] == 2047 and H.wave_rows(2049)[7][0] == 896
    assert H.probe_rows(5) == [0, 1, 2, 3, 4]                        # waves of one row each
    assert H.probe_rows(37) == [0, 3, 4, 5, 9, 10, 14, 15, 19, 20, 24, 25, 29, 30, 34, 35, 36]
    for b in (0, 3, 4, 127, 128, 511, 512, 1023, 1024, 1151, 1152, 1535, 1536, 2047, 2048):
        assert b in H.probe_rows(2049), b
    # 513 values of JR = 4 rows are 2052 > HT * 4 = 2048: the second staging iteration; 1025 and 2049 rows are two and three rounds
    assert H.STAGE_ROWS == 512 and H.BCH == 1024


SENSITIVE = [c for c in H.CASES if c.C and c.B > 4]


@pytest.mark.parametrize('c', SENSITIVE, ids=H.case_id)
def test_a_lost_batch_row_shows_under_the_bars(c):
    """A weight pass that skipped, doubled or misplaced one batch row -- at a row group, wave, staging or round boundary -- moves each of the four
    gradients by more than 100 times the bar the GPU test holds it to."""
    r = H.reference(c)
    dz2 = H.f64(H.inputs(c)['dz2'])
    worst = {}
    for b in H.probe_rows(c.B):
        for k, lost in (('dW1', np.outer(r['dz1'][b], r['a0'][b])), ('db1', r['dz1'][b]), ('dW2', np.outer(dz2[b], r['a1'][b])), ('db2', dz2[b])):
            e = np.abs(lost).max() / np.abs(r[k]).max()
            worst[k] = min(worst.get(k, np.inf), e)
            assert e > 100 * H.GRAD_RTOL, (k, b, e)
    print('head-ref %s: least relative change of a lost probe row ' % H.case_id(c) + ' '.join('%s %.1e' % kv for kv in worst.items()))


# ----------------------------------------------------------------------------- headroom of the gradient bar
@pytest.mark.parametrize('B', [5, 512, 513, 1025, 2049])
def test_float32_weight_pass_leaves_headroom_under_the_gradient_bar(B):
    """weight_rows' summation order walked in float32 numpy at Hin = H1 = 32, C = 5: within 6e-7 of float64 where the bar is 5e-6, within a quarter
    of the a-priori bound, and a lost boundary row is at least 57 bounds away.  So the bars of the B <= 512 test carry over to B = 2049 (about 8 x
    headroom) and the GPU file introduces no tolerance of its own."""
    c = H.Case('headroom', B, 32, 32, 5, 0.5, True)
    r = H.reference(c)
    dz2 = H.inputs(c)['dz2']
    f32 = lambda a: a.astype(np.float32)
    for name, D, A, ref, refb in (('dW1', f32(r['dz1']), f32(r['a0']), r['dW1'], r['db1']), ('dW2', dz2, f32(r['a1']), r['dW2'], r['db2'])):
        out, bias = H.weight_rows_f32(D, A)
        exact = H.f64(D).T @ H.f64(A)                                # of the float32 operands the walk was given
        bound = H.weight_bound(D, A)
        live = bound > 0                                             # (a small batch leaves elements every row's mask or ReLU zeroes: exact zeros)
        assert live.any() and not out[~live].any()
        err, errb = H.relerr(out.astype(np.float64), exact), H.relerr(bias.astype(np.float64), H.f64(D).sum(0))
        ratio = float((np.abs(out - exact)[live] / bound[live]).max())
        lost = min(float((np.abs(np.outer(H.f64(D[b]), H.f64(A[b])))[live] / bound[live]).max()) for b in H.probe_rows(B))
        print('head-ref headroom B=%d %s: relerr %.2e (bias %.2e), error / bound %.3f, lost row / bound %.0f' % (B, name, err, errb, ratio, lost))
        assert H.relerr(exact, ref) < 1e-6 and H.relerr(H.f64(D).sum(0), refb) < 1e-6      # (the float32 operands are the reference's)
        assert err < 6e-7 and errb < 6e-7
        assert ratio < 0.25
        assert lost > 57
