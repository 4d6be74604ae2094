"""CPU checks of what tests/test_attention_forms_gpu.py stands on: the reference it compares with, the case lists, and the bounds it derives from
float32 numpy (tests/attention_ref.py)."""
import numpy as np
import pytest

import attention_ref as A
from oracle import ref_numpy as R
from varlen_ref import attention_ragged


def _f64(c, *names):
    return [c[n].astype(np.float64) for n in names]


@pytest.mark.parametrize('H,T,B,scale', [(128, 67, 3, 'unit'), (64, 33, 2, 'flat'), (256, 35, 1, 'sat'), (8, 5, 3, 'zeros'), (1, 4, 2, 'flat')])
def test_helper_reproduces_the_oracle_when_fed_the_oracles_pre(H, T, B, scale):
    c = A.make_case(H, T, B, scale)
    out, hn, Wa, ba, dctx = _f64(c, 'out', 'hn', 'Wa', 'ba', 'dctx')
    ctxr, cache = R.attention_fwd(out, hn, Wa, ba)
    doutr, dhnr, dWar, dbar = R.attention_bwd(dctx, Wa, cache)
    ctx, alpha, dout, dpre = A.attention_from_pre(out, cache[2], dctx)
    assert np.abs(ctx - ctxr).max() < 1e-12 and np.abs(alpha - cache[5]).max() < 1e-12 and np.abs(dout - doutr).max() < 1e-12
    assert np.abs(dpre.T @ cache[1] - dWar).max() < 1e-12 and np.abs(dpre.sum(0) - dbar).max() < 1e-12 and np.abs(dpre @ Wa - dhnr[0]).max() < 1e-12


@pytest.mark.parametrize('H,T,scale', [(128, 67, 'unit'), (64, 131, 'flat'), (16, 9, 'zeros')])
def test_helper_reproduces_the_ragged_row_loop(H, T, scale):
    c = A.make_case(H, T, A.RAGGED_B, scale, ragged=True)
    out, hn, Wa, ba, dctx = _f64(c, 'out', 'hn', 'Wa', 'ba', 'dctx')
    n = c['lengths']
    assert n[0] == T and n[1] == 1 and n[2] == 0
    ref = attention_ragged(out, n, hn, Wa, ba, dctx)
    pre = hn.sum(0) @ Wa.T + ba
    ctx, alpha, dout, dpre = A.attention_from_pre(c['out_in'].astype(np.float64), pre, dctx, n)       # NaN behind the lengths: never read
    assert np.abs(ctx - ref['ctx']).max() < 1e-12 and np.abs(alpha - ref['alpha']).max() < 1e-12 and np.abs(dout - ref['dout']).max() < 1e-12
    live = n > 0                                                     # (the row loop skips an empty row: it adds nothing to the weight gradients)
    assert not dpre[~live].any()
    assert np.abs(dpre.T @ hn.sum(0) - ref['dWa']).max() < 1e-12 and np.abs(dpre.sum(0) - ref['dba']).max() < 1e-12
    assert np.abs((dpre @ Wa)[live] - ref['dhn'][0][live]).max() < 1e-12


def test_cache_border_table_is_the_launchers_arithmetic():
    for H, T, cf, cb in A.CACHE_BORDER + A.SOFTMAX_STRIDE:
        assert A.cached(H, T) == (cf, cb), (H, T)
    for H in (64, 128, 256):
        assert all(A.cached(H, T) == (True, True) for T in A.tile_edges(H))
        both, mixed, none = A.FORM_T[H]
        assert A.cached(H, both) == (True, True) and A.cached(H, mixed) == (True, False) and A.cached(H, none) == (False, False)
        last_f = max(T for T in range(1, 700) if A.cached(H, T)[0]); last_b = max(T for T in range(1, 700) if A.cached(H, T)[1])
        assert (last_f, last_b) == {64: (629, 620), 128: (317, 314), 256: (159, 158)}[H]
    assert [A.rows_per_pass(H) for H in (64, 128, 256)] == [32, 16, 8]
    assert {A.dense_B(H, T) for H, T, _, r, _ in A.flat_family() if not r} == {1, 2, 3}
    for H in (64, 128, 256):
        assert any(B == 1 for h, T, B, r, _ in A.flat_family() if h == H and not r)


def test_flat_family_is_flat_and_float32_numpy_stays_inside_the_recorded_figures():
    """The figures the GPU file's flat bounds are 16 x of: the largest deviation of attention_from_pre in float32 numpy from float64, both fed the
    float32 projection, over every flat case.  attention_ref.FLAT_F32 records them; another numpy build may sum in another order, hence the quarter
    of slack here -- the GPU bounds are 16 x the RECORDED figures and do not move with this measurement."""
    worst = dict(ctx=0.0, alpha=0.0, dout=0.0, dpre=0.0)
    for H, T, B, ragged, scale in A.flat_family():
        c = A.make_case(H, T, B, scale, ragged)
        pre = A.pre_f32(c)
        ref = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'])
        assert A.is_flat(ref[1], c['lengths']), (H, T, B, ragged, ref[1].max())
        if T >= 80 and not ragged:
            assert ref[1].max() < 0.05
        got = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'], dtype=np.float32)
        for k, v in A.deviations(got, ref).items():
            worst[k] = max(worst[k], v)
    print('float32 numpy against float64 over the flat family:', ' '.join('%s %.3g' % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= 1.25 * A.FLAT_F32[k], (k, v)
        assert v > A.FLAT_F32[k] / 4, (k, v, 'the recorded figure is stale')


@pytest.mark.parametrize('scale', ['unit', 'sat'])
def test_unit_and_saturated_cases_leave_float32_room_under_the_ceiling(scale):
    """These two scales are held to the suite's older bounds only.  At the unit scale the softmax is nearly one-hot and dpre a difference of nearly
    equal sums, so the cases are chosen where float32 numpy itself stays a factor 8 under every bound AND one float32 rounding of the softmax
    backward's dot moves dpre by less than a sixteenth of its bound (attention_ref.dpre_condition): a kernel is then not failed for the conditioning
    of its inputs.  (2, 35, 256) at the unit scale is the counter-example: alpha.max() = 0.999, one rounding moves dpre by 0.9e-4; float32 numpy
    happens to land 6e-6 from float64 there and the MI355X 1.6e-4.)"""
    for H in (64, 128, 256):
        for T in A.FORM_T[H]:
            for ragged in (False, True):
                c = A.make_case(H, T, A.RAGGED_B if ragged else A.dense_B(H, T), scale, ragged)
                pre = A.pre_f32(c)
                ref = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'])
                got = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'], dtype=np.float32)
                for k, v in A.deviations(got, ref).items():
                    assert v < A.CEILING[k] / 8, (H, T, ragged, k, v)
                assert A.dpre_condition(c, pre) < A.CEILING['dpre'] / 16, (H, T, ragged)
    bad = A.make_case(256, 35, 1, 'unit')
    assert A.dpre_condition(bad, A.pre_f32(bad)) > A.CEILING['dpre'] / 2


@pytest.mark.parametrize('H,T,tstar', [(64, 130, 127), (128, 318, 0), (256, 34, 33), (128, 66, 64)])
def test_one_hot_construction_is_one_hot_in_float32(H, T, tstar):
    for ragged in (False, True):
        c = A.make_exact_case(H, T, A.RAGGED_B if ragged else 2, tstar, ragged)
        pre = A.pre_f32(c)
        assert np.array_equal(pre, np.broadcast_to(c['ba'], pre.shape))                  # Wa = 0: pre = ba
        assert (c['ba'] == 100.0).sum() == 4 and (c['ba'] == 0.0).sum() > H // 2 and np.signbit(c['ba'][c['ba'] == 0.0]).any() and (c['ba'] < 0).any()
        ctx, alpha, dout, dpre = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'], dtype=np.float32)
        h = c['out'][..., :H] + c['out'][..., H:]
        for b in range(c['B']):
            t = int(c['tstar'][b])
            if t < 0:
                assert not ctx[b].any() and not alpha[b].any() and not dout[b].any()
                continue
            want = np.zeros(T, np.float32); want[t] = 1.0
            assert np.array_equal(alpha[b], want)
            assert np.array_equal(ctx[b], h[b, t])
            assert np.array_equal(dout[b, t], np.concatenate([c['dctx'][b], c['dctx'][b]]))
            assert not np.delete(dout[b], t, axis=0).any()
        assert not dpre[:, c['zero_j']].any()
