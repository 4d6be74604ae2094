"""CPU checks of what tests/test_attention512_gpu.py stands on: the geometry of the H = 512 attention instances, its case list, and the bounds it
derives from float32 numpy (tests/attention512_ref.py, tests/attention_ref.py)."""
import numpy as np
import pytest

import attention_ref as A
import attention512_ref as G

pytest.importorskip('torch')
import test_attention512_gpu as T512                 # the table under test lives in the GPU file (importing it needs no device)


def test_geometry_and_cache_border_are_the_launchers_arithmetic():
    assert A.rows_per_pass(G.H) == 0                 # why this width has its own helper
    assert (G.LANES, G.NV, G.R, G.R * A.AU) == (64, 2, 8, 32)
    # fixed + max(T, R) * H * 4 <= LDS_MAX, fixed = (Tp + 32) * 4 forward and (2 * Tp + 32) * 4 backward
    need = lambda T, k: (k * ((T + 3) & ~3) + 32) * 4 + max(T, G.R) * G.H * 4
    last_f = max(T for T in range(1, 200) if need(T, 1) <= A.LDS_MAX); last_b = max(T for T in range(1, 200) if need(T, 2) <= A.LDS_MAX)
    assert (last_f, last_b) == (79, 79)
    assert need(79, 1) == 162240 and need(80, 1) == 164288 and A.LDS_MAX == 163840
    for T in range(1, 200):
        assert G.cached(T) == (need(T, 1) <= A.LDS_MAX, need(T, 2) <= A.LDS_MAX)
    R, RA = G.R, G.R * A.AU
    assert set(G.T_LIST) >= {1, R - 1, R, R + 1, RA - 1, RA, RA + 1, 2 * RA + 3, last_f, last_f + 1, A.AT + 1}
    assert [G.cached(T)[0] for T in G.ZEROS_T] == [True, False] and [G.cached(T)[0] for T in G.EXACT_T] == [True, False]
    assert {G.dense_B(T) for T in G.T_LIST} == {1, 2, 3}


def test_flat_family_is_flat_and_the_gpu_bounds_are_16x_float32_numpy():
    """The largest deviation of attention_from_pre in float32 numpy from float64, both fed the float32 projection, over every flat and zeros case
    of the GPU file.  Another numpy build may sum in another order, hence the quarter of slack against the recorded figures; the GPU bounds are 16 x
    the RECORDED figures, at least 16 / 1.25 x what is measured here and at most the suite's ceiling."""
    worst = dict(ctx=0.0, alpha=0.0, dout=0.0, dpre=0.0)
    for T, B, ragged, scale in G.flat_family():
        c = A.make_case(G.H, T, B, scale, ragged)
        pre = A.pre_f32(c)
        ref = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'])
        assert A.is_flat(ref[1], c['lengths']), (T, B, ragged, ref[1].max())
        if T >= 80 and not ragged:
            assert ref[1].max() < 0.05
        got = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'], dtype=np.float32)
        for k, v in A.deviations(got, ref).items():
            worst[k] = max(worst[k], v)
    print('float32 numpy against float64 over the H = 512 flat family:', ' '.join('%s %.3g' % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= 1.25 * T512.H512_F32[k], (k, v)
        assert v > T512.H512_F32[k] / 4, (k, v, 'the recorded figure is stale')
        assert 16 * v / 1.25 <= T512.H512_BOUNDS[k] <= A.CEILING[k], (k, v)
        assert T512.H512_BOUNDS[k] == min(16 * T512.H512_F32[k], A.CEILING[k])


@pytest.mark.parametrize('scale', ['unit', 'sat'])
def test_unit_and_saturated_cases_are_chosen_by_the_dpre_condition(scale):
    """One float32 rounding of the softmax backward's dot must move dpre by less than 1e-5: (512, 33) qualifies dense and ragged, and float32 numpy
    stays a factor 8 under every ceiling there.  (512, 35) ragged and (512, 80) at the unit scale do not -- the softmax is one-hot, which the exact
    construction covers."""
    for ragged in (False, True):
        c = A.make_case(G.H, G.UNIT_T, A.RAGGED_B if ragged else G.dense_B(G.UNIT_T), scale, ragged)
        pre = A.pre_f32(c)
        ref = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'])
        got = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'], dtype=np.float32)
        for k, v in A.deviations(got, ref).items():
            assert v < A.CEILING[k] / 8, (ragged, k, v)
        cond = A.dpre_condition(c, pre)
        print(scale, 'ragged' if ragged else 'dense', 'dpre_condition %.3g' % cond)
        assert cond < 1e-5, (ragged, cond)
    if scale == 'unit':
        for T, B, ragged in ((35, A.RAGGED_B, True), (80, G.dense_B(80), False)):
            bad = A.make_case(G.H, T, B, 'unit', ragged)
            assert A.dpre_condition(bad, A.pre_f32(bad)) >= 1e-5, (T, ragged)


@pytest.mark.parametrize('T,tstar', [(33, 32), (80, 79)])
def test_one_hot_construction_is_one_hot_in_float32(T, tstar):
    for ragged in (False, True):
        c = A.make_exact_case(G.H, T, A.RAGGED_B if ragged else 2, tstar, ragged)
        pre = A.pre_f32(c)
        assert np.array_equal(pre, np.broadcast_to(c['ba'], pre.shape))
        ctx, alpha, dout, dpre = A.attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'], dtype=np.float32)
        for b in range(c['B']):
            t = int(c['tstar'][b])
            if t < 0:
                assert not ctx[b].any() and not alpha[b].any() and not dout[b].any()
                continue
            want = np.zeros(T, np.float32); want[t] = 1.0
            assert np.array_equal(alpha[b], want)
        assert not dpre[:, c['zero_j']].any()
