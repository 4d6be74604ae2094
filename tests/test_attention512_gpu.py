"""Parity of the H = 512 instances of attention.hip -- attn_{fwd,bwd}2_kernel<128, CACHE, RAG>, 4 + 4 -- at their tile, cache and softmax edges.

The harness is tests/test_attention_forms_gpu.py's, imported: `out` between NaN guard rows, every output between fences of 7.0, every case twice
from fresh buffers bit for bit, the launch-instance log proving which kernels ran, the reference attention_ref.attention_from_pre() in float64 on
the pre-activations the device computed.  Geometry (tests/attention512_ref.py): a wave per row, NV = 2 pieces per lane, R = 8 rows per pass,
R * AU = 32 per loop trip, h_t cached up to T = 79 in both directions.

Cases: T in 1; 7, 8, 9 (R); 31, 32, 33 (R AU); 67 (2 R AU + 3); 79, 80 (the cache border); 513 (a second trip of the t += AT softmax loops), flat,
dense and ragged (B = 4: lengths T, 1, 0 and an interior one); zeros at T = 33 and 80; unit and sat at T = 33 at the suite's ceiling (chosen by
attention_ref.dpre_condition, tests/test_attention512_cpu.py); the one-hot construction at T = 33 and 80.  A misaligned `out` / `dctx` still
falls to the first-generation kernels.

Bounds of the flat and zeros cases: 16 x the largest deviation of float32 numpy from float64 over the same cases (H512_F32 below; the CPU file
measures it again and holds this table to it), under the suite's ceiling.  The figures for ctx and alpha are above attention_ref.FLAT_F32 -- a sum
of 512 products per score where the other widths have at most 256 -- so the width has its own table.

Measured on the MI355X, largest figure over the flat and zeros cases: ctx 3.2e-07, alpha 3.2e-08, dout 2.2e-07, dpre 2.6e-07 -- under float32 numpy's
own; unit and saturated cases (ceiling 1e-4 / 1e-5): ctx <= 2.5e-06, alpha <= 4.5e-07, dout <= 3.8e-06, dpre <= 3.0e-06.
"""
import numpy as np
import pytest

import attention_ref as A
import attention512_ref as G
import test_attention_forms_gpu as F

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

H = G.H
# largest deviation of attention_from_pre(dtype=float32) from float64 over attention512_ref.flat_family()
H512_F32 = dict(ctx=5.2e-7, alpha=8.2e-8, dout=4.2e-7, dpre=6.1e-7)
H512_BOUNDS = {k: min(16 * v, A.CEILING[k]) for k, v in H512_F32.items()}

RAG = pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])


def _forms(T, ragged):
    cf, cb = G.cached(T)
    return F._v2('fwd', H, cf, ragged), F._v2('bwd', H, cb, ragged)


def _keeping_the_other_files_record(fn, *a, **kw):
    """The imported harness notes every instance it judged in its own module's _SEEN / _FIG, which that file's last test compares with ITS list of
    instances: what this file launches is taken out again."""
    seen, fig = set(F._SEEN), {k: dict(v) for k, v in F._FIG.items()}
    try:
        return fn(*a, **kw)
    finally:
        F._SEEN.clear(); F._SEEN.update(seen)
        F._FIG.clear(); F._FIG.update(fig)


def _run(request, c, bounds, label, **kw):
    return _keeping_the_other_files_record(F._run, request, c, bounds, label, **kw)


def _case(T, ragged, scale):
    return A.make_case(H, T, A.RAGGED_B if ragged else G.dense_B(T), scale, ragged)


@RAG
@pytest.mark.parametrize('T', G.T_LIST)
def test_tile_edges_cache_border_and_softmax_stride(request, T, ragged):
    """The instance assertion fails without the H = 512 instances: the log then shows attn_fwd_kernel / attn_bwd_kernel."""
    c = _case(T, ragged, 'flat')
    _run(request, c, H512_BOUNDS, F._label(c), forms=_forms(T, ragged))


@RAG
@pytest.mark.parametrize('scale', ['unit', 'sat'])
def test_unit_and_saturated_scales(request, scale, ragged):
    c = _case(G.UNIT_T, ragged, scale)
    _run(request, c, A.CEILING, F._label(c), forms=_forms(G.UNIT_T, ragged))


@RAG
@pytest.mark.parametrize('T', G.ZEROS_T)
def test_exact_zeros_in_pre_are_masked(request, T, ragged):
    """As tests/test_attention_forms_gpu.py's: pre is 0.0 or -0.0 on a quarter of the features while the sum the mask has to drop is not zero."""
    c = _case(T, ragged, 'zeros')
    z = c['zero_j']
    dev_pre = F._host(F._call(request, c), c)['pre']
    assert not dev_pre[:, z].any(), 'pre is not an exact zero where Wa has a zero row and ba is +-0'
    pre_bits = dev_pre.copy(); pre_bits[:, z] = c['ba'][z]
    assert np.signbit(pre_bits[:, z]).any() and not np.signbit(pre_bits[:, z]).all()
    h, ref = _run(request, c, H512_BOUNDS, F._label(c), pre_bits=pre_bits, forms=_forms(T, ragged))
    live = np.ones(c['B'], bool) if c['lengths'] is None else c['lengths'] > 1
    open_pre = h['pre'].astype(np.float64); open_pre[:, z] = 1e-30
    unmasked = A.attention_from_pre(c['out_in'], open_pre, c['dctx'], c['lengths'])[3]
    assert (np.abs(unmasked[live][:, z]) > 1e-3 * np.abs(ref[3]).max()).mean() > 0.9, 'the mask has nothing to drop in this case'
    assert not F._bits(h['dpre'])[:, z].any() and not F._bits(h['dWa'])[z].any() and not F._bits(h['dba'])[z].any()


@pytest.mark.parametrize('T,tstar', [(33, 0), (33, 31), (33, 32), (80, 0), (80, 79)], ids=['first', 'RAU-1', 'RAU', 're-read first', 're-read last'])
def test_one_hot_softmax_has_exact_outcomes(request, T, tstar):
    assert G.cached(T) == (T == 33, T == 33)
    c = A.make_exact_case(H, T, 1 + tstar % 3, tstar)
    _keeping_the_other_files_record(F._exact, request, c, forms=_forms(T, False))


@pytest.mark.parametrize('T', G.EXACT_T)
def test_one_hot_softmax_has_exact_outcomes_ragged(request, T):
    """t* = len - 1 in every utterance; the empty one gives ctx = 0 bits."""
    c = A.make_exact_case(H, T, A.RAGGED_B, 0, ragged=True)
    _keeping_the_other_files_record(F._exact, request, c, forms=_forms(T, True))


@RAG
@pytest.mark.parametrize('what', ['out', 'dctx'])
def test_alignment_fallback(request, what, ragged):
    """`out` one float into its allocation: both directions run the first-generation kernels.  `dctx` one float in: only the backward does."""
    T = 33
    c = _case(T, ragged, 'flat')
    forms = (F._v1('fwd', ragged) if what == 'out' else F._v2('fwd', H, True, ragged), F._v1('bwd', ragged))
    h, _ = _run(request, c, H512_BOUNDS, F._label(c) + ' %s+4B' % what, off_out=int(what == 'out'), off_dctx=int(what == 'dctx'), forms=forms)
    h2, _ = _run(request, c, H512_BOUNDS, F._label(c) + ' aligned', forms=_forms(T, ragged))
    assert np.array_equal(F._bits(h['pre']), F._bits(h2['pre']))
    if what == 'dctx':
        assert np.array_equal(F._bits(h['ctx']), F._bits(h2['ctx'])) and np.array_equal(F._bits(h['alpha']), F._bits(h2['alpha']))
    w = lambda x: x.astype(np.float64)
    twin = A.deviations(tuple(w(h[k]) for k in ('ctx', 'alpha', 'dout', 'dpre')), tuple(w(h2[k]) for k in ('ctx', 'alpha', 'dout', 'dpre')))
    for k, v in twin.items():
        assert v < H512_BOUNDS[k], (k, v)
