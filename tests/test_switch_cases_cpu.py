"""CPU checks of tests/switch_cases.py: the case lists, the row loop against tests/varlen_ref.py, and the quantised-cache helpers that
turn the oracle's backward into the oracle of the 16-bit saved-gate forms (DEP_LSTM_SV16=1; the GRU sweeps' default).

The last test measures how far the quantised backward is from the plain one AT THE SHAPES OF THE GPU CASES: it must be inside the
suite's 1e-4 relerr on its own, or the GPU test's bar against the quantised reference would say nothing about the bar against the
plain one -- and the figure is what a correct 16-bit kernel is expected to show against the plain oracle."""
import numpy as np
import pytest

import switch_cases as S
from oracle import ref_numpy as R


def _mask(c, seed):
    if c['p'] == 0:
        return None
    dirs = 1 if c['cell'] == 'gru' else 2
    keep = np.random.default_rng(seed).random((c['B'], c['T'], c['H'] * dirs)) >= c['p']
    return keep / (1.0 - c['p'])


def test_case_lists_are_consistent():
    names = set()
    for tag, (env, cases) in S.ENVIRONMENTS.items():
        assert set(env) <= set(S.SWITCHES), tag
        assert len({c['name'] for c in cases}) == len(cases), tag
        names |= {c['name'] for c in cases}
        for c in cases:
            assert c['B'] <= 37 and (c['T'] <= 7 or (c['T'] == 20 and S.writes_pk_image(c)))      # no full-size shapes
    base = {c['name'] for c in S.ENVIRONMENTS['default'][1]}
    for tag in ('sv16_off', 'lstm_sv16', 'trace', 'trace_sv16_off'):
        assert {c['name'] for c in S.ENVIRONMENTS[tag][1]} <= base, tag    # every switched case has its baseline
    assert [c['name'] for c in S.ENVIRONMENTS['default'][1] if S.writes_pk_image(c)] == [c['name'] for c in S.GRU_FUSED_PK]
    for c in S.GRU_LAYER + S.LSTM:
        if c['ragged']:
            n = S.inputs(c)['lengths']
            assert n[0] == c['T'] and n[1] == 1 and n[2] == 0          # a full row, a one-step row, an empty row


def test_inputs_are_deterministic_and_float32_rounded():
    c = S.LSTM[3]
    a, b = S.inputs(c), S.inputs(dict(c))
    for k in ('x', 'dy', 'dh_n'):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], S.f32(a[k]))
    assert all(np.array_equal(a['P'][n], b['P'][n]) for n in a['names'])


@pytest.mark.parametrize('c', [S.GRU_LAYER[1], S.GRU_FUSED[2], S.LSTM[3], S.LSTM[5]], ids=lambda c: c['name'])
def test_the_row_loop_is_the_ragged_oracle(c):
    """reference() with nothing quantised: the dense call is the oracle's, the ragged one tests/varlen_ref.py's; the loop that the
    quantised reference takes gives the same numbers (identity in place of the quantiser)."""
    inp = S.inputs(c)
    mask = _mask(c, 3)
    plain = S.reference(c, inp, mask)
    q = S.quantise_gru_caches, S.quantise_lstm_caches
    try:
        S.quantise_gru_caches = S.quantise_lstm_caches = lambda caches: caches
        loop = S.reference(c, inp, mask, quantised=True)
    finally:
        S.quantise_gru_caches, S.quantise_lstm_caches = q
    for k in ('y', 'h_n', 'dx') + (('pooled',) if c['cell'] == 'gru' else ()):
        assert np.abs(plain[k] - loop[k]).max() < 1e-13, k
    for n in inp['names']:
        assert np.abs(plain['G'][n] - loop['G'][n]).max() < 1e-12, n


def test_quantising_moves_every_gate_by_at_most_half_an_lsb():
    c = S.LSTM[0]
    inp = S.inputs(c)
    _, _, caches = R.bilstm_stack_fwd(inp['x'], inp['P'], inp['prefix'], S.LAYERS)
    H = c['H']
    for (x, ys, cs, g, rev), (xq, ysq, csq, gq, revq) in zip(caches, S.quantise_lstm_caches(caches)):
        assert xq is x and ysq is ys and csq is cs and revq == rev     # only the gates are stored in 16 bits
        assert gq is not g and (gq != g).any()
        tanh_gate = np.zeros(g.shape[-1], bool); tanh_gate[2 * H:3 * H] = True
        assert np.abs(gq - g)[..., ~tanh_gate].max() <= 0.5 / 65535 + 1e-16
        assert np.abs(gq - g)[..., tanh_gate].max() <= 0.5 / 32767 + 1e-16
        assert np.abs(gq - g)[..., tanh_gate].max() > 0.5 / 65535      # ... and g really has the coarser format
        assert np.array_equal(gq[..., ~tanh_gate] * 65535, np.round(gq[..., ~tanh_gate] * 65535))
    c = S.GRU_LAYER[0]
    inp = S.inputs(c)
    _, caches = R.gru_stack_fwd(inp['x'], inp['P'], inp['prefix'], S.LAYERS)
    for (x, ys, r, z, n, hn), (xq, ysq, rq, zq, nq, hnq) in zip(caches, S.quantise_gru_caches(caches)):
        assert xq is x and ysq is ys and hnq is hn
        assert (rq != r).any() and (zq != z).any() and (nq != n).any()
        assert max(np.abs(rq - r).max(), np.abs(zq - z).max()) <= 0.5 / 65535 + 1e-16
        assert 0.5 / 65535 < np.abs(nq - n).max() <= 0.5 / 32767 + 1e-16


QUANT_CASES = S.LSTM + S.GRU_LAYER + S.GRU_FUSED + S.GRU_FUSED_PK


def test_the_quantised_backward_stays_inside_the_suites_bar_at_the_gpu_shapes():
    """Worst relerr of any tensor of the quantised backward against the plain one, over every BiLSTM case of DEP_LSTM_SV16=1 and every
    GRU case (masks of the case's p from numpy's generator here: any mask serves).  Measured: BiLSTM 2.5e-5, GRU 2.1e-5."""
    worst = {'lstm': 0.0, 'gru': 0.0}
    for c in QUANT_CASES:
        inp = S.inputs(c)
        mask = _mask(c, 11)
        a, b = S.reference(c, inp, mask), S.reference(c, inp, mask, quantised=True)
        for k in ('y', 'h_n'):
            assert np.abs(a[k] - b[k]).max() < 1e-13, (c['name'], k)    # the forward does not read the saved gates
        for n in list(inp['names']) + ['dx']:
            ta, tb = (a['dx'], b['dx']) if n == 'dx' else (a['G'][n], b['G'][n])
            e = S.relerr(tb, ta)
            assert 0.0 < e < 1e-4, (c['name'], n, e)
            worst[c['cell']] = max(worst[c['cell']], e)
    print('quantised vs plain oracle backward, worst relerr: BiLSTM %.2e, GRU %.2e' % (worst['lstm'], worst['gru']))
