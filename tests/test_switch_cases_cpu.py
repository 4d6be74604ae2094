"""CPU checks of tests/switch_cases.py: the case lists, the row loop against tests/varlen_ref.py, and the quantised-cache helpers that
turn the oracle's backward into the oracle of the 16-bit saved-gate forms (DEP_LSTM_SV16=1; the GRU sweeps' default).

The last test measures how far the quantised backward is from the plain one AT THE SHAPES OF THE GPU CASES: it must be inside the
suite's 1e-4 relerr on its own, or the GPU test's bar against the quantised reference would say nothing about the bar against the
plain one -- and the figure is what a correct 16-bit kernel is expected to show against the plain oracle.  That holds at init-scale gates
only: the tests of the gate regimes below measure, per regime case, what the storage format costs where update gates sit near 1 (it
does not hold 1e-4 there), and pin on the reference alone that the GPU test's bound for those cases is one a correct kernel meets."""
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
    assert [c['name'] for c in S.ENVIRONMENTS['default'][1] if S.writes_pk_image(c)] == \
           [c['name'] for c in S.GRU_FUSED_PK + [r for r in S.GRU_FUSED_REGIMES if r['T'] == 20]]
    for c in S.GRU_LAYER + S.LSTM + S.GRU_LAYER_REGIMES + S.LSTM_REGIMES:
        if c['ragged']:
            n = S.inputs(c)['lengths']
            assert n[0] == c['T'] and n[1] == 1 and n[2] == 0          # a full row, a one-step row, an empty row


def test_regime_cases_are_the_init_draw_moved():
    """Names: an init case keeps its name, another regime appends its own.  Inputs: the seed ignores the regime, so a regime case is
    its init twin with exactly the documented change, float32-rounded again; everything else (dy, dpooled, dh_n, lengths) is the twin's."""
    assert all(c['regime'] == 'init' and not c['name'].endswith('-init') for c in S.GRU_LAYER + S.GRU_LAYER_256 + S.GRU_FUSED + S.GRU_FUSED_PK + S.LSTM)
    assert all(c['regime'] != 'init' and c['name'].endswith('-' + c['regime']) for c in S.REGIME_CASES)
    assert {c['regime'] for c in S.GRU_FUSED_REGIMES} == set(S.REGIMES) - {'init'} and len(S.TRACE_REGIME) == 1
    assert {c['regime'] for c in S.GRU_LAYER_REGIMES + S.LSTM_REGIMES} == {'memory', 'sat'}
    for c in (S.GRU_FUSED_REGIMES[0], S.GRU_LAYER_REGIMES[1], S.LSTM_REGIMES[1], S.LSTM_REGIMES[2]) + \
             tuple(next(r for r in S.GRU_FUSED_REGIMES if r['regime'] == g) for g in ('reset', 'sat', 'drive')):
        H, gru = c['H'], c['cell'] == 'gru'
        a, b = S.inputs(dict(c, regime='init')), S.inputs(c)
        assert a['names'] == b['names'] and all(np.array_equal(a[k], b[k]) for k in a if k not in ('P', 'names', 'prefix', 'x', 'lengths'))
        assert (a['lengths'] is None and b['lengths'] is None) or np.array_equal(a['lengths'], b['lengths'])
        assert np.array_equal(b['x'], S.f32(a['x'] * 10.0) if c['regime'] == 'drive' else a['x'])
        moved = 0
        for n in a['names']:
            pa, pb = a['P'][n], b['P'][n]
            assert np.array_equal(pb, S.f32(pb)), n
            want = pa
            if 'bias_ih' in n and c['regime'] in ('memory', 'reset'):
                want = pa.copy()
                blk = slice(H, 2 * H) if c['regime'] == 'memory' else slice(0, H)      # z of [r | z | n], f of [i | f | g | o]; r
                want[blk] += 4.0 if c['regime'] == 'memory' else -4.0
                moved += 1
            elif 'weight_' in n and c['regime'] == 'sat':
                want = pa * 4.0
                moved += 1
            assert np.array_equal(pb, S.f32(want)), n
        assert moved == {'memory': 2 if gru else 4, 'reset': 2, 'sat': 4 if gru else 8, 'drive': 0}[c['regime']]


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


# ----------------------------------------------------------------------------- the gate regimes: what the storage alone does
F_DELTA_BAR = 2.5e-5        # a quarter of the suite's 1e-4 may go to what float32 gate functions cannot hold; the rest is the kernel's


@pytest.mark.parametrize('c', S.REGIME_CASES, ids=lambda c: c['name'])
def test_what_the_saved_gate_storage_costs_in_each_regime(c):
    """Three figures per regime case, oracle against oracle in float64 (S.storage_figures), each the worst relerr over the tensors
    the case's backward returns:
      E_q  the 16-bit saved gates.  Above 1e-4 wherever update gates sit near 1: dn = dh (1 - z) takes the half-LSB of unorm16
           (7.6e-6 absolute) relative to 1 - z = 0.02.  Pinned for the fused 'memory' cases at F <= 16: the 16-bit format does not hold
           the suite's bar there, and tests/test_switch_forms_gpu.py bounds those forms by RTOL + 2 E_q instead.
      F_d  fp32 gates moved by the fast gate functions' documented error: at most a quarter of the bar, in every regime -- so a
           kernel that saves fp32 gates is held to 1e-4 against the exact oracle everywhere (the regime constants were chosen to keep this).
      sim  moved, then quantised -- a simulated 16-bit device: under 1e-4 + 2 E_q, the GPU bound, on the reference alone.
    Measured: 'memory' E_q 2.0e-4 .. 4.0e-4 (GRU), 2.2e-5 (BiLSTM); 'reset' 5.6e-5 .. 1.9e-4; 'sat' / 'drive' 1.9e-5 .. 7.4e-5;
    F_d <= 9.7e-6; sim / E_q 0.92 .. 1.31."""
    f = S.storage_figures(c, S.inputs(c), _mask(c, 11))
    (eq, nq), (fd, nf), (sim, ns) = f['E_q'], f['F_d'], f['sim']
    short = lambda n: n.rsplit('.', 1)[-1]
    print('gate-regimes %s: E_q %.3e (%s)  F_d %.3e (%s)  simulated 16-bit device %.3e (%s) = %.2f E_q'
          % (c['name'], eq, short(nq), fd, short(nf), sim, short(ns), sim / eq))
    assert 0.0 < fd <= F_DELTA_BAR, (nf, fd)
    assert 0.0 < sim < 1e-4 + 2 * eq, (ns, sim, eq)
    if c in S.GRU_FUSED_REGIMES and c['regime'] == 'memory' and c['F'] <= 16:
        assert eq > 1e-4, (nq, eq)


def test_the_left_out_case_misses_the_forward_bar_by_the_split_products_alone():
    """switch_cases.LEFT_OUT: 'sat' at 37 x 20 x 256 with dropout.  A float64 forward whose products alone are the split-precision ones
    (16 mantissa bits per operand, three of the four partial products) is already past 1e-4 absolute on y there -- 1.07e-4; the device
    shows 1.086e-4 -- so no gate phase can bring the case inside the bar, and the case stays out until the products carry more bits.
    Its twin without dropout is inside (9.3e-5 here, 9.46e-5 on the device) and stays in the lists; at init scale the same products
    cost 4.4e-6."""
    (c,) = S.LEFT_OUT
    assert c['name'] not in {k['name'] for cases in S.ENVIRONMENTS.values() for k in cases[1]}
    figs = {}
    for k in (c, dict(c, p=0.0), dict(c, regime='init')):
        inp, mask = S.inputs(k), _mask(k, 11)
        y, _ = R.gru_stack_fwd(inp['x'], inp['P'], inp['prefix'], S.LAYERS, None if mask is None else [mask])
        figs[(k['regime'], k['p'])] = np.abs(S.split_products_forward(k, inp, mask) - y).max()
    print('split products alone, worst abs on y: ' + ', '.join('%s p=%g %.3e' % (r, p, e) for (r, p), e in figs.items()))
    assert figs[('sat', 0.5)] > 1e-4 > figs[('sat', 0.0)] > 5e-5
    assert figs[('init', 0.5)] < 1e-5
