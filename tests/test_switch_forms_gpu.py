"""Sweep parity of the instances that only an environment switch selects.

The instance tables of the cluster families (csrc/rnn_cluster_bwd.hip, rnn_cluster_lstm.hip, rnn_fused2.hip, rnn_fused2_bwd.hip) hold
rows that DEP_SV16=0, DEP_LSTM_SV16=1, DEP_TRACE=1 or dep_set_gemm_mode(3) select.  The switches are read once per process, so
tests/switch_probe.py runs the case lists of tests/switch_cases.py in ONE child process per environment, once per session; the tests
below read that cache, compare with the float64 oracle built from the same seeded inputs, and add the instances the children launched
to the session's record (tests/test_zz_instance_tables_gpu.py closes the tables over it).

  default         the baseline of every bit-identity below, itself held to the oracle -- and, for the GRU cases (16-bit saved gates are
                  their default), to the oracle backward fed the quantised gates as a second reference
  DEP_SV16=0      fp32 saved GRU gates: oracle parity at the suite's bars, forward bit-identical to the default
  DEP_LSTM_SV16=1 16-bit saved BiLSTM gates: the reference is the oracle backward fed the quantised gates (tests/switch_cases.py,
                  pinned on the CPU by tests/test_switch_cases_cpu.py), bar 1e-4 relerr; forward bit-identical to the default
                  (lstm_fwd_cluster reads SV16 in the service waves' write-out alone: the width of the saved-gate rows and the packing
                  of what the compute waves left in LDS)
  DEP_TRACE=1     (and DEP_TRACE=1 DEP_SV16=0: the stamped fused forward has a row per saved-gate format) every output and gradient
                  bit-identical to the unstamped run; the trace tools (tools/trace_*.py) make a plain call, so nothing else is set up
  DEP_FUSED2_BWD=0, modes 2 / 3: the per-layer bf16-storage backward against the fp32-storage one, bars of
                  test_bf16_storage_mode_has_its_own_tolerance; the fused bf16-storage forms run in-process (the mode is no switch)

Shapes: at most 37 utterances x 7 steps, except where a row needs the PK image of the gate gradients (the stamped fused backward, every
bf16-storage form, gru2_bwd_fused<.., true, true>): the smallest stack that writes it is 37 x 20 with F = 256 (switch_cases.GRU_FUSED_PK).

Every child runs under a time limit; a child that does not exit 0 fails every test of its environment and is not started again, and
after a child that died on a signal or ran into its limit no further child is started in the session.

Figures of the last device run (one MI355X), worst relerr of any gradient or dx over an environment's cases (this module prints the
figure of every case in lines `switch-forms ...`); "quantised" = against the oracle backward fed the 16-bit gates:
  DEP_LSTM_SV16=1   BiLSTM                 plain oracle 2.97e-5 (bias_ih_l0, T = 7 dense)   quantised 9.05e-6   <- the asserted one
  default           BiLSTM (fp32 gates)    plain oracle 5.90e-6
  default           GRU per-layer sweeps   plain oracle 1.77e-5 (dx, H = 512 ragged)        quantised 8.18e-6
  default           GRU fused stack        plain oracle 1.90e-5 (dx, 33 x 4, dropout)       quantised 1.33e-5
  DEP_SV16=0        GRU per-layer sweeps   plain oracle 7.52e-6
  DEP_SV16=0        GRU fused stack        plain oracle 6.63e-6
  (the quantisation alone, oracle against oracle on the CPU: BiLSTM 2.5e-5, GRU 2.1e-5 -- tests/test_switch_cases_cpu.py)
  mode 3 against mode 2: a gradient moves by at most 1.2e-3 of its scale in the fused forms, 1.7e-3 on the per-layer backward (bar 1e-2)
Outside init-scale gates (the regimes of tests/switch_cases.py; same run; worst relerr of any gradient or dx over the regime's cases; E_q = what
the 16-bit storage alone does to a case, oracle against oracle; the 16-bit forms are held to RTOL + 2 E_q of the case, the fp32-gate forms to RTOL):
  regime    16-bit GRU gates (default): plain oracle | quantised | E_q             fp32 GRU gates (DEP_SV16=0)
  memory    1.72e-4 .. 3.95e-4 | 6.31e-5 .. 2.26e-4 | 1.74e-4 .. 3.95e-4            3.79e-6 .. 7.72e-6
  reset     6.44e-5 .. 1.86e-4 | 3.58e-5 .. 1.31e-4 | 6.40e-5 .. 1.93e-4            5.85e-6 .. 1.14e-5
  sat       2.16e-5 .. 6.27e-5 | 1.50e-5 .. 5.37e-5 | 1.93e-5 .. 5.15e-5            6.92e-6 .. 3.00e-5
  drive     2.11e-5 .. 6.43e-5 | 1.46e-5 .. 4.72e-5 | 1.99e-5 .. 4.47e-5            5.18e-6 .. 3.88e-5
  BiLSTM    DEP_LSTM_SV16=1: memory 2.09e-5 | 8.55e-6 | 1.98e-5, sat 2.74e-5 | 2.43e-5 | 2.87e-5;   default (fp32 gates): memory 3.43e-6, sat 1.19e-5
  outputs   worst abs on y / h_n / pooled: memory 1.0e-6, reset 7.2e-6, drive 8.0e-5 (h_n of layer 0 at 37 x 20), sat 2.5e-5 at T <= 7 and
            9.46e-5 at 37 x 20 x 256 without dropout -- with dropout 1.086e-4, past ATOL: the one case left out (switch_cases.LEFT_OUT; the
            split-precision products' operand format, not the gate phase: tests/test_switch_cases_cpu.py)
Wall time of a child, 8 to 85 cases: 2.2 to 2.9 s.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import switch_cases as S

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]
HERE = os.path.dirname(os.path.abspath(__file__))

ATOL = 1e-4         # the suite's bars (tests/test_kernels_gpu.py): absolute on outputs, relerr per gradient tensor
RTOL = 1e-4

_RUNS = {}          # environment tag -> {'cases': {name: {array name: array}}, 'wall': seconds} | {'error': text}
_STOP = []          # set once a child died on a signal or ran into its time limit
_REFS = {}          # (case name, quantised) -> reference


@pytest.fixture(scope='session')
def switch_dir(tmp_path_factory):
    return tmp_path_factory.mktemp('switch_forms')


def run_environment(tag, out_dir):
    """The child of one environment: started at most once per session."""
    if tag in _RUNS:
        return _RUNS[tag]
    if _STOP:
        _RUNS[tag] = {'error': 'not started: ' + _STOP[0]}
        return _RUNS[tag]
    env_vars, cases = S.ENVIRONMENTS[tag]
    jobs = [[str(out_dir / f'{tag}_{i}.npz'), c] for i, c in enumerate(cases)]
    spec = str(out_dir / f'{tag}.json')
    with open(spec, 'w') as f:
        json.dump(jobs, f)
    env = {k: v for k, v in os.environ.items() if k not in S.SWITCHES}
    env.update(env_vars)
    limit = 120 + 5 * len(cases)                    # start-up (imports, code objects) + a few tenths of a second per case, with room
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, 'switch_probe.py'), '--batch', spec], env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        _STOP.append(f'the child of environment {tag!r} ran into its time limit of {limit} s')
        _RUNS[tag] = {'error': _STOP[0] + '\n' + str(e.stdout or '')[-2000:] + str(e.stderr or '')[-3000:]}
        return _RUNS[tag]
    wall = time.time() - t0
    if r.returncode != 0:
        msg = f'the child of environment {tag!r} exited with {r.returncode}'
        if r.returncode < 0 or r.returncode in (134, 137, 139):
            _STOP.append(msg)
        _RUNS[tag] = {'error': msg + '\n' + r.stdout[-2000:] + r.stderr[-3000:]}
        return _RUNS[tag]
    print(f'switch-forms child {tag} ({" ".join(k + "=" + v for k, v in env_vars.items()) or "no switch"}): {len(cases)} cases, {wall:.1f} s')
    _RUNS[tag] = {'cases': {c['name']: dict(np.load(out)) for out, c in jobs}, 'wall': wall}
    return _RUNS[tag]


def results(tag, out_dir):
    run = run_environment(tag, out_dir)
    assert 'error' not in run, run['error']
    return run['cases']


def instances(res):
    return set(str(s) for s in res['instances'])


def record(request, *runs):
    """What the children launched for the cases this test compared -> the session's record of oracle-tested instances."""
    rec = request.config._dep_instances.setdefault(request.node.nodeid, set())
    for res in runs:
        rec.update(instances(res))


def reference(c, mask, quantised=False):
    key = (c['name'], quantised)
    if key not in _REFS:
        _REFS[key] = S.reference(c, S.inputs(c), mask, quantised)
    return _REFS[key]


def f64(a):
    return np.asarray(a).astype(np.float64)


def check_outputs(c, res, ref, tag=''):
    if c['regime'] != 'init':                       # (printed before any assertion, like the gradients' figures)
        print(f'switch-forms {tag} {c["name"]}: outputs, worst abs vs the oracle: ' +
              ', '.join('%s %.3e' % (k, np.abs(f64(res[k]) - ref[k]).max()) for k in ('y', 'h_n', 'pooled') if k in res))
    assert np.abs(f64(res['y']) - ref['y']).max() < ATOL, 'y'
    assert np.abs(f64(res['h_n']) - ref['h_n']).max() < ATOL, 'h_n'
    if c['cell'] == 'gru':
        assert np.abs(f64(res['pooled']) - ref['pooled']).max() < ATOL, 'pooled'
    if c['ragged']:
        pad = np.arange(c['T'])[None, :] >= S.inputs(c)['lengths'][:, None]
        assert not res['y'].view(np.int32)[pad].any(), 'y is not exactly 0.0 at padded positions'
        if c['dx']:
            assert not res['dx'].view(np.int32)[pad].any(), 'dx is not exactly 0.0 at padded positions'


def gradient_errors(c, res, ref):
    """[(tensor name, relerr)] of every weight gradient, and of dx where the case has one."""
    names = S.inputs(c)['names']
    out = [(n, S.relerr(f64(res['g%d' % i]), ref['G'][n])) for i, n in enumerate(names)]
    for i, n in enumerate(names):
        assert np.isfinite(res['g%d' % i]).all(), n
    if c['dx']:
        out.append(('dx', S.relerr(f64(res['dx']), ref['dx'])))
    return out


def report(tag, c, plain, quant=None):
    wp = max(plain, key=lambda v: v[1])
    line = f'switch-forms {tag} {c["name"]}: worst relerr vs the oracle {wp[1]:.3e} ({wp[0]})'
    if quant is not None:
        wq = max(quant, key=lambda v: v[1])
        line += f', vs the oracle fed the 16-bit gates {wq[1]:.3e} ({wq[0]})'
    print(line)


def forward_is_bit_identical(a, b):
    for k in ('y', 'pooled', 'h_n'):
        if k in a or k in b:
            assert np.array_equal(a[k], b[k]), (k, float(np.abs(f64(a[k]) - f64(b[k])).max()))


ident = lambda c: c['name']
TF = {True: 'true', False: 'false'}


# ----------------------------------------------------------------------------- the switch took effect
def switched_rows(tag, c):
    """The table rows environment `tag` exists for, as case c must launch them (and as the default environment must not)."""
    D, Y = TF[c['p'] > 0], TF[c['form'] == 'full']
    fused = c['cell'] == 'gru' and c['H'] == 256 and c['impl'] == 3 and not c['ragged']
    if tag == 'sv16_off':
        if fused:
            return {'gru2_fwd_fused<%s, false, false>' % D, 'gru2_bwd_fused<%s, %s, false, false>' % (D, Y)}
        dense = {64: 'gru_bwd_cluster_r1<1, true, 4, false>', 128: 'gru_bwd_cluster_r1<2, true, 4, false>',
                 256: 'gru_bwd_cluster_r1<4, true, 4, false, false, true>', 512: 'gru_bwd_cluster_r1<8, true, 0>'}
        ragged = {64: 'gru_bwd_cluster_r1<1, true, 4, false, false, false, true>', 128: 'gru_bwd_cluster_r1<2, true, 4, false, false, false, true>',
                  256: 'gru_bwd_cluster_r1<4, true, 4, false, false, true, true>', 512: 'gru_bwd_cluster_r1<8, true, 0, false, false, false, true>'}
        return {(ragged if c['ragged'] else dense)[c['H']]}
    if tag == 'lstm_sv16':
        return {'lstm_fwd_cluster<true, true, true>', 'lstm_bwd_cluster<true, true, true>'} if c['ragged'] else \
               {'lstm_fwd_cluster<true, true>', 'lstm_bwd_cluster<true, true>'}
    if tag == 'trace':
        if not fused:
            return set()                            # the per-layer and BiLSTM sweeps stamp through a run-time pointer: no row of their own
        rows = {'gru2_fwd_fused<%s, true, true>' % D}
        if c['form'] == 'model' and S.writes_pk_image(c):               # the stamped backward is the model form's, PK image
            rows.add('gru2_bwd_fused<%s, false, true, true, true>' % D)
        return rows
    if tag == 'trace_sv16_off':
        return {'gru2_fwd_fused<%s, true, false>' % D}
    assert tag == 'layer_bwd'
    return {'gru2_fwd_fused<%s, false, true, true>' % D, 'gru_bwd_cluster_r1<4, true, 4, true, true, true>'} if c['mode'] == 3 else set()


# every switch-selected row by name: the union of switched_rows over an environment's cases must be exactly this
ROWS = {
    'sv16_off': {'gru_bwd_cluster_r1<1, true, 4, false>', 'gru_bwd_cluster_r1<2, true, 4, false>', 'gru_bwd_cluster_r1<8, true, 0>',
                 'gru_bwd_cluster_r1<1, true, 4, false, false, false, true>', 'gru_bwd_cluster_r1<2, true, 4, false, false, false, true>',
                 'gru_bwd_cluster_r1<8, true, 0, false, false, false, true>',
                 'gru_bwd_cluster_r1<4, true, 4, false, false, true>', 'gru_bwd_cluster_r1<4, true, 4, false, false, true, true>',
                 'gru2_fwd_fused<true, false, false>', 'gru2_fwd_fused<false, false, false>',
                 'gru2_bwd_fused<true, true, false, false>', 'gru2_bwd_fused<true, false, false, false>',
                 'gru2_bwd_fused<false, true, false, false>', 'gru2_bwd_fused<false, false, false, false>'},
    'lstm_sv16': {'lstm_fwd_cluster<true, true>', 'lstm_bwd_cluster<true, true>', 'lstm_fwd_cluster<true, true, true>', 'lstm_bwd_cluster<true, true, true>'},
    'trace': {'gru2_fwd_fused<true, true, true>', 'gru2_fwd_fused<false, true, true>',
              'gru2_bwd_fused<true, false, true, true, true>', 'gru2_bwd_fused<false, false, true, true, true>'},
    'trace_sv16_off': {'gru2_fwd_fused<true, true, false>', 'gru2_fwd_fused<false, true, false>'},
    'layer_bwd': {'gru_bwd_cluster_r1<4, true, 4, true, true, true>', 'gru2_fwd_fused<true, false, true, true>', 'gru2_fwd_fused<false, false, true, true>'},
}


@pytest.mark.parametrize('tag', list(ROWS))
def test_the_switch_selected_its_rows(tag, switch_dir):
    """Case by case: the environment's launch log holds the rows it exists for and the default environment's log for the same case
    holds none of them.  Good numbers from a case whose switch changed nothing would prove nothing about those rows."""
    cases = S.ENVIRONMENTS[tag][1]
    got = results(tag, switch_dir)
    base = results('default', switch_dir) if tag != 'layer_bwd' else {}
    seen = set()
    for c in cases:
        want = {'(%s)' % r for r in switched_rows(tag, c)}
        inst = instances(got[c['name']])
        assert want <= inst, (c['name'], sorted(want - inst), sorted(inst))
        seen |= want
        if c['name'] in base:
            both = instances(base[c['name']]) & {'(%s)' % r for r in ROWS[tag]}
            assert not both, (c['name'], sorted(both))
        if tag == 'layer_bwd':                      # the fused backward is switched off, and only mode 3 stores bf16
            assert not any('gru2_bwd_fused' in s for s in inst), (c['name'], sorted(inst))
            if c['mode'] == 2:
                assert not inst & {'(%s)' % r for r in ROWS[tag]}, (c['name'], sorted(inst))
    assert seen == {'(%s)' % r for r in ROWS[tag]}, sorted(seen ^ {'(%s)' % r for r in ROWS[tag]})


# ----------------------------------------------------------------------------- the default environment: both references
def storage_error(c, mask):
    """E_q of a regime case (tests/test_switch_cases_cpu.py): what the 16-bit saved gates alone do to its backward, the oracle fed the
    quantised gates against the exact oracle, worst relerr over the tensors the case returns.  From the oracle, never from the device."""
    return S.worst_relerr(c, S.inputs(c), reference(c, mask, quantised=True), reference(c, mask))[0]


def check_16bit_regime(tag, c, res, mask):
    """A regime case on a 16-bit saved-gate form: every gradient and dx against the EXACT oracle under RTOL + 2 E_q(case).  E_q is the
    storage format's own error at this case; the factor 2 covers a rounding pattern that differs from the oracle's (the device's gates
    differ from the oracle's by up to 4e-7, which moves about 3 % of the codes) -- the CPU test holds a simulated device to the same bound."""
    plain = gradient_errors(c, res, reference(c, mask))
    report(tag, c, plain, gradient_errors(c, res, reference(c, mask, quantised=True)))
    e_q = storage_error(c, mask)
    print(f'switch-forms {tag} {c["name"]}: E_q {e_q:.3e}, bound {RTOL + 2 * e_q:.3e}')
    for n, e in plain:
        assert e < RTOL + 2 * e_q, (n, e, e_q)


@pytest.mark.parametrize('c', S.ENVIRONMENTS['default'][1], ids=ident)
def test_default_forms_against_the_oracle(c, switch_dir, request):
    """The baseline of the bit-identities below is itself right.  The GRU cases run with 16-bit saved gates by default: they are also
    held to the oracle backward fed the quantised gates, the reference of the operation they compute (same bar).  Outside the init
    regime the 16-bit GRU forms are held to the exact oracle under RTOL + 2 E_q (check_16bit_regime); the BiLSTM saves fp32 gates by
    default and keeps RTOL against the exact oracle in every regime."""
    res = results('default', switch_dir)[c['name']]
    mask = f64(res['mask']) if c['p'] > 0 else None
    ref = reference(c, mask)
    check_outputs(c, res, ref, 'default')
    if c['regime'] != 'init' and c['cell'] == 'gru':
        check_16bit_regime('default', c, res, mask)
    else:
        plain = gradient_errors(c, res, ref)
        quant = gradient_errors(c, res, reference(c, mask, quantised=True)) if c['cell'] == 'gru' else None
        report('default', c, plain, quant)
        for n, e in plain + (quant or []):
            assert e < RTOL, (n, e)
    record(request, res)


# ----------------------------------------------------------------------------- DEP_SV16=0
@pytest.mark.parametrize('c', S.ENVIRONMENTS['sv16_off'][1], ids=ident)
def test_fp32_saved_gates_against_the_oracle(c, switch_dir, request):
    res = results('sv16_off', switch_dir)[c['name']]
    base = results('default', switch_dir)[c['name']]
    ref = reference(c, f64(res['mask']) if c['p'] > 0 else None)
    check_outputs(c, res, ref, 'DEP_SV16=0')
    errs = gradient_errors(c, res, ref)
    report('DEP_SV16=0', c, errs)
    for n, e in errs:
        assert e < RTOL, (n, e)
    forward_is_bit_identical(res, base)             # the gates are only stored for the backward
    record(request, res)


# ----------------------------------------------------------------------------- DEP_LSTM_SV16=1
@pytest.mark.parametrize('c', S.ENVIRONMENTS['lstm_sv16'][1], ids=ident)
def test_16bit_saved_bilstm_gates_against_the_oracle_fed_the_quantised_gates(c, switch_dir, request):
    res = results('lstm_sv16', switch_dir)[c['name']]
    base = results('default', switch_dir)[c['name']]
    mask = f64(res['mask']) if c['p'] > 0 else None
    check_outputs(c, res, reference(c, mask), 'DEP_LSTM_SV16=1')
    if c['regime'] != 'init':
        check_16bit_regime('DEP_LSTM_SV16=1', c, res, mask)
    else:
        quant = gradient_errors(c, res, reference(c, mask, quantised=True))
        report('DEP_LSTM_SV16=1', c, gradient_errors(c, res, reference(c, mask)), quant)   # (the plain oracle: a figure, no bar)
        for n, e in quant:
            assert e < RTOL, (n, e)
    forward_is_bit_identical(res, base)             # SV16 touches the write-out of the saved gates alone (module docstring)
    assert any(not np.array_equal(res[k], base[k]) for k in res if k.startswith('g')), 'the 16-bit gates moved no gradient'
    record(request, res)


# ----------------------------------------------------------------------------- DEP_TRACE=1
@pytest.mark.parametrize('tag,c', [('trace', c) for c in S.ENVIRONMENTS['trace'][1]] + [('trace_sv16_off', c) for c in S.ENVIRONMENTS['trace_sv16_off'][1]],
                         ids=lambda v: v if isinstance(v, str) else v['name'])
def test_stamped_variants_are_bit_identical(tag, c, switch_dir, request):
    """The stamps touch no arithmetic: every output and every gradient equals the unstamped run's, which the tests above hold to the oracle."""
    res = results(tag, switch_dir)[c['name']]
    base = results('default' if tag == 'trace' else 'sv16_off', switch_dir)[c['name']]
    assert sorted(k for k in res if k != 'instances') == sorted(k for k in base if k != 'instances')
    for k in res:
        if k != 'instances':
            assert np.isfinite(res[k]).all(), k
            assert np.array_equal(res[k], base[k]), (k, float(np.abs(f64(res[k]) - f64(base[k])).max()))
    record(request, res)


# ----------------------------------------------------------------------------- bf16 storage (dep_set_gemm_mode(3))
def check_bf16_storage(a, b):
    """Bars of test_bf16_storage_mode_has_its_own_tolerance: a = mode 2 (single bf16 products, fp32 storage), b = mode 3."""
    forward_is_bit_identical({k: a[k] for k in ('pooled', 'h_n')}, {k: b[k] for k in ('pooled', 'h_n')})
    worst = 0.0
    for k in a:
        if k.startswith('g') or k == 'dx':
            assert np.isfinite(b[k]).all(), k
            rel = np.abs(f64(a[k]) - f64(b[k])).max() / max(np.abs(f64(a[k])).max(), 1e-30)
            worst = max(worst, rel)
            assert rel < 1e-2, (k, rel)
    assert worst > 1e-5                             # the mode is really in effect
    return worst


@pytest.mark.parametrize('c', S.GRU_FUSED_PK, ids=ident)
def test_per_layer_bf16_storage_backward(c, switch_dir, request):
    """DEP_FUSED2_BWD=0: gru_bwd_cluster_r1<4, true, 4, true, true, true> behind the fused bf16-storage forward."""
    got = results('layer_bwd', switch_dir)
    a, b = got[c['name'][:-1] + '2'], got[c['name'][:-1] + '3']
    worst = check_bf16_storage(a, b)
    print(f'switch-forms DEP_FUSED2_BWD=0 {c["name"]}: bf16 storage moves a gradient by at most {worst:.3e} of its scale')
    record(request, a, b)


@pytest.mark.parametrize('c', S.GRU_FUSED_PK, ids=ident)
def test_fused_bf16_storage_forms(c):
    """In-process: the fused forward and backward of mode 3, both call forms, dropout off and on (conftest.py records the instances)."""
    from icassp2022_depression_amd import _lib as L
    import switch_probe
    D, Y = TF[c['p'] > 0], TF[c['form'] == 'full']
    try:
        a = switch_probe.run_case(dict(c, mode=2), own_log=False)
        mid = L.instance_log_read()
        b = switch_probe.run_case(dict(c, mode=3), own_log=False)
        inst = L.instance_log_read()
    finally:
        L.set_gemm_mode(1, 1 << 28)
    want = {'(gru2_fwd_fused<%s, false, true, true>)' % D, '(gru2_bwd_fused<%s, %s, true, true, false, true>)' % (D, Y)}
    assert want <= inst and not want & mid, (sorted(want), sorted(inst))
    worst = check_bf16_storage(a, b)
    print(f'switch-forms mode 3 {c["name"]}: bf16 storage moves a gradient by at most {worst:.3e} of its scale')


def test_bf16_storage_refuses_a_stack_too_small_for_the_pk_image():
    """Below the PK threshold (tests/switch_cases.py, GRU_FUSED_PK) the bf16-storage backward has no form to run: the call fails loudly,
    it does not fall back to fp32 storage behind a bf16 forward."""
    from icassp2022_depression_amd import _lib as L
    import switch_probe
    c = S.GRU_FUSED[1]
    assert c['T'] % 2 == 0 and not S.writes_pk_image(c)
    try:
        with pytest.raises(L.DepError, match='bf16-storage mode needs the pre-split gate-gradient path'):
            switch_probe.run_case(dict(c, mode=3), own_log=False)
    finally:
        L.set_gemm_mode(1, 1 << 28)
