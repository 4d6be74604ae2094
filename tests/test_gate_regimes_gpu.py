"""GPU parity outside init-scale gates, for the sweep families the children of tests/test_switch_forms_gpu.py do not reach.

Every other parity test draws weights and biases uniform in +-1/sqrt(H) and a standard normal x: every gate sits near 0.5.  The regimes
of tests/switch_cases.py (apply_regime) move the same kind of draw to where a trained network lives -- 'memory': update / forget gates
near 0.98, 'sat': weights times 4, saturated candidates and cell values -- where a gate function that saturates badly, a wrong order in
(1 - z) n + z h or a lost factor (1 - z) shows and init-scale inputs hide it.

  A  the generic (impl 1) and tile-MFMA (impl 2) sweeps, GRU and BiLSTM, forward and backward
  B  the bidirectional GRU on the tile sweeps
  C  recurrent state in and out: one forward_state / backward_state call with a non-zero hx (cx); one impl = 4 forward from hx in eval mode
  D  one long chain: the fused two-layer GRU at 16 x 300 x 256, H = 256, 'memory', the training step's call form -- the only case in
     the suite where the forward error can accumulate over the ~50 steps a z of 0.98 remembers

A to C save fp32 gates: every output within 1e-4 absolute, every gradient, dx and state gradient within 1e-4 relerr of the exact float64
reference (tests/hx_ref.py, pinned against stock torch in tests/test_rnn_state_cpu.py).  D runs twice: in this process with the
default 16-bit saved gates, held to the exact oracle under RTOL + 2 E_q (E_q: what the storage format alone does to this case, from the
oracle -- tests/test_switch_cases_cpu.py), and once in a child with DEP_SV16=0 (the switch is read once per process), held to RTOL.
Every check prints its worst figures ('gate-regimes <section> ...'; pytest -s shows them).

Figures of the last device run (one MI355X), worst over a section's cases, memory | sat:
  A  generic and tile sweeps   outputs 5.1e-7 | 2.3e-6 abs      gradients 3.1e-6 | 7.7e-6 relerr
  B  BiGRU                     outputs 1.8e-7 | 1.8e-6          gradients 4.2e-6 | 4.3e-6
  C  state call                outputs 5.4e-7 | 1.0e-6          gradients 3.2e-6 | 5.5e-6;   impl = 4 from hx: outputs 7.7e-7 | 2.1e-5
  D  16 x 300 x 256 memory     outputs 1.2e-6;  gradients: 16-bit gates 1.69e-4 (E_q 1.67e-4, bound 4.3e-4; 3.8e-5 from the oracle fed the
                               16-bit gates), fp32 gates 5.5e-6
Run on the MI355X box:  python -m pytest tests/test_gate_regimes_gpu.py -m gpu -q -s
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hx_ref
import switch_cases as S

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]
HERE = os.path.dirname(os.path.abspath(__file__))

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

ATOL = 1e-4
RTOL = 1e-4
NAN = float('nan')
LAYERS = 2
REGIMES = ('memory', 'sat')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


@pytest.fixture(autouse=True)
def gemm_mode():
    """The split-precision contractions on every size, what the models run (tests/switch_probe.py sets the same)."""
    L.set_gemm_mode(1, 0)
    yield
    L.set_gemm_mode(1, 1 << 28)


def worst(e):
    return max(e, key=lambda v: float('inf') if v[0] != v[0] else v[0])


def compare(section, what, outs, grads=(), rtol=RTOL):
    """outs / grads: lists of (name, device value as float64, reference).  The worst figures are printed before any assertion."""
    ea = [(float(np.abs(a - b).max()) if np.isfinite(a).all() else NAN, n) for n, a, b in outs]
    er = [(float(S.relerr(a, b)) if np.isfinite(a).all() else NAN, n) for n, a, b in grads]
    print(f'gate-regimes {section} {what}:' + (f' worst abs {worst(ea)[0]:.3e} ({worst(ea)[1]})' if ea else '') +
          (f' worst rel {worst(er)[0]:.3e} ({worst(er)[1]})' if er else ''))
    for e, n in ea:
        assert e < ATOL, f'{n}: {e:.3e}'
    for (e, n), (_, a, b) in zip(er, grads):
        if not b.any():                                                # (dW_hh of a single step from a zero state)
            assert 'weight_hh' in n and not a.any(), f'{n}: the reference gradient is zero'
        assert e < rtol, f'{n}: {e:.3e}'
    return worst(er)[0] if er else 0.0


def draw(cell, dirs, B, T, F, H, regime, seed):
    """An init-scale draw (switch_cases.make_rnn_params, x standard normal) moved to `regime`."""
    rng = np.random.default_rng(seed)
    P, names, prefix = S.make_rnn_params(rng, cell, F, H, LAYERS, dirs)
    x = S.f32(rng.standard_normal((B, T, F)))
    P, x = S.apply_regime(regime, cell, P, x)
    return rng, P, names, prefix, x


def run_stack(section, cell, dirs, B, T, F, H, impl, regime, state=False):
    """One forward + backward of a two-layer stack in `regime` against hx_ref.stack; state: hx (cx) in, dhx (dcx) out, dc_n in."""
    gru = cell == 'gru'
    W, K = H * dirs, LAYERS * dirs
    rng, P, names, prefix, x = draw(cell, dirs, B, T, F, H, regime, B * 1000 + T * 100 + F + H + impl + dirs)
    hx = S.f32(rng.standard_normal((K, B, H)) * 0.6) if state else None
    cx = S.f32(rng.standard_normal((K, B, H)) * 0.6) if state and not gru else None
    dy = S.f32(rng.standard_normal((B, T, W)) * 0.3)
    dpool = S.f32(rng.standard_normal((B, W))) if gru else None
    dhn = S.f32(rng.standard_normal((K, B, H)) * 0.3)
    dcn = S.f32(rng.standard_normal((K, B, H)) * 0.3) if state and not gru else None
    opt = lambda a: None if a is None else dev(a)
    Wd = [dev(P[n]) for n in names]
    Gd = [torch.full_like(w, NAN) for w in Wd]
    xd, hxd, cxd = dev(x), opt(hx), opt(cx)
    rnn = L.Rnn(L.CELL_GRU if gru else L.CELL_LSTM, B, T, F, H, LAYERS, dirs, True, 0.0, L.POOL_MEAN if gru else L.POOL_NONE, DEV, impl=impl)
    assert rnn.status_word() is None                                   # the sweeps of rnn_sweep.hip, no cluster plan
    rnn.reserve.fill_(NAN)
    pooled = nans(B, W) if gru else None
    h_n = nans(K, B, H)
    c_n = nans(K, B, H) if state and not gru else None
    rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, hx=hxd, cx=cxd, c_n=c_n)
    dxd = nans(B, T, F)
    dhxd = nans(K, B, H) if state else None
    dcxd = nans(K, B, H) if state and not gru else None
    rnn.backward(xd, Wd, Gd, dy=dev(dy), dpooled=opt(dpool), dh_n=dev(dhn), dx=dxd, hx=hxd, cx=cxd, dc_n=opt(dcn), dhx=dhxd, dcx=dcxd)
    rnn.check()
    ref = hx_ref.stack(x, P, prefix, cell, dirs, LAYERS, hx=hx, cx=cx, pool='mean' if gru else 'none', dy=dy, dpooled=dpool, dhn=dhn, dcn=dcn)
    outs = [(f'layer {l} output', host(rnn.layer_output(l)), yl) for l, yl in enumerate(ref['ys'])]
    outs.append(('h_n', host(h_n), ref['h_n']))
    if gru:
        outs.append(('pooled', host(pooled), ref['pooled']))
    if c_n is not None:
        outs.append(('c_n', host(c_n), ref['c_n']))
    gr = [(n, host(g), ref['G'][n]) for n, g in zip(names, Gd)] + [('dx', host(dxd), ref['dx'])]
    if state:
        gr.append(('dhx', host(dhxd), ref['dhx']))
        if not gru:
            gr.append(('dcx', host(dcxd), ref['dcx']))
    kind = {1: 'generic', 2: 'tile'}[impl]
    compare(section, f'{cell} dirs={dirs} {B}x{T}x{F} H={H} {kind} {regime}' + (' with state' if state else ''), outs, gr)
    inst = {s for s in L.instance_log_read() if re.search(r'(gru|lstm)2?_(fwd|bwd)_', s)}
    assert inst and all(re.search(r'%s_(fwd|bwd)_%s<' % (cell, 'generic' if impl == 1 else 'mfma'), s) for s in inst), sorted(inst)


# ----------------------------------------------------------------------------- A. the generic and tile-MFMA sweeps
# (cell, B, T, F, H): a chain of 20 steps in one wave | a ragged batch tile at the widths the models run (two hidden tiles per wave)
FAMILY_CASES = [('gru', 6, 20, 24, 16), ('gru', 37, 9, 64, 256), ('lstm', 6, 20, 24, 16), ('lstm', 19, 11, 40, 128)]


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('impl', [1, 2], ids=['generic', 'tile'])
@pytest.mark.parametrize('cell,B,T,F,H', FAMILY_CASES)
def test_generic_and_tile_sweeps(cell, B, T, F, H, impl, regime):
    L.instance_log_read(reset=True)
    run_stack('A', cell, 1 if cell == 'gru' else 2, B, T, F, H, impl, regime)


# ----------------------------------------------------------------------------- B. the bidirectional GRU
# tests/test_bigru_gpu.py's smallest shape (one step) and its first with more than one batch tile and three hidden tiles per wave
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('B,T,F,H', [(2, 1, 5, 16), (19, 11, 40, 48)])
def test_bigru_on_the_tile_sweeps(B, T, F, H, regime):
    L.instance_log_read(reset=True)
    run_stack('B', 'gru', 2, B, T, F, H, 2, regime)


# ----------------------------------------------------------------------------- C. recurrent state
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_state_call_with_a_nonzero_state(cell, regime):
    L.instance_log_read(reset=True)
    run_stack('C', cell, 1 if cell == 'gru' else 2, 5, 7, 12, 48, 2, regime, state=True)


@pytest.mark.parametrize('regime', REGIMES)
def test_per_layer_cluster_forward_from_a_state(regime):
    """impl = 4 in eval mode: gru_fwd_cluster_r1 started from hx."""
    B, T, F, H = 33, 4, 16, 256
    rng, P, names, prefix, x = draw('gru', 1, B, T, F, H, regime, B * 1000 + T * 100 + F + H + 4)
    hx = S.f32(rng.standard_normal((LAYERS, B, H)) * 0.6)
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, LAYERS, 1, L.RUN_EVAL, 0.0, L.POOL_MEAN, DEV, impl=L.IMPL_CLUSTER_PER_LAYER)
    assert rnn.status_word() is not None                               # a cluster descriptor
    rnn.reserve.fill_(NAN)
    pooled, h_n, y = nans(B, H), nans(LAYERS, B, H), nans(B, T, H)
    L.instance_log_read(reset=True)
    rnn.forward(dev(x), [dev(P[n]) for n in names], pooled=pooled, h_n=h_n, y=y, hx=dev(hx))
    rnn.check()
    inst = {s for s in L.instance_log_read() if re.search(r'gru2?_fwd_', s)}
    assert inst and all('gru_fwd_cluster_r1<8, true>' in s for s in inst), sorted(inst)
    ref = hx_ref.stack(x, P, prefix, 'gru', 1, LAYERS, hx=hx, pool='mean')
    compare('C', f'impl=4 eval from hx {B}x{T}x{F} H={H} {regime}',
            [(f'layer {l} output', host(rnn.layer_output(l)), yl) for l, yl in enumerate(ref['ys'])] +
            [('y', host(y), ref['y']), ('pooled', host(pooled), ref['pooled']), ('h_n', host(h_n), ref['h_n'])])


# ----------------------------------------------------------------------------- D. the long chain
LONG = S._case('gru', 16, 300, 256, 256, form='model', regime='memory')
_LONG = {}


def long_chain():
    """The inputs, both oracle backwards and E_q of LONG, once per session."""
    if not _LONG:
        inp = S.inputs(LONG)
        exact, quant = S.references(LONG, inp, None, [None, S.quantise_gru_caches])
        _LONG.update(inp=inp, exact=exact, quant=quant, e_q=S.worst_relerr(LONG, inp, quant, exact)[0])
    return _LONG


def long_chain_lists(res, ref, names):
    outs = [(k, res[k].astype(np.float64), ref[k]) for k in ('y', 'pooled', 'h_n')]
    grads = [(n, res['g%d' % i].astype(np.float64), ref['G'][n]) for i, n in enumerate(names)]
    return outs, grads


def test_long_chain_with_16bit_saved_gates():
    """The default of the fused stack.  Outputs at ATOL (the forward does not read the saved gates); gradients against the exact
    oracle under RTOL + 2 E_q, and the figure against the oracle fed the 16-bit gates printed beside it."""
    import switch_probe
    lc = long_chain()
    res = switch_probe.run_case(LONG, own_log=False)
    assert not any('gru2_fwd_fused<false, false, false>' in s for s in L.instance_log_read()), 'this process runs with DEP_SV16=0'
    _LONG['res'] = res
    outs, grads = long_chain_lists(res, lc['exact'], lc['inp']['names'])
    vs_q = max(S.relerr(a, lc['quant']['G'][n]) for n, a, _ in grads)
    print(f'gate-regimes D {LONG["name"]}: E_q {lc["e_q"]:.3e}, bound {RTOL + 2 * lc["e_q"]:.3e}; vs the oracle fed the 16-bit gates {vs_q:.3e}')
    compare('D', '16-bit saved gates', outs, grads, rtol=RTOL + 2 * lc['e_q'])


def test_long_chain_with_fp32_saved_gates(tmp_path):
    """DEP_SV16=0 in a child process: the kernels' own arithmetic over 300 steps at the project's bar, and the bits of the default
    run's forward (the gates are only stored for the backward)."""
    lc = long_chain()
    out = tmp_path / 'long.npz'
    spec = tmp_path / 'long.json'
    spec.write_text(json.dumps([[str(out), LONG]]))
    env = {k: v for k, v in os.environ.items() if k not in S.SWITCHES}
    env['DEP_SV16'] = '0'
    r = subprocess.run([sys.executable, os.path.join(HERE, 'switch_probe.py'), '--batch', str(spec)], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, f'the child exited with {r.returncode}\n' + r.stdout[-2000:] + r.stderr[-3000:]
    res = dict(np.load(out))
    assert '(gru2_fwd_fused<false, false, false>)' in set(str(s) for s in res['instances']), sorted(res['instances'])
    outs, grads = long_chain_lists(res, lc['exact'], lc['inp']['names'])
    compare('D', 'fp32 saved gates (DEP_SV16=0)', outs, grads)
    if 'res' in _LONG:
        for k in ('y', 'pooled', 'h_n'):
            assert np.array_equal(res[k], _LONG['res'][k]), k
