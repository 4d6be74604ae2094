"""Recurrent state in and out, the parts that need no GPU: the yardstick of the GPU tests (tests/hx_ref.py) against stock
torch.nn.GRU / torch.nn.LSTM float64 autograd with a random initial state, the same yardstick with a zero state against the
composition of the unchanged oracle (tests/stack_ref.py), and the refusals dep_rnn_forward_state / dep_rnn_backward_state make
before any HIP call.  Bars are those of tests/test_varlen_cpu.py: 1e-13 on outputs, 1e-12 relative on gradients."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hx_ref
from stack_ref import stack as oracle_stack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = 'rnn'
STATE = ('dep_rnn_forward_state', 'dep_rnn_backward_state')
CASES = [(cell, dirs, L, T) for cell in ('gru', 'lstm') for dirs in (1, 2) for L in (1, 2, 3) for T in (9, 1)]
ident = lambda c: '-'.join(str(v) for v in c)


def _params(rng, cell, F, H, L, dirs):
    G = 3 if cell == 'gru' else 4
    P = {}
    for l in range(L):
        for d in range(dirs):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else H * dirs
            for nm, shp in (('weight_ih', (G * H, inp)), ('weight_hh', (G * H, H)), ('bias_ih', (G * H,)), ('bias_hh', (G * H,))):
                P[f'{PREFIX}.{nm}_{sfx}'] = rng.uniform(-0.4, 0.4, shp)
    return P


def _rel_ok(a, ref, what):
    assert np.abs(a - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what


@pytest.mark.parametrize('case', CASES, ids=ident)
def test_hx_ref_equals_torch_with_a_random_state(case):
    """y, h_n, c_n, dx, every weight gradient and the gradients of hx / cx, with dy, dh_n and dc_n all non-zero."""
    torch = pytest.importorskip('torch')
    cell, dirs, L, T = case
    B, F, H = 7, 5, 6
    rng = np.random.default_rng(11 + 7 * dirs + 31 * L + T)
    P = _params(rng, cell, F, H, L, dirs)
    x = rng.standard_normal((B, T, F))
    hx = rng.standard_normal((L * dirs, B, H)) * 0.7
    cx = rng.standard_normal((L * dirs, B, H)) * 0.7 if cell == 'lstm' else None
    dy = rng.standard_normal((B, T, dirs * H))
    dhn = rng.standard_normal((L * dirs, B, H))
    dcn = rng.standard_normal((L * dirs, B, H)) if cell == 'lstm' else None
    mod = (torch.nn.GRU if cell == 'gru' else torch.nn.LSTM)(F, H, num_layers=L, batch_first=True, bidirectional=dirs == 2).double()
    with torch.no_grad():
        for k, v in P.items():
            getattr(mod, k.split('.', 1)[1]).copy_(torch.from_numpy(v))
    xt = torch.from_numpy(x).requires_grad_(True)
    ht = torch.from_numpy(hx).requires_grad_(True)
    if cell == 'gru':
        yt, hnt = mod(xt, ht)
        loss = (yt * torch.from_numpy(dy)).sum() + (hnt * torch.from_numpy(dhn)).sum()
    else:
        ct = torch.from_numpy(cx).requires_grad_(True)
        yt, (hnt, cnt) = mod(xt, (ht, ct))
        loss = (yt * torch.from_numpy(dy)).sum() + (hnt * torch.from_numpy(dhn)).sum() + (cnt * torch.from_numpy(dcn)).sum()
    loss.backward()
    r = hx_ref.stack(x, P, PREFIX, cell, dirs, L, hx=hx, cx=cx, dy=dy, dhn=dhn, dcn=dcn)
    assert np.abs(r['y'] - yt.detach().numpy()).max() < 1e-13
    assert np.abs(r['h_n'] - hnt.detach().numpy()).max() < 1e-13
    _rel_ok(r['dx'], xt.grad.numpy(), 'dx')
    _rel_ok(r['dhx'], ht.grad.numpy(), 'dhx')
    if cell == 'lstm':
        assert np.abs(r['c_n'] - cnt.detach().numpy()).max() < 1e-13
        _rel_ok(r['dcx'], ct.grad.numpy(), 'dcx')
    assert np.abs(ht.grad.numpy()).max() > 0
    for k, g in r['G'].items():
        _rel_ok(g, getattr(mod, k.split('.', 1)[1]).grad.numpy(), k)


@pytest.mark.parametrize('case', CASES, ids=ident)
def test_hx_ref_with_a_zero_state_equals_the_oracle_composition(case):
    cell, dirs, L, T = case
    B, F, H = 7, 5, 6
    rng = np.random.default_rng(3 + 5 * dirs + 17 * L + T)
    P = _params(rng, cell, F, H, L, dirs)
    x = rng.standard_normal((B, T, F))
    dy = rng.standard_normal((B, T, dirs * H))
    dhn = rng.standard_normal((L * dirs, B, H))
    pool = 'mean' if cell == 'gru' else 'none'
    dpooled = rng.standard_normal((B, dirs * H)) if cell == 'gru' else None
    ref = oracle_stack(x, P, PREFIX, cell, dirs, L, pool=pool, dy=dy, dpooled=dpooled, dhn=dhn)
    for hx in (None, np.zeros((L * dirs, B, H))):
        r = hx_ref.stack(x, P, PREFIX, cell, dirs, L, hx=hx, cx=hx if cell == 'lstm' else None, pool=pool, dy=dy, dpooled=dpooled, dhn=dhn)
        assert np.abs(r['y'] - ref['y']).max() < 1e-13
        assert np.abs(r['h_n'] - ref['h_n']).max() < 1e-13
        for l in range(L):
            assert np.abs(r['ys'][l] - ref['ys'][l]).max() < 1e-13
        if cell == 'gru':
            assert np.abs(r['pooled'] - ref['pooled']).max() < 1e-13
        _rel_ok(r['dx'], ref['dx'], 'dx')
        for k, g in r['G'].items():
            _rel_ok(g, ref['G'][k], k)


# ----------------------------------------------------------------------------- the built library, without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib
    return _lib, _lib.load()


def test_state_symbols_in_header_library_and_binding(lib):
    _lib, _ = lib
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in STATE:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), f'{name} is not declared in include/dep_rnn.h'
        assert name in _lib.EXPORTS and name in exported, name
    for struct in ('dep_rnn_state', 'dep_rnn_state_grad'):
        assert re.search(r'\}\s*' + struct + r'\s*;', header), struct
    assert 'h0 = c0 = 0 always' not in header


FAKE = 0x1000           # a non-NULL state pointer: the refusals under test come before anything reads it


def _fwd(_lib, L, desc, st):
    return L.dep_rnn_forward_state(C.byref(desc), None, None, None, None, None, None if st is None else C.byref(st), None, 0, None, 0, None)


def _bwd(_lib, L, desc, st):
    return L.dep_rnn_backward_state(C.byref(desc), None, None, None, None, None, None if st is None else C.byref(st), None, None,
                                    None, 0, None, 0, None, None)


CLUSTER = [('gru', 256, 1, 0), ('gru', 256, 1, 3), ('lstm', 128, 2, 0)]


@pytest.mark.parametrize('cell,H,dirs,impl', CLUSTER)
def test_state_on_a_cluster_descriptor_is_refused_with_the_rule(lib, cell, H, dirs, impl):
    _lib, L = lib
    for training in (_lib.RUN_EVAL, _lib.RUN_TRAIN):
        desc = _lib.RnnDesc(_lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM, 4, 3, 8, H, 2, dirs, training, 0.0, 0, _lib.POOL_NONE, impl)
        assert L.dep_rnn_workspace_xbuf_offset(C.byref(desc)) != C.c_size_t(-1).value           # the layout has a cluster exchange buffer
        assert _fwd(_lib, L, desc, _lib.RnnState(FAKE, None, None)) == -1                        # DEP_ERR_ARG
        msg = L.dep_last_error().decode()
        assert 'dep_rnn_forward_state' in msg and 'cluster exchange buffer' in msg and 'dep_rnn_workspace_xbuf_offset' in msg, msg
        assert f'H = {H}' in msg and f'impl = {impl}' in msg, msg
    assert _bwd(_lib, L, desc, _lib.RnnStateGrad(None, None, None, FAKE, None)) == -1
    msg = L.dep_last_error().decode()
    assert 'dep_rnn_backward_state' in msg and 'cluster exchange buffer' in msg, msg
    # without state the same descriptor is not refused by this rule: it gets as far as the plain call's own argument checks
    assert _fwd(_lib, L, desc, None) == -1 and 'cluster exchange buffer' not in L.dep_last_error().decode()
    assert _fwd(_lib, L, desc, _lib.RnnState(None, None, None)) == -1 and 'cluster exchange buffer' not in L.dep_last_error().decode()


@pytest.mark.parametrize('member', ['cx', 'c_n'])
def test_cell_state_on_a_gru_is_refused(lib, member):
    _lib, L = lib
    desc = _lib.RnnDesc(_lib.CELL_GRU, 4, 3, 8, 16, 2, 1, _lib.RUN_TRAIN, 0.0, 0, _lib.POOL_NONE, 2)
    assert L.dep_rnn_workspace_xbuf_offset(C.byref(desc)) == C.c_size_t(-1).value
    st = _lib.RnnState(None, None, None)
    setattr(st, member, FAKE)
    assert _fwd(_lib, L, desc, st) == -1
    assert "LSTM's cell state" in L.dep_last_error().decode()
    for m in ('cx', 'dc_n', 'dcx'):
        sg = _lib.RnnStateGrad(None, None, None, None, None)
        setattr(sg, m, FAKE)
        assert _bwd(_lib, L, desc, sg) == -1
        assert "LSTM's cell state" in L.dep_last_error().decode(), m
