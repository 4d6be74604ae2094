"""Recurrent state together with lengths, the parts that need no GPU: the expectation builder of the GPU tests
(tests/state_varlen_ref.py) against stock torch float64 autograd over a packed batch with a random initial state; chunk composition
on the builder alone (what justifies the len_b = 0 pass-through); the new symbols in header, library and binding; and the refusals
dep_rnn_forward_state_varlen / dep_rnn_backward_state_varlen make before any HIP call.
Bars are those of tests/test_rnn_state_cpu.py: 1e-13 on outputs, 1e-12 relative on gradients."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import state_varlen_ref as svr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = 'rnn'
NEW = ('dep_rnn_forward_state_varlen', 'dep_rnn_backward_state_varlen')
CASES = [(cell, dirs, L) for cell in ('gru', 'lstm') for dirs in (1, 2) for L in (1, 2, 3)]
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


# ----------------------------------------------------------------------------- (a) the builder against stock torch
@pytest.mark.parametrize('case', CASES, ids=ident)
def test_builder_equals_torch_packed_with_a_random_state(case):
    """pack_padded_sequence(enforce_sorted=False) into nn.GRU / nn.LSTM with random hx / cx and non-zero dy, dh_n, dc_n.  torch refuses
    a length of 0, so it runs the rows with len_b >= 1; the builder runs all rows, and its weight gradients must not move for the
    empty ones."""
    torch = pytest.importorskip('torch')
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    cell, dirs, L = case
    B, T, F, H = 8, 9, 5, 6
    K = L * dirs
    rng = np.random.default_rng(101 + 7 * dirs + 31 * L + (cell == 'lstm'))
    lengths = np.array([T, 1, 0, 4, 2, 0, T - 1, 3])
    P = _params(rng, cell, F, H, L, dirs)
    x = rng.standard_normal((B, T, F))
    hx = rng.standard_normal((K, B, H)) * 0.7
    cx = rng.standard_normal((K, B, H)) * 0.7 if cell == 'lstm' else None
    dy = rng.standard_normal((B, T, dirs * H))
    dhn = rng.standard_normal((K, B, H))
    dcn = rng.standard_normal((K, B, H)) if cell == 'lstm' else None
    r = svr.stack(x, lengths, P, PREFIX, cell, dirs, L, hx=hx, cx=cx, dy=dy, dhn=dhn, dcn=dcn)

    live = np.nonzero(lengths > 0)[0]
    mod = (torch.nn.GRU if cell == 'gru' else torch.nn.LSTM)(F, H, num_layers=L, batch_first=True, bidirectional=dirs == 2).double()
    with torch.no_grad():
        for k, v in P.items():
            getattr(mod, k.split('.', 1)[1]).copy_(torch.from_numpy(v))
    xt = torch.from_numpy(x[live]).requires_grad_(True)
    ht = torch.from_numpy(np.ascontiguousarray(hx[:, live])).requires_grad_(True)
    packed = pack_padded_sequence(xt, torch.from_numpy(lengths[live]), batch_first=True, enforce_sorted=False)
    sel = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, live]))
    if cell == 'gru':
        yp, hnt = mod(packed, ht)
        extra = (hnt * sel(dhn)).sum()
    else:
        ct = torch.from_numpy(np.ascontiguousarray(cx[:, live])).requires_grad_(True)
        yp, (hnt, cnt) = mod(packed, (ht, ct))
        extra = (hnt * sel(dhn)).sum() + (cnt * sel(dcn)).sum()
    yt, _ = pad_packed_sequence(yp, batch_first=True, total_length=T)
    ((yt * torch.from_numpy(dy[live])).sum() + extra).backward()

    assert np.abs(r['y'][live] - yt.detach().numpy()).max() < 1e-13
    assert np.abs(r['h_n'][:, live] - hnt.detach().numpy()).max() < 1e-13
    _rel_ok(r['dx'][live], xt.grad.numpy(), 'dx')
    _rel_ok(r['dhx'][:, live], ht.grad.numpy(), 'dhx')
    assert np.abs(ht.grad.numpy()).max() > 0
    if cell == 'lstm':
        assert np.abs(r['c_n'][:, live] - cnt.detach().numpy()).max() < 1e-13
        _rel_ok(r['dcx'][:, live], ct.grad.numpy(), 'dcx')
    for k, g in r['G'].items():
        _rel_ok(g, getattr(mod, k.split('.', 1)[1]).grad.numpy(), k)
    # padding, and the rows torch cannot run: the state and its gradient pass through bit for bit, everything else is 0
    for b in range(B):
        assert not r['y'][b, lengths[b]:].any() and not r['dx'][b, lengths[b]:].any()
    for b in np.nonzero(lengths == 0)[0]:
        assert np.array_equal(r['h_n'][:, b], hx[:, b]) and np.array_equal(r['dhx'][:, b], dhn[:, b])
        if cell == 'lstm':
            assert np.array_equal(r['c_n'][:, b], cx[:, b]) and np.array_equal(r['dcx'][:, b], dcn[:, b])


# ----------------------------------------------------------------------------- (b) chunk composition, on the builder alone
@pytest.mark.parametrize('L', [1, 2])
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_chunks_compose_under_the_pass_through_rule(cell, L):
    """Unidirectional T = 7 cut as 1 + 4 + 2 with per-chunk lengths clip(n_b - t_start, 0, Tc): the forward carries the state, the
    backward walks the chunks in reverse with dhx / dcx fed back as dh_n / dc_n.  Outputs and summed weight gradients equal the builder
    on the whole ragged sequence -- which holds only if a row that has ended (chunk length 0) hands h / c and dh / dc through."""
    B, T, F, H, cuts = 6, 7, 5, 6, (1, 4, 2)
    lstm = cell == 'lstm'
    rng = np.random.default_rng(7 + L + 10 * lstm)
    n = np.array([7, 0, 1, 5, 3, 6])
    P = _params(rng, cell, F, H, L, 1)
    x = rng.standard_normal((B, T, F))
    hx = rng.standard_normal((L, B, H)) * 0.7
    cx = rng.standard_normal((L, B, H)) * 0.7 if lstm else None
    dy = rng.standard_normal((B, T, H))
    dhn = rng.standard_normal((L, B, H))
    dcn = rng.standard_normal((L, B, H)) if lstm else None
    whole = svr.stack(x, n, P, PREFIX, cell, 1, L, hx=hx, cx=cx, dy=dy, dhn=dhn, dcn=dcn)

    h, c = hx, cx
    chunks = []
    t0 = 0
    for Tc in cuts:
        nc = np.clip(n - t0, 0, Tc)
        f = svr.stack(x[:, t0:t0 + Tc], nc, P, PREFIX, cell, 1, L, hx=h, cx=c)
        chunks.append((t0, Tc, nc, h, c, f['y']))
        h, c = f['h_n'], f.get('c_n')
        t0 += Tc
    assert np.abs(np.concatenate([ch[-1] for ch in chunks], 1) - whole['y']).max() < 1e-13
    assert np.abs(h - whole['h_n']).max() < 1e-13
    if lstm:
        assert np.abs(c - whole['c_n']).max() < 1e-13
    dh, dc = dhn, dcn
    dx = np.zeros_like(x)
    G = {k: np.zeros_like(v) for k, v in P.items()}
    for t0, Tc, nc, h0, c0, _ in reversed(chunks):
        r = svr.stack(x[:, t0:t0 + Tc], nc, P, PREFIX, cell, 1, L, hx=h0, cx=c0, dy=dy[:, t0:t0 + Tc], dhn=dh, dcn=dc)
        dx[:, t0:t0 + Tc] = r['dx']
        for k in G:
            G[k] += r['G'][k]
        dh, dc = r['dhx'], r.get('dcx')
    _rel_ok(dx, whole['dx'], 'dx')
    _rel_ok(dh, whole['dhx'], 'dhx')
    if lstm:
        _rel_ok(dc, whole['dcx'], 'dcx')
    for k in G:
        _rel_ok(G[k], whole['G'][k], k)


# ----------------------------------------------------------------------------- the built library, without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib
    return _lib, _lib.load()


def test_state_varlen_symbols_in_header_library_and_binding(lib):
    _lib, _ = lib
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW + ('dep_stream_accumulate', 'dep_stream_finish'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), f'{name} is not declared in include/dep_rnn.h'
        assert name in _lib.EXPORTS and name in exported, name
    for method in ('forward_state_varlen', 'backward_state_varlen'):
        assert callable(getattr(_lib.Rnn, method, None)), method


FAKE = 0x1000           # a non-NULL pointer: the refusals under test come before anything reads it


def _fwd(L, desc, st, lengths=FAKE):
    return L.dep_rnn_forward_state_varlen(C.byref(desc), None, lengths, None, None, None, None, None if st is None else C.byref(st),
                                          None, 0, None, 0, None)


def _bwd(L, desc, st, lengths=FAKE):
    return L.dep_rnn_backward_state_varlen(C.byref(desc), None, lengths, None, None, None, None, None if st is None else C.byref(st),
                                           None, None, None, 0, None, 0, None, None)


def test_null_lengths_is_refused(lib):
    _lib, L = lib
    desc = _lib.RnnDesc(_lib.CELL_GRU, 4, 3, 8, 16, 2, 1, _lib.RUN_TRAIN, 0.0, 0, _lib.POOL_NONE, 2)
    assert _fwd(L, desc, _lib.RnnState(FAKE, None, None), lengths=None) == -1                  # DEP_ERR_ARG
    msg = L.dep_last_error().decode()
    assert 'dep_rnn_forward_state_varlen' in msg and 'lengths' in msg, msg
    assert _bwd(L, desc, _lib.RnnStateGrad(FAKE, None, None, None, None), lengths=None) == -1
    msg = L.dep_last_error().decode()
    assert 'dep_rnn_backward_state_varlen' in msg and 'lengths' in msg, msg


@pytest.mark.parametrize('cell,H,dirs,impl', [('gru', 256, 1, 0), ('gru', 256, 1, 3), ('lstm', 128, 2, 0)])
def test_ragged_state_on_a_cluster_descriptor_is_refused_with_the_rule(lib, cell, H, dirs, impl):
    _lib, L = lib
    for training in (_lib.RUN_EVAL, _lib.RUN_TRAIN):
        desc = _lib.RnnDesc(_lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM, 4, 3, 8, H, 2, dirs, training, 0.0, 0, _lib.POOL_NONE, impl)
        assert L.dep_rnn_workspace_xbuf_offset(C.byref(desc)) != C.c_size_t(-1).value           # the layout has a cluster exchange buffer
        assert _fwd(L, desc, _lib.RnnState(FAKE, None, None)) == -1
        msg = L.dep_last_error().decode()
        assert 'dep_rnn_forward_state_varlen' in msg and 'cluster exchange buffer' in msg and 'dep_rnn_workspace_xbuf_offset' in msg, msg
        assert f'H = {H}' in msg and f'impl = {impl}' in msg, msg
    assert _bwd(L, desc, _lib.RnnStateGrad(None, None, None, FAKE, None)) == -1
    msg = L.dep_last_error().decode()
    assert 'dep_rnn_backward_state_varlen' in msg and 'cluster exchange buffer' in msg, msg
    # without state the same descriptor is not refused by this rule: it gets as far as the plain ragged call's own argument checks
    assert _fwd(L, desc, None) == -1 and 'cluster exchange buffer' not in L.dep_last_error().decode()
    assert _fwd(L, desc, _lib.RnnState(None, None, None)) == -1 and 'cluster exchange buffer' not in L.dep_last_error().decode()


@pytest.mark.parametrize('member', ['cx', 'c_n'])
def test_ragged_cell_state_on_a_gru_is_refused(lib, member):
    _lib, L = lib
    desc = _lib.RnnDesc(_lib.CELL_GRU, 4, 3, 8, 16, 2, 1, _lib.RUN_TRAIN, 0.0, 0, _lib.POOL_NONE, 2)
    assert L.dep_rnn_workspace_xbuf_offset(C.byref(desc)) == C.c_size_t(-1).value
    st = _lib.RnnState(None, None, None)
    setattr(st, member, FAKE)
    assert _fwd(L, desc, st) == -1
    assert "LSTM's cell state" in L.dep_last_error().decode()
    for m in ('cx', 'dc_n', 'dcx'):
        sg = _lib.RnnStateGrad(None, None, None, None, None)
        setattr(sg, m, FAKE)
        assert _bwd(L, desc, sg) == -1
        assert "LSTM's cell state" in L.dep_last_error().decode(), m
