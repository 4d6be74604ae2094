"""GPU parity of the recurrent state together with lengths (dep_rnn_forward_state_varlen / dep_rnn_backward_state_varlen) on the
per-layer tile-MFMA and generic sweeps, and the ragged AudioGRU stream built on it.

The expectation is tests/state_varlen_ref.py: a row loop around the unchanged tests/hx_ref.stack at T' = len_b, pinned against stock
torch's packed nn.GRU / nn.LSTM in tests/test_state_varlen_cpu.py.  Bars are the project's: 1e-4 absolute on every layer's output, y,
pooled, h_n, c_n; 1e-4 relerr on dx, every gradient tensor, dhx, dcx.  Both parity GEMM modes.  Outputs, gradients and the reserve
are pre-filled with NaN.  Every check prints its worst figures ('rnn-state V* ...'; pytest -s shows them).
The helpers are those of tests/test_rnn_state_gpu.py (the dense state call's tests).
Run on the MI355X box:  python -m pytest tests/test_state_varlen_gpu.py -m gpu -q"""
import ctypes as C
import re

import numpy as np
import pytest

import state_varlen_ref as svr
from varlen_ref import lengths_mix

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

from test_rnn_state_gpu import (ATOL, NAN, PREFIX, STATE_SWEEP, all_grads, bits, case_rng, check_sweeps, compare, dev, f32, gemm_mode,  # noqa: E402,F401
                                host, ident, make_audio, make_params, make_rnn, nans, sweep_instances)

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')


def ilen(n):
    return torch.from_numpy(np.asarray(n, dtype=np.int32)).to(DEV)


def lengths_ok(n, T):
    """What a parity length vector must hold: a full row, an empty one, a row of one step (T = 1: the full row is that one), and in every
    16-row tile that has more than three rows a row with 2 <= len <= T-1 -- the row whose reverse sweep starts inside the sequence,
    behind a dead position: the one a backward that takes h_prev / c_prev of that step from memory gets wrong."""
    ok = (n == T).any() and (n == 0).any() and (n == 1).any()
    if T >= 3:
        for r0 in range(0, len(n), 16):
            tile = n[r0:r0 + 16]
            if len(tile) > 3:
                ok = ok and ((tile >= 2) & (tile <= T - 1)).any()
    return bool(ok)


def parity_lengths(B, T):
    n = lengths_mix(B, T)
    seed = 0
    while not lengths_ok(n, T) and seed < 64:          # redrawn with fixed seeds, never skipped
        n = lengths_mix(B, T, np.random.default_rng(1000 + seed))
        seed += 1
    assert lengths_ok(n, T), n
    return n


def run_ragged(cell, dirs, B, T, F, H, Lyr, impl, rng, grads, lengths, p=0.0, seed=0, with_state=True):
    """One ragged forward + backward with a state that is non-zero in every layer and direction.  Returns the (outs, grads) lists for
    compare(), the sweep instances the two calls logged, and the tensors the bit-exact checks look at."""
    gru = cell == 'gru'
    W, K = H * dirs, Lyr * dirs
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    x = f32(rng.standard_normal((B, T, F)))
    for b in range(B):
        x[b, lengths[b]:] = 0.0                                        # finite padding
    hx = f32(rng.standard_normal((K, B, H)) * 0.6) if with_state else None
    cx = None if gru or not with_state else f32(rng.standard_normal((K, B, H)) * 0.6)
    opt = lambda a: None if a is None else dev(a)
    Wd = [dev(P[n]) for n in names]
    Gd = [torch.full_like(w, NAN) for w in Wd]
    xd, hxd, cxd, nd = dev(x), opt(hx), opt(cx), ilen(lengths)
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl, p)
    assert rnn.status_word() is None                                   # no cluster exchange buffer: the sweeps of rnn_sweep.hip run the stack
    pooled = nans(B, W) if gru else None
    h_n = nans(K, B, H)
    c_n = None if gru else nans(K, B, H)
    before = L.instance_log_read()
    rnn.forward_state_varlen(xd, Wd, nd, seed=seed, pooled=pooled, h_n=h_n, hx=hxd, cx=cxd, c_n=c_n)
    masks = None
    if p > 0:
        masks = [host(L.dropout_mask(B * T * W, p, seed, 16 + l, DEV)).reshape(B, T, W) for l in range(Lyr - 1)]      # site = DEP_SITE_RNN0 + l
    dy = f32(rng.standard_normal((B, T, W)) * 0.3) if 'dy' in grads else None
    dpool = f32(rng.standard_normal((B, W))) if 'dpooled' in grads else None
    dhn = f32(rng.standard_normal((K, B, H)) * 0.3) if 'dhn' in grads else None
    dcn = f32(rng.standard_normal((K, B, H)) * 0.3) if 'dcn' in grads else None
    dxd, dhxd = nans(B, T, F), nans(K, B, H)
    dcxd = None if gru else nans(K, B, H)
    dhnd, dcnd = opt(dhn), opt(dcn)
    rnn.backward_state_varlen(xd, Wd, Gd, nd, dy=opt(dy), dpooled=opt(dpool), dh_n=dhnd, dx=dxd, hx=hxd, cx=cxd, dc_n=dcnd, dhx=dhxd, dcx=dcxd)
    rnn.check()
    inst = sweep_instances(L.instance_log_read() - before)
    ref = svr.stack(x, lengths, P, PREFIX, cell, dirs, Lyr, hx=hx, cx=cx, pool='mean' if gru else 'none', dy=dy, dpooled=dpool, dhn=dhn,
                    dcn=dcn, masks=masks)
    outs = [(f'layer {l} output', host(rnn.layer_output(l)), yl) for l, yl in enumerate(ref['ys'])]
    outs.append(('y', host(rnn.layer_output()), ref['y']))
    hn = host(h_n)
    outs += [(f'h_n[{i}]', hn[i], ref['h_n'][i]) for i in range(K)]
    if gru:
        outs.append(('pooled', host(pooled), ref['pooled']))
    else:
        cn = host(c_n)
        outs += [(f'c_n[{i}]', cn[i], ref['c_n'][i]) for i in range(K)]
    gr = []
    for l in range(Lyr - 1, -1, -1):                                   # the order the backward forms them: the first layer that is off
        gr += [(n, host(g), ref['G'][n]) for n, g in zip(names, Gd) if re.search(r'_l%d(_reverse)?$' % l, n)]
    gr.append(('dx', host(dxd), ref['dx']))
    dh = host(dhxd)
    gr += [(f'dhx[{i}]', dh[i], ref['dhx'][i]) for i in range(K)]
    if not gru:
        dc = host(dcxd)
        gr += [(f'dcx[{i}]', dc[i], ref['dcx'][i]) for i in range(K)]
    t = dict(rnn=rnn, h_n=h_n, hx=hxd, c_n=c_n, cx=cxd, dhx=dhxd, dh_n=dhnd, dcx=dcxd, dc_n=dcnd, dx=dxd, pooled=pooled, masks=masks,
             Gd=Gd, names=names)
    return outs, gr, inst, t


def check_padding_and_pass_through(t, lengths, Lyr):
    """Padded positions of every output sequence and of dx are exactly 0.0; an empty row's state and state gradient pass through bit
    for bit (int32 views) and its pooled row is 0."""
    for l in range(Lyr):
        y = host(t['rnn'].layer_output(l))
        for b, n in enumerate(lengths):
            assert not y[b, n:].any(), f'layer {l} output, row {b}: a padded position is not 0'
    dx = host(t['dx'])
    for b, n in enumerate(lengths):
        assert not dx[b, n:].any(), f'dx, row {b}: a padded position is not 0'
    empty = np.nonzero(np.asarray(lengths) == 0)[0]
    assert len(empty)
    for out, inp, what in ((t['h_n'], t['hx'], 'h_n vs hx'), (t['c_n'], t['cx'], 'c_n vs cx'), (t['dhx'], t['dh_n'], 'dhx vs dh_n'),
                           (t['dcx'], t['dc_n'], 'dcx vs dc_n')):
        if out is None:
            continue
        o = bits(out)[:, empty]
        assert np.array_equal(o, bits(inp)[:, empty] if inp is not None else np.zeros_like(o)), what
    if t['pooled'] is not None:
        assert not host(t['pooled'])[empty].any()


# ----------------------------------------------------------------------------- V-A. parity against state_varlen_ref
# (cell, dirs, B, T, F, H, L, impl).  B = 19: two 16-row tiles with a partial second one.  H = 16 / 48: one and several column tiles per
# wave.  H = 20 with impl = 1: the generic kernels.  dirs = 2: the reverse direction's first live step t = len_b - 1 (GRU: tile only).
# T = 1: lengths in {0, 1}, the state's dW_hh term is all of dW_hh.
PARITY_CASES = [
    ('gru', 1, 19, 9, 12, 48, 2, 2), ('gru', 2, 19, 9, 12, 16, 2, 2), ('gru', 2, 19, 5, 12, 48, 3, 2),
    ('lstm', 1, 19, 9, 12, 16, 2, 2), ('lstm', 2, 19, 9, 12, 16, 2, 2), ('lstm', 2, 19, 5, 12, 48, 3, 2),
    ('gru', 1, 5, 7, 7, 20, 2, 1), ('lstm', 2, 5, 5, 7, 20, 3, 1),
    ('gru', 2, 19, 1, 12, 48, 1, 2), ('lstm', 2, 19, 1, 12, 48, 1, 2),
]


@pytest.mark.parametrize('case', PARITY_CASES, ids=ident)
def test_ragged_state_parity_all_gradient_inputs(case, gemm_mode):
    cell, dirs, B, T, F, H, Lyr, impl = case
    n = parity_lengths(B, T)
    outs, gr, inst, t = run_ragged(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, B, T, F, H, Lyr, impl), all_grads(cell), n)
    compare('V-A', ident(case), outs, gr)
    check_sweeps(inst, cell, impl)
    check_padding_and_pass_through(t, n, Lyr)


ALONE_CASES = [('gru', 2, 19, 9, 12, 16, 2, 2), ('gru', 1, 5, 7, 7, 20, 2, 1), ('lstm', 2, 19, 9, 12, 16, 2, 2), ('lstm', 2, 5, 5, 7, 20, 3, 1)]


@pytest.mark.parametrize('which', [0, 1, 2])
@pytest.mark.parametrize('case', ALONE_CASES, ids=ident)
def test_ragged_state_parity_each_gradient_input_alone(case, which, gemm_mode):
    """dy, dpooled (GRU) / dc_n (LSTM) and dh_n each alone: an input treated as absent, or one that only works beside another, shows."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    g = all_grads(cell)[which]
    n = parity_lengths(B, T)
    outs, gr, _, t = run_ragged(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, B, T, F, H, which), (g,), n)
    compare('V-A', ident(case) + ' ' + g + ' alone', outs, gr)
    check_padding_and_pass_through(t, n, Lyr)


@pytest.mark.parametrize('case', [('gru', 2, 19, 9, 12, 16, 2, 2), ('lstm', 2, 19, 9, 12, 16, 2, 2)], ids=ident)
def test_ragged_state_parity_with_dropout_masks(case, gemm_mode):
    """L = 2, p = 0.5: the dense call's masks (unchanged element index); the reference is fed the mask dep_dropout_mask draws."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    n = parity_lengths(B, T)
    outs, gr, _, t = run_ragged(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, B, T, F, H, 5), all_grads(cell), n, p=0.5, seed=4321)
    masks = t['masks']
    assert len(masks) == 1 and set(np.unique(masks[0])).issubset({0.0, 2.0}) and 0.3 < (masks[0] == 0).mean() < 0.7
    compare('V-A', ident(case) + ' p=0.5', outs, gr)


# ----------------------------------------------------------------------------- V-B. equivalences
@pytest.mark.parametrize('case', [('gru', 2, 19, 5, 12, 16, 2, 2), ('lstm', 2, 19, 5, 12, 48, 2, 2), ('gru', 1, 5, 5, 7, 20, 2, 1),
                                  ('lstm', 2, 5, 5, 7, 20, 2, 1)], ids=ident)
def test_lengths_all_T_is_the_dense_state_call(case, gemm_mode):
    cell, dirs, B, T, F, H, Lyr, impl = case
    gru = cell == 'gru'
    W, K = H * dirs, Lyr * dirs
    rng = case_rng(dirs, B, T, F, H, 21)
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    hx = dev(rng.standard_normal((K, B, H)) * 0.6)
    cx = None if gru else dev(rng.standard_normal((K, B, H)) * 0.6)
    dyd, dhnd = dev(rng.standard_normal((B, T, W)) * 0.3), dev(rng.standard_normal((K, B, H)) * 0.3)
    dcnd = None if gru else dev(rng.standard_normal((K, B, H)) * 0.3)
    dpd = dev(rng.standard_normal((B, W))) if gru else None
    nd = ilen(np.full(B, T))
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl)

    def run(ragged):
        rnn.reserve.fill_(NAN)
        pooled, h_n, c_n = nans(B, W) if gru else None, nans(K, B, H), None if gru else nans(K, B, H)
        Gd = [torch.full_like(w, NAN) for w in Wd]
        dx, dhx, dcx = nans(B, T, F), nans(K, B, H), None if gru else nans(K, B, H)
        if ragged:
            rnn.forward_state_varlen(xd, Wd, nd, pooled=pooled, h_n=h_n, hx=hx, cx=cx, c_n=c_n)
            y = rnn.layer_output().clone()
            rnn.backward_state_varlen(xd, Wd, Gd, nd, dy=dyd, dpooled=dpd, dh_n=dhnd, dx=dx, hx=hx, cx=cx, dc_n=dcnd, dhx=dhx, dcx=dcx)
        else:
            rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, hx=hx, cx=cx, c_n=c_n)
            y = rnn.layer_output().clone()
            rnn.backward(xd, Wd, Gd, dy=dyd, dpooled=dpd, dh_n=dhnd, dx=dx, hx=hx, cx=cx, dc_n=dcnd, dhx=dhx, dcx=dcx)
        rnn.check()
        outs = [('y', y), ('pooled', pooled), ('h_n', h_n), ('c_n', c_n)]
        grads = list(zip(names, Gd)) + [('dx', dx), ('dhx', dhx), ('dcx', dcx)]
        return [(n, host(v)) for n, v in outs if v is not None], [(n, host(v)) for n, v in grads if v is not None]

    (ro, rg), (do, dg) = run(True), run(False)
    compare('V-B', ident(case) + ' lengths all T vs dense', [(n, a, b) for (n, a), (_, b) in zip(ro, do)], [(n, a, b) for (n, a), (_, b) in zip(rg, dg)])


def raw_forward(rnn, x, nd, Wd, st, y=None, pooled=None, h_n=None):
    for i, w in enumerate(Wd):
        rnn._warr[i] = w.data_ptr()
    rnn.desc.seed = 0
    p = lambda t: None if t is None else t.data_ptr()
    L.check(rnn.lib.dep_rnn_forward_state_varlen(C.byref(rnn.desc), p(x), p(nd), rnn._warr, p(y), p(pooled), p(h_n),
                                                 None if st is None else C.byref(st), p(rnn.reserve), rnn.reserve.numel() * 4,
                                                 p(rnn.workspace), rnn.workspace.numel() * 4, L.stream()), 'dep_rnn_forward_state_varlen')


def raw_backward(rnn, x, nd, Wd, Gd, st, dy=None, dpooled=None, dh_n=None, dx=None):
    for i, (w, g) in enumerate(zip(Wd, Gd)):
        rnn._warr[i] = w.data_ptr(); rnn._garr[i] = g.data_ptr()
    p = lambda t: None if t is None else t.data_ptr()
    L.check(rnn.lib.dep_rnn_backward_state_varlen(C.byref(rnn.desc), p(x), p(nd), rnn._warr, p(dy), p(dpooled), p(dh_n),
                                                  None if st is None else C.byref(st), rnn._garr, p(dx), p(rnn.reserve),
                                                  rnn.reserve.numel() * 4, p(rnn.workspace), rnn.workspace.numel() * 4, L.stream(), None),
            'dep_rnn_backward_state_varlen')


PLAIN_CASES = [('gru', 2, 19, 5, 12, 48, 2, 2), ('gru', 1, 5, 5, 7, 20, 2, 1), ('lstm', 2, 19, 5, 12, 32, 2, 2), ('lstm', 2, 5, 5, 7, 20, 2, 1),
               ('gru', 1, 20, 6, 12, 128, 2, 3)]       # the last one: a cluster descriptor, where only the call without state is accepted


@pytest.mark.parametrize('case', PLAIN_CASES, ids=ident)
def test_all_null_state_is_the_plain_ragged_call(case, gemm_mode):
    """st = NULL and a struct of NULLs give the bits of dep_rnn_forward_varlen / dep_rnn_backward_varlen and log the same instances."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    gru = cell == 'gru'
    W, K = H * dirs, Lyr * dirs
    rng = case_rng(dirs, B, T, F, H, impl, 2)
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    n = parity_lengths(B, T)
    x = f32(rng.standard_normal((B, T, F)))
    for b in range(B):
        x[b, n[b]:] = 0.0
    Wd = [dev(P[k]) for k in names]
    xd, nd = dev(x), ilen(n)
    dyd, dhnd = dev(rng.standard_normal((B, T, W)) * 0.3), dev(rng.standard_normal((K, B, H)) * 0.3)
    dpd = dev(rng.standard_normal((B, W))) if gru else None
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl)

    def run(fwd, bwd):
        rnn.reserve.fill_(NAN)
        y, pooled, h_n = nans(B, T, W), nans(B, W) if gru else None, nans(K, B, H)
        Gd = [torch.full_like(w, NAN) for w in Wd]
        dx = nans(B, T, F)
        L.instance_log_read(reset=True)
        fwd(y, pooled, h_n)
        bwd(Gd, dx)
        rnn.check()
        torch.cuda.synchronize()
        return [('y', y), ('pooled', pooled), ('h_n', h_n), ('dx', dx)] + list(zip(names, Gd)), L.instance_log_read(reset=True)

    plain, plain_log = run(lambda y, pooled, h_n: rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, y=y, lengths=nd),
                           lambda Gd, dx: rnn.backward(xd, Wd, Gd, dy=dyd, dpooled=dpd, dh_n=dhnd, dx=dx, lengths=nd))
    for what, sf, sb in [('st = NULL', None, None), ('a struct of NULLs', L.RnnState(None, None, None), L.RnnStateGrad(None, None, None, None, None))]:
        got, log = run(lambda y, pooled, h_n: raw_forward(rnn, xd, nd, Wd, sf, y=y, pooled=pooled, h_n=h_n),
                       lambda Gd, dx: raw_backward(rnn, xd, nd, Wd, Gd, sb, dy=dyd, dpooled=dpd, dh_n=dhnd, dx=dx))
        for (k, a), (_, b) in zip(plain, got):
            if a is not None:
                assert torch.isfinite(a).all(), k
                assert np.array_equal(bits(a), bits(b)), f'{what}: {k} differs from the plain ragged call'
        assert log == plain_log, (what, sorted(log ^ plain_log))


# ----------------------------------------------------------------------------- V-C. the launch-instance log
@pytest.mark.parametrize('case', [('gru', 1, 19, 5, 12, 48, 2, 2), ('gru', 2, 19, 5, 12, 16, 2, 2), ('gru', 1, 5, 5, 7, 20, 2, 1),
                                  ('lstm', 2, 19, 5, 12, 16, 2, 2), ('lstm', 2, 5, 5, 7, 20, 2, 1)], ids=ident)
def test_a_ragged_state_call_launches_the_plain_ragged_calls_instances(case):
    """The set of sweep instances a ragged state call logs is the set the same descriptor's plain ragged call logs (the state is a set
    of run-time pointers: no instance was added), and they are the ragged instances of rnn_sweep.hip."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    gru = cell == 'gru'
    K = Lyr * dirs
    rng = case_rng(dirs, B, T, F, H, 13)
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    Gd = [torch.empty_like(w) for w in Wd]
    xd = dev(rng.standard_normal((B, T, F)))
    dyd = dev(rng.standard_normal((B, T, H * dirs)))
    hx = dev(rng.standard_normal((K, B, H)))
    cx = None if gru else dev(rng.standard_normal((K, B, H)))
    nd = ilen(parity_lengths(B, T))
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl)
    h_n, dx = nans(K, B, H), nans(B, T, F)
    L.instance_log_read(reset=True)
    rnn.forward_state_varlen(xd, Wd, nd, h_n=h_n, hx=hx, cx=cx, c_n=None if gru else nans(K, B, H))
    rnn.backward_state_varlen(xd, Wd, Gd, nd, dy=dyd, dx=dx, hx=hx, cx=cx, dhx=nans(K, B, H), dcx=None if gru else nans(K, B, H))
    torch.cuda.synchronize()
    with_state = L.instance_log_read(reset=True)
    rnn.forward(xd, Wd, h_n=h_n, lengths=nd)
    rnn.backward(xd, Wd, Gd, dy=dyd, dx=dx, lengths=nd)
    torch.cuda.synchronize()
    plain = L.instance_log_read()
    sw = sweep_instances(with_state)
    assert sw and all(re.fullmatch(STATE_SWEEP, s) for s in sw), sorted(sw)
    assert all(re.search(r'<(\d, )?true', s) for s in sw), sorted(sw)           # the RAG instances
    assert sw == sweep_instances(plain), (sorted(sw), sorted(sweep_instances(plain)))


# ----------------------------------------------------------------------------- V-D. h_n aliasing hx, c_n aliasing cx
@pytest.mark.parametrize('case', [('gru', 2, 19, 5, 12, 48, 3, 2), ('gru', 1, 5, 5, 7, 20, 3, 1), ('lstm', 2, 19, 5, 12, 16, 3, 2),
                                  ('lstm', 2, 5, 5, 7, 20, 3, 1)], ids=ident)
def test_h_n_may_alias_hx_on_a_ragged_call(case):
    cell, dirs, B, T, F, H, Lyr, impl = case
    gru = cell == 'gru'
    K = Lyr * dirs
    rng = case_rng(dirs, B, T, F, H, 9)
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    hx = dev(rng.standard_normal((K, B, H)) * 0.6)
    cx = None if gru else dev(rng.standard_normal((K, B, H)) * 0.6)
    nd = ilen(parity_lengths(B, T))
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl)
    h_n, c_n = nans(K, B, H), None if gru else nans(K, B, H)
    rnn.forward_state_varlen(xd, Wd, nd, h_n=h_n, hx=hx, cx=cx, c_n=c_n)
    y = rnn.layer_output().clone()
    rnn.reserve.fill_(NAN)
    h2, c2 = hx.clone(), None if gru else cx.clone()
    rnn.forward_state_varlen(xd, Wd, nd, h_n=h2, hx=h2, cx=c2, c_n=c2)
    assert torch.isfinite(h_n).all() and not torch.equal(h_n, hx)
    assert np.array_equal(bits(y), bits(rnn.layer_output())), 'y'
    assert np.array_equal(bits(h_n), bits(h2)), 'h_n written over hx'
    if not gru:
        assert torch.isfinite(c_n).all() and np.array_equal(bits(c_n), bits(c2)), 'c_n written over cx'


# ----------------------------------------------------------------------------- V-E. chunked equals whole on the device
@pytest.mark.parametrize('H,impl', [(48, 2), (20, 1)])
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_ragged_chunked_equals_whole(cell, H, impl, gemm_mode):
    """T = 7 cut as (1, 4, 2) with per-chunk lengths clip(n_b - t_start, 0, Tc): rows end before, inside and at a cut.  The forward carries
    the state in place, the backward walks the chunks in reverse with dhx / dcx as the previous chunk's dh_n / dc_n; held against the
    builder on the WHOLE ragged sequence."""
    gru = cell == 'gru'
    B, T, F, Lyr, cuts = 19, 7, 12, 2, (1, 4, 2)
    rng = case_rng(H, impl, 5 if gru else 6)
    n = rng.integers(0, T + 1, B)
    n[:5] = [7, 0, 1, 5, 3]; n[16:19] = [3, 7, 0]
    P, names = make_params(rng, cell, F, H, Lyr, 1)
    x = f32(rng.standard_normal((B, T, F)))
    for b in range(B):
        x[b, n[b]:] = 0.0
    hx0 = f32(rng.standard_normal((Lyr, B, H)) * 0.6)
    cx0 = None if gru else f32(rng.standard_normal((Lyr, B, H)) * 0.6)
    dy = f32(rng.standard_normal((B, T, H)) * 0.3)
    dhn = f32(rng.standard_normal((Lyr, B, H)) * 0.3)
    dcn = None if gru else f32(rng.standard_normal((Lyr, B, H)) * 0.3)
    ref = svr.stack(x, n, P, PREFIX, cell, 1, Lyr, hx=hx0, cx=cx0, dy=dy, dhn=dhn, dcn=dcn)
    Wd = [dev(P[k]) for k in names]
    h = dev(hx0)
    c = None if gru else dev(cx0)
    chunks = []
    t0 = 0
    for Tc in cuts:
        rnn = make_rnn(cell, 1, B, Tc, F, H, Lyr, impl)
        xc, nc = dev(x[:, t0:t0 + Tc]), ilen(np.clip(n - t0, 0, Tc))
        hx, cx = h.clone(), None if gru else c.clone()                 # the backward of this chunk needs what its forward started from
        rnn.forward_state_varlen(xc, Wd, nc, h_n=h, hx=h, cx=c, c_n=c)  # carried in place
        chunks.append((rnn, xc, nc, hx, cx, t0, Tc, host(rnn.layer_output())))
        t0 += Tc
    y = np.concatenate([ch[-1] for ch in chunks], 1)
    dh = dev(dhn)
    dc = None if gru else dev(dcn)
    dx = np.zeros((B, T, F))
    Gsum = [np.zeros_like(P[k]) for k in names]
    for rnn, xc, nc, hx, cx, t0, Tc, _ in reversed(chunks):
        Gd = [torch.full_like(w, NAN) for w in Wd]
        dxd, dhx = nans(B, Tc, F), nans(Lyr, B, H)
        dcx = None if gru else nans(Lyr, B, H)
        rnn.backward_state_varlen(xc, Wd, Gd, nc, dy=dev(dy[:, t0:t0 + Tc]), dh_n=dh, dx=dxd, hx=hx, cx=cx, dc_n=dc, dhx=dhx, dcx=dcx)
        dx[:, t0:t0 + Tc] = host(dxd)
        for i, g in enumerate(Gd):
            Gsum[i] += host(g)
        dh, dc = dhx, dcx
    outs = [('y', y, ref['y'])] + [(f'h_n[{i}]', host(h)[i], ref['h_n'][i]) for i in range(Lyr)]
    gr = [(k, g, ref['G'][k]) for k, g in zip(names, Gsum)] + [('dx', dx, ref['dx'])] + [(f'dhx[{i}]', host(dh)[i], ref['dhx'][i]) for i in range(Lyr)]
    if not gru:
        outs += [(f'c_n[{i}]', host(c)[i], ref['c_n'][i]) for i in range(Lyr)]
        gr += [(f'dcx[{i}]', host(dc)[i], ref['dcx'][i]) for i in range(Lyr)]
    compare('V-E', f'{cell} H={H} impl={impl}', outs, gr)


# ----------------------------------------------------------------------------- V-F. the ragged stream
def oracle_rows(sd, x, totals, cfg, variant):
    """The oracle run row by row on x[b:b+1, :n_b] (rows with n_b > 0): {b: (out, z)}."""
    from oracle import ref_numpy as R
    Pm = R.to_f64({k: v for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'})
    res = {}
    for b, nb in enumerate(totals):
        if nb > 0:
            out, cache = R.audio_forward(Pm, x[b:b + 1, :nb].astype(np.float64), {'rnn_layers': cfg['rnn_layers']}, variant)
            res[b] = (out[0], cache['z'][0])
    return res


def stream_ragged(model, x, totals, cuts, device_push):
    s = model.stream()
    t0 = 0
    for i, Tc in enumerate(cuts):
        chunk, nc = x[:, t0:t0 + Tc], np.clip(np.asarray(totals) - t0, 0, Tc).astype(np.int32)
        if i == device_push:
            s.push(torch.from_numpy(chunk).to(DEV), torch.from_numpy(nc).to(DEV))
        else:
            s.push(chunk, nc)
        t0 += Tc
    return s.output()


def check_stream(variant, H, B, totals, cuts, F=12, seed=0):
    model, sd, cfg = make_audio(variant, F, H, seed=seed)
    T = sum(cuts)
    x = np.random.default_rng(H + B).standard_normal((B, T, F)).astype(np.float32)
    for b in range(B):
        x[b, totals[b]:] = 0.0
    model.eval()
    got = stream_ragged(model, x, totals, cuts, device_push=1)
    whole = model(x, lengths=np.asarray(totals, dtype=np.int32))
    gz, go, wz, wo = host(got._z), host(got.data), host(whole._z), host(whole.data)
    rows = oracle_rows(sd, x, totals, cfg, variant)
    ez = [float(np.abs(gz - wz).max()), max(float(np.abs(gz[b] - z).max()) for b, (_, z) in rows.items())]
    eo = [float(np.abs(go - wo).max()), max(float(np.abs(go[b] - o).max()) for b, (o, _) in rows.items())]
    print(f'rnn-state V-F {variant} H={H}: z vs model {ez[0]:.3e} vs oracle rows {ez[1]:.3e}; out vs model {eo[0]:.3e} vs oracle rows {eo[1]:.3e}')
    assert np.isfinite(gz).all() and np.isfinite(go).all()
    assert max(ez) < ATOL and max(eo) < ATOL
    for b in np.nonzero(np.asarray(totals) == 0)[0]:                    # a recording without frames: the whole ragged call's row
        assert np.array_equal(gz[b], wz[b]) and np.array_equal(go[b], wo[b]), b


@pytest.mark.parametrize('H', [32, 48])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_ragged_stream_equals_whole_and_oracle(variant, H):
    check_stream(variant, H, 5, [7, 0, 1, 5, 3], (1, 4, 2), seed=21 + H)


def test_ragged_stream_at_h256_equals_oracle():
    check_stream('clf', 256, 3, [4, 0, 2], (1, 2, 1), seed=5)


def test_ragged_stream_refusals():
    model, _, _ = make_audio('clf', 12, 32, seed=3)
    model.eval()
    chunk = np.zeros((5, 2, 12), np.float32)
    s = model.stream()
    with pytest.raises(L.DepError, match='lengths'):
        s.push(chunk, np.array([2, 1, 0, 2], np.int32))                        # four values for five recordings
    s = model.stream()
    with pytest.raises(L.DepError, match='lengths'):
        s.push(chunk, np.array([2.0, 1.0, 0.0, 2.0, 1.0], np.float32))         # not integers
    s = model.stream()
    with pytest.raises(L.DepError, match='lengths'):
        s.push(chunk, torch.zeros(5, dtype=torch.int64, device=DEV))           # a device vector is read in place: int32 only
    s = model.stream()
    s.push(chunk, np.array([2, 1, 0, 2, 1], np.int32))
    with pytest.raises(L.DepError, match='lengths'):
        s.push(chunk)                                                          # lengths on every push or on none
    s = model.stream()
    s.push(chunk)
    with pytest.raises(L.DepError, match='lengths'):
        s.push(chunk, np.array([2, 1, 0, 2, 1], np.int32))


# ----------------------------------------------------------------------------- V-G. the binding's own refusal
def test_state_varlen_methods_require_lengths():
    B, T, F, H, Lyr = 4, 3, 8, 16, 2
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, Lyr, 1, True, 0.0, L.POOL_MEAN, DEV, impl=2)
    P, names = make_params(np.random.default_rng(0), 'gru', F, H, Lyr, 1)
    Wd = [dev(P[n]) for n in names]
    xd = dev(np.zeros((B, T, F)))
    hx = torch.zeros(Lyr, B, H, device=DEV)
    with pytest.raises(L.DepError, match='lengths'):
        rnn.forward_state_varlen(xd, Wd, None, h_n=hx, hx=hx)
    with pytest.raises(L.DepError, match='lengths'):
        rnn.backward_state_varlen(xd, Wd, [torch.empty_like(w) for w in Wd], None, dh_n=hx, hx=hx)
