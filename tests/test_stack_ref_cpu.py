"""The yardstick of tests/test_stack_depth_gpu.py, and the reserve layout at every depth -- no GPU needed.

tests/stack_ref.py (a composition of the unchanged oracle's layer functions for any cell / dirs / L) against stock torch.nn.GRU /
torch.nn.LSTM in float64 with autograd: unidirectional GRU, unidirectional LSTM and bidirectional LSTM at L = 1, 3, 5, dense and
ragged (a per-row loop over nn.* on x[b:b+1, :len_b]), with each gradient input alone: dy, dh_n (non-zero in every layer and
direction) and, for the GRU, the gradient of a mean and of a sum pool.  Both sides are float64 evaluations of the same formulas:
1e-10 absolute.  At L = 2 the builder must give exactly what the oracle's own gru_stack_* / bilstm_stack_* give.
The size queries of the built library: the y / dropout(y) offsets of an L-layer stack for L = 1 .. 8."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_numpy as R
from stack_ref import stack, stack_bwd, stack_fwd

NONE = C.c_size_t(-1).value
TOL = 1e-10
STACKS = [('gru', 1), ('lstm', 1), ('lstm', 2)]


def _params(rng, cell, dirs, F, H, L):
    G = 3 if cell == 'gru' else 4
    P = {}
    for l in range(L):
        for d in range(dirs):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else dirs * H
            for nm, shp in (('weight_ih', (G * H, inp)), ('weight_hh', (G * H, H)), ('bias_ih', (G * H,)), ('bias_hh', (G * H,))):
                P[f'rnn.{nm}_{sfx}'] = rng.uniform(-0.4, 0.4, shp)
    return P


def _torch_run(torch, mod, x, lengths, pool, grad):
    """Outputs and, for the one gradient input `grad` = (kind, array), dx and the weight gradients of stock torch: the whole batch at
    once (lengths None) or row by row on x[b:b+1, :len_b], gradients summed over rows, dead positions and empty rows 0."""
    B, T, F = x.shape
    lstm = isinstance(mod, torch.nn.LSTM)
    D = 2 if mod.bidirectional else 1
    H, Ly = mod.hidden_size, mod.num_layers
    out = dict(y=np.zeros((B, T, D * H)), pooled=np.zeros((B, D * H)), h_n=np.zeros((Ly * D, B, H)), dx=np.zeros((B, T, F)),
               G={n: np.zeros(tuple(p.shape)) for n, p in mod.named_parameters()})
    blocks = [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), int(lengths[b])) for b in range(B)]
    params = [p for _, p in mod.named_parameters()]
    for rows, n in blocks:
        if n == 0:
            continue
        xt = torch.from_numpy(np.ascontiguousarray(x[rows, :n])).requires_grad_(True)
        yt, hid = mod(xt)
        hid = hid[0] if lstm else hid
        out['y'][rows, :n] = yt.detach().numpy(); out['h_n'][:, rows] = hid.detach().numpy()
        pt = None
        if pool != 'none':
            pt = yt.mean(1) if pool == 'mean' else yt.sum(1)
            out['pooled'][rows] = pt.detach().numpy()
        kind, g = grad
        if kind == 'dy':
            loss = (yt * torch.from_numpy(np.ascontiguousarray(g[rows, :n]))).sum()
        elif kind == 'dhn':
            loss = (hid * torch.from_numpy(np.ascontiguousarray(g[:, rows]))).sum()
        else:
            loss = (pt * torch.from_numpy(np.ascontiguousarray(g[rows]))).sum()
        grads = torch.autograd.grad(loss, [xt] + params, allow_unused=True)
        out['dx'][rows, :n] = grads[0].numpy()
        for (nm, _), gp in zip(mod.named_parameters(), grads[1:]):
            if gp is not None:
                out['G'][nm] += gp.numpy()
    return out


@pytest.mark.parametrize('form', ['dense', 'ragged'])
@pytest.mark.parametrize('L', [1, 3, 5])
@pytest.mark.parametrize('cell,dirs', STACKS)
def test_stack_builder_equals_torch(cell, dirs, L, form):
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(100 * L + 10 * dirs + (cell == 'gru'))
    B, T, F, H = 6, 7, 5, 4
    lengths = np.array([7, 1, 0, 4, 7, 2], dtype=np.int32) if form == 'ragged' else None
    P = _params(rng, cell, dirs, F, H, L)
    x = rng.standard_normal((B, T, F))
    mod = (torch.nn.GRU if cell == 'gru' else torch.nn.LSTM)(F, H, num_layers=L, batch_first=True, bidirectional=dirs == 2).double()
    with torch.no_grad():
        for k, v in P.items():
            getattr(mod, k.split('.', 1)[1]).copy_(torch.from_numpy(v))
    dhn = rng.standard_normal((L * dirs, B, H))
    assert all(np.abs(dhn[i]).min() > 0 for i in range(L * dirs))              # non-zero in every layer and direction
    grads = [('none', 'dy', rng.standard_normal((B, T, dirs * H))), ('none', 'dhn', dhn)]
    if cell == 'gru':
        grads += [('mean', 'dpooled', rng.standard_normal((B, H))), ('sum', 'dpooled', rng.standard_normal((B, H)))]
    for pool, kind, g in grads:
        want = _torch_run(torch, mod, x, lengths, pool, (kind, g))
        got = stack(x, P, 'rnn', cell, dirs, L, lengths=lengths, pool=pool, **{kind: g})
        tag = f'{kind} {pool}'
        assert np.abs(got['y'] - want['y']).max() < TOL, tag
        assert np.abs(got['ys'][L - 1] - want['y']).max() < TOL, tag
        assert np.abs(got['h_n'] - want['h_n']).max() < TOL, tag
        assert np.abs(got['pooled'] - want['pooled']).max() < TOL, tag
        assert np.abs(got['dx'] - want['dx']).max() < TOL, tag
        assert np.abs(want['dx']).max() > 1e-6, tag                            # the gradient input reached the bottom of the stack
        assert len(got['G']) == 4 * L * dirs
        for k, gv in got['G'].items():
            assert np.abs(gv - want['G'][k.split('.', 1)[1]]).max() < TOL, (tag, k)
        if lengths is not None:
            dead = np.arange(T)[None, :] >= lengths[:, None]
            assert not got['y'][dead].any() and not got['dx'][dead].any()
            assert not got['h_n'][:, lengths == 0].any() and not got['pooled'][lengths == 0].any()
            for yl in got['ys']:
                assert not yl[dead].any()


def test_lower_layer_outputs_are_the_shallower_stacks_top():
    """ys[l] of an L-layer stack is the top output of the (l+1)-layer stack over the same weights (what torch would return for it)."""
    rng = np.random.default_rng(9)
    for cell, dirs in STACKS:
        P = _params(rng, cell, dirs, 5, 4, 3)
        x = rng.standard_normal((3, 6, 5))
        full = stack(x, P, 'rnn', cell, dirs, 3)
        for l in range(3):
            assert np.array_equal(full['ys'][l], stack(x, P, 'rnn', cell, dirs, l + 1)['y']), (cell, dirs, l)


@pytest.mark.parametrize('masked', [False, True])
def test_at_two_layers_the_builder_is_the_oracles_stack(masked):
    """Exactly (np.array_equal): the new builder cannot drift from R.gru_stack_* / R.bilstm_stack_*, the yardstick of the other tests."""
    rng = np.random.default_rng(3)
    B, T, F, H = 4, 6, 5, 4
    x = rng.standard_normal((B, T, F))
    # unidirectional GRU: the oracle's BPTT has no dh_n entry
    P = _params(rng, 'gru', 1, F, H, 2)
    masks = [(rng.random((B, T, H)) < 0.5) * 2.0] if masked else None
    dy = rng.standard_normal((B, T, H))
    y_o, c_o = R.gru_stack_fwd(x, P, 'rnn', 2, masks)
    dx_o, G_o = R.gru_stack_bwd(dy, P, 'rnn', 2, c_o, masks)
    r = stack(x, P, 'rnn', 'gru', 1, 2, dy=dy, masks=masks)
    assert np.array_equal(r['y'], y_o) and np.array_equal(r['dx'], dx_o)
    assert np.array_equal(r['h_n'], np.stack([c_o[0][1][:, -1], c_o[1][1][:, -1]]))
    assert np.array_equal(r['ys'][0], c_o[0][1])
    assert set(r['G']) == set(G_o)
    for k in G_o:
        assert np.array_equal(r['G'][k], G_o[k]), k
    # bidirectional LSTM
    P = _params(rng, 'lstm', 2, F, H, 2)
    masks = [(rng.random((B, T, 2 * H)) < 0.5) * 2.0] if masked else None
    dy = rng.standard_normal((B, T, 2 * H)); dhn = rng.standard_normal((4, B, H))
    y_o, hn_o, c_o = R.bilstm_stack_fwd(x, P, 'rnn', 2, masks)
    dx_o, G_o = R.bilstm_stack_bwd(dy, dhn, P, 'rnn', 2, c_o, masks)
    y, hn, caches, ys = stack_fwd(x, P, 'rnn', 'lstm', 2, 2, masks)
    dx, G = stack_bwd(dy, dhn, P, 'rnn', 'lstm', 2, 2, caches, masks)
    r = stack(x, P, 'rnn', 'lstm', 2, 2, dy=dy, dhn=dhn, masks=masks)
    for a, b, c in ((y, r['y'], y_o), (hn, r['h_n'], hn_o), (dx, r['dx'], dx_o)):
        assert np.array_equal(a, c) and np.array_equal(b, c)
    assert set(r['G']) == set(G_o)
    for k in G_o:
        assert np.array_equal(G[k], G_o[k]) and np.array_equal(r['G'][k], G_o[k]), k


# ----------------------------------------------------------------------------- the reserve layout at every depth
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()                                   # (no-op when the library is current)
    from icassp2022_depression_amd import _lib
    return _lib, _lib.load()


@pytest.mark.parametrize('impl', [0, 1])
@pytest.mark.parametrize('cell,dirs', STACKS)
def test_layer_offsets_at_every_depth(lib, cell, dirs, impl):
    """DEP_RUN_TRAIN with p > 0: every layer's y and every lower layer's dropout(y) is its own array inside the reserve."""
    _lib, so = lib
    B, T, F, H = 20, 7, 12, 128
    n = B * T * H * dirs * 4
    c = _lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM
    pool = _lib.POOL_MEAN if cell == 'gru' else _lib.POOL_NONE
    for Ly in range(1, 9):
        d = _lib.RnnDesc(c, B, T, F, H, Ly, dirs, _lib.RUN_TRAIN, 0.5, 0, pool, impl)
        rb, wb = so.dep_rnn_reserve_bytes(C.byref(d)), so.dep_rnn_workspace_bytes(C.byref(d))
        assert rb > 0 and wb > 0, Ly
        ys = [so.dep_rnn_reserve_y_offset(C.byref(d), l) for l in range(Ly)]
        yd = [so.dep_rnn_reserve_ydrop_offset(C.byref(d), l) for l in range(Ly - 1)]
        for seq in (ys, yd):
            assert all(o != NONE and o % 16 == 0 and o + n <= rb for o in seq), (Ly, seq, rb)
            assert all(b - a >= n for a, b in zip(seq, seq[1:])), (Ly, seq)       # strictly increasing, a whole array apart
        spans = sorted((o, o + n) for o in ys + yd)
        assert all(b[0] >= a[1] for a, b in zip(spans, spans[1:])), (Ly, spans)   # and y / dropout(y) do not overlap each other
        assert so.dep_rnn_reserve_ydrop_offset(C.byref(d), Ly - 1) == NONE
        assert so.dep_rnn_reserve_y_offset(C.byref(d), Ly) == NONE and so.dep_rnn_reserve_y_offset(C.byref(d), -1) == NONE
    for Ly in (0, 9):
        d = _lib.RnnDesc(c, B, T, F, H, Ly, dirs, _lib.RUN_TRAIN, 0.5, 0, pool, impl)
        assert so.dep_rnn_reserve_bytes(C.byref(d)) == 0 and so.dep_rnn_workspace_bytes(C.byref(d)) == 0, Ly
        assert so.dep_rnn_reserve_y_offset(C.byref(d), 0) == NONE
