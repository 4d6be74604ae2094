"""GPU parity of the recurrent state in and out (dep_rnn_forward_state / dep_rnn_backward_state): hx / cx coming in, c_n going out,
dhx / dcx out and dc_n in, on the per-layer tile-MFMA and generic sweeps; and the streamed AudioGRU built on it.

The expectation for a non-zero state is tests/hx_ref.py (float64 numpy, pinned against stock torch in tests/test_rnn_state_cpu.py);
chunked-equals-whole is held against tests/stack_ref.py on the WHOLE sequence, the composition of the unchanged oracle.  Bars are the
project's (tests/test_stack_depth_gpu.py): 1e-4 absolute on every layer's output, y, pooled, h_n, c_n; 1e-4 relerr on dx, every
gradient tensor, dhx, dcx.  Both parity GEMM modes.  Outputs, gradients and the reserve are pre-filled with NaN.
Every check prints its worst figures ('rnn-state <section> ...'; pytest -s shows them).
Run on the MI355X box:  python -m pytest tests/test_rnn_state_gpu.py -m gpu -q"""
import ctypes as C
import re

import numpy as np
import pytest

import hx_ref
from stack_ref import stack as oracle_stack

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

ATOL = 1e-4
RTOL = 1e-4
PREFIX = 'rnn'
NAN = float('nan')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def make_params(rng, cell, F, H, Lyr, dirs):
    G = 3 if cell == 'gru' else 4
    P = {}; names = []
    k = 1.0 / np.sqrt(H)
    for l in range(Lyr):
        for d in range(dirs):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else H * dirs
            for nm, shp in (('weight_ih', (G * H, inp)), ('weight_hh', (G * H, H)), ('bias_ih', (G * H,)), ('bias_hh', (G * H,))):
                key = f'{PREFIX}.{nm}_{sfx}'
                P[key] = f32(rng.uniform(-k, k, shp))
                names.append(key)
    return P, names


@pytest.fixture(params=['f32', 'bf16x3'])
def gemm_mode(request):
    """Both precision modes of the parity path (forced on every contraction size), as in tests/test_stack_depth_gpu.py."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


def sweep_instances(log):
    return {re.sub(r'^\(|\)$', '', re.sub(r' @ .*$', '', s)) for s in log if re.search(r'(gru|lstm)2?_(fwd|bwd)_', s)}


STATE_SWEEP = r'(gru|lstm)_(fwd|bwd)_(mfma|generic)<.*>'


def case_rng(*v):
    return np.random.default_rng(sum(int(a) * 7 ** i for i, a in enumerate(v)))


ident = lambda c: '-'.join(str(v) for v in c)


def make_rnn(cell, dirs, B, T, F, H, Lyr, impl, p=0.0, training=True):
    gru = cell == 'gru'
    rnn = L.Rnn(L.CELL_GRU if gru else L.CELL_LSTM, B, T, F, H, Lyr, dirs, training, p, L.POOL_MEAN if gru else L.POOL_NONE, DEV, impl=impl)
    rnn.reserve.fill_(NAN)
    return rnn


def worst(e):
    return max(e, key=lambda v: float('inf') if v[0] != v[0] else v[0])


def compare(section, what, outs, grads):
    """outs / grads: lists of (name, device value as float64, reference).  The worst figures are printed before any assertion."""
    ea = [(float(np.abs(a - b).max()) if np.isfinite(a).all() else NAN, n) for n, a, b in outs]
    er = [(float(relerr(a, b)) if np.isfinite(a).all() else NAN, n) for n, a, b in grads]
    print(f'rnn-state {section} {what}:' + (f' worst abs {worst(ea)[0]:.3e} ({worst(ea)[1]})' if ea else '') +
          (f' worst rel {worst(er)[0]:.3e} ({worst(er)[1]})' if er else ''))
    for e, n in ea:
        assert e < ATOL, f'{n}: {e:.3e}'
    for (e, n), (_, _, b) in zip(er, grads):
        assert np.abs(b).max() > 0, f'{n}: the reference gradient is trivially zero'
        assert e < RTOL, f'{n}: {e:.3e}'


def run_state(cell, dirs, B, T, F, H, Lyr, impl, rng, grads, p=0.0, seed=0):
    """One forward + backward with a state that is non-zero in every layer and direction.  grads: which of dy / dpooled (GRU) /
    dhn / dcn (LSTM) go in.  Returns the (outs, grads) lists for compare() and the sweep instances the two calls logged."""
    gru = cell == 'gru'
    W = H * dirs
    K = Lyr * dirs
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    x = f32(rng.standard_normal((B, T, F)))
    hx = f32(rng.standard_normal((K, B, H)) * 0.6)
    cx = None if gru else f32(rng.standard_normal((K, B, H)) * 0.6)
    Wd = [dev(P[n]) for n in names]
    Gd = [torch.full_like(w, NAN) for w in Wd]
    xd, hxd, cxd = dev(x), dev(hx), None if gru else dev(cx)
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl, p)
    assert rnn.status_word() is None                                   # no cluster exchange buffer: the sweeps of rnn_sweep.hip run the stack
    pooled = nans(B, W) if gru else None
    h_n = nans(K, B, H)
    c_n = None if gru else nans(K, B, H)
    before = L.instance_log_read()
    rnn.forward(xd, Wd, seed=seed, pooled=pooled, h_n=h_n, hx=hxd, cx=cxd, c_n=c_n)
    masks = None
    if p > 0:
        masks = [host(L.dropout_mask(B * T * W, p, seed, 16 + l, DEV)).reshape(B, T, W) for l in range(Lyr - 1)]      # site = DEP_SITE_RNN0 + l
    dy = f32(rng.standard_normal((B, T, W)) * 0.3) if 'dy' in grads else None
    dpool = f32(rng.standard_normal((B, W))) if 'dpooled' in grads else None
    dhn = f32(rng.standard_normal((K, B, H)) * 0.3) if 'dhn' in grads else None
    dcn = f32(rng.standard_normal((K, B, H)) * 0.3) if 'dcn' in grads else None
    dxd, dhxd = nans(B, T, F), nans(K, B, H)
    dcxd = None if gru else nans(K, B, H)
    opt = lambda a: None if a is None else dev(a)
    rnn.backward(xd, Wd, Gd, dy=opt(dy), dpooled=opt(dpool), dh_n=opt(dhn), dx=dxd, hx=hxd, cx=cxd, dc_n=opt(dcn), dhx=dhxd, dcx=dcxd)
    rnn.check()
    inst = sweep_instances(L.instance_log_read() - before)
    ref = hx_ref.stack(x, P, PREFIX, cell, dirs, Lyr, hx=hx, cx=cx, pool='mean' if gru else 'none', dy=dy, dpooled=dpool, dhn=dhn, dcn=dcn,
                       masks=masks)
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
    return outs, gr, inst, masks


# ----------------------------------------------------------------------------- A. parity against hx_ref
# (cell, dirs, B, T, F, H, L, impl).  B = 19: two tiles, rows past B in the last one.  T = 1: only sweep step 0 exists, the state's
# dW_hh term is all of dW_hh.  T = 2 and 5: both LDS planes as the last one written.  H = 16 / 48 / 256: one wave; three tiles per
# wave; eight waves with two tiles each (T = 2).  H = 20 with impl = 1: the generic kernels.  L = 1 and 3: the per-layer offsets.
# dirs = 2: the reverse direction's t0 = T-1 (GRU: tile only).
PARITY_CASES = [
    ('gru', 1, 19, 5, 12, 48, 3, 2), ('gru', 2, 19, 5, 12, 16, 3, 2), ('gru', 2, 19, 1, 12, 48, 1, 2), ('gru', 1, 19, 2, 12, 16, 1, 2),
    ('gru', 2, 19, 2, 8, 256, 1, 2), ('gru', 1, 5, 5, 7, 20, 3, 1), ('gru', 1, 4, 1, 7, 20, 1, 1), ('gru', 1, 4, 2, 7, 20, 1, 1),
    ('lstm', 1, 19, 5, 12, 48, 3, 2), ('lstm', 2, 19, 5, 12, 16, 3, 2), ('lstm', 2, 19, 1, 12, 48, 1, 2), ('lstm', 1, 19, 2, 12, 16, 1, 2),
    ('lstm', 2, 19, 2, 8, 256, 1, 2), ('lstm', 2, 5, 5, 7, 20, 3, 1), ('lstm', 2, 4, 1, 7, 20, 1, 1), ('lstm', 1, 4, 2, 7, 20, 1, 1),
]


def all_grads(cell):
    return ('dy', 'dpooled', 'dhn') if cell == 'gru' else ('dy', 'dhn', 'dcn')


def check_sweeps(inst, cell, impl):
    kind = 'generic' if impl == 1 else 'mfma'
    assert inst and all(re.fullmatch(rf'{cell}_(fwd|bwd)_{kind}<.*>', s) for s in inst), sorted(inst)
    assert {re.search(r'_(fwd|bwd)_', s).group(1) for s in inst} == {'fwd', 'bwd'}, sorted(inst)


@pytest.mark.parametrize('case', PARITY_CASES, ids=ident)
def test_state_parity_all_gradient_inputs(case, gemm_mode):
    cell, dirs, B, T, F, H, Lyr, impl = case
    outs, gr, inst, _ = run_state(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, B, T, F, H, Lyr, impl), all_grads(cell))
    compare('A', ident(case), outs, gr)
    check_sweeps(inst, cell, impl)


ALONE_CASES = [('gru', 2, 19, 5, 12, 16, 3, 2), ('gru', 1, 5, 5, 7, 20, 3, 1), ('lstm', 2, 19, 5, 12, 16, 3, 2), ('lstm', 2, 5, 5, 7, 20, 3, 1)]


@pytest.mark.parametrize('which', [0, 1, 2])
@pytest.mark.parametrize('case', ALONE_CASES, ids=ident)
def test_state_parity_each_gradient_input_alone(case, which, gemm_mode):
    """dy, dpooled (GRU) / dc_n (LSTM) and dh_n each alone: an input treated as absent, or one that only works beside another, shows."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    g = all_grads(cell)[which]
    outs, gr, _, _ = run_state(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, B, T, F, H, which), (g,))
    compare('A', ident(case) + ' ' + g + ' alone', outs, gr)


@pytest.mark.parametrize('case', [('gru', 2, 19, 5, 12, 16, 2, 2), ('lstm', 2, 19, 5, 12, 16, 2, 2), ('gru', 1, 5, 5, 7, 20, 2, 1)], ids=ident)
def test_state_parity_with_dropout_masks(case, gemm_mode):
    """L = 2, p = 0.5: the mask site is unaffected by the state; the reference is fed the mask dep_dropout_mask draws for it."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    outs, gr, _, masks = run_state(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, B, T, F, H, 5), all_grads(cell), p=0.5, seed=4321)
    assert len(masks) == 1 and set(np.unique(masks[0])).issubset({0.0, 2.0}) and 0.3 < (masks[0] == 0).mean() < 0.7
    compare('A', ident(case) + ' p=0.5', outs, gr)


# ----------------------------------------------------------------------------- B. chunked equals whole, against the unchanged oracle
@pytest.mark.parametrize('H,impl', [(48, 2), (20, 1)])
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_chunked_equals_whole_against_the_oracle(cell, H, impl, gemm_mode):
    """T = 7 cut as (1, 4, 2): the forward carries the state, the backward walks the chunks in reverse order with each chunk's dhx / dcx
    as the previous chunk's dh_n / dc_n.  y and dx concatenated, the final h_n and the weight gradients summed over the chunks equal
    the whole call's -- exact BPTT across a chunk boundary."""
    gru = cell == 'gru'
    B, T, F, Lyr, cuts = 19, 7, 12, 2, (1, 4, 2)
    rng = case_rng(H, impl, 3 if gru else 4)
    P, names = make_params(rng, cell, F, H, Lyr, 1)
    x = f32(rng.standard_normal((B, T, F)))
    dy = f32(rng.standard_normal((B, T, H)) * 0.3)
    dhn = f32(rng.standard_normal((Lyr, B, H)) * 0.3)
    ref = oracle_stack(x, P, PREFIX, cell, 1, Lyr, dy=dy, dhn=dhn)
    Wd = [dev(P[n]) for n in names]
    h = torch.zeros(Lyr, B, H, device=DEV)
    c = None if gru else torch.zeros(Lyr, B, H, device=DEV)
    chunks = []
    t0 = 0
    for Tc in cuts:
        rnn = make_rnn(cell, 1, B, Tc, F, H, Lyr, impl)
        xc = dev(x[:, t0:t0 + Tc])
        hx, cx = h.clone(), None if gru else c.clone()                 # the backward of this chunk needs what its forward started from
        rnn.forward(xc, Wd, h_n=h, hx=h, cx=c, c_n=c)                  # carried in place
        chunks.append((rnn, xc, hx, cx, t0, Tc, host(rnn.layer_output())))
        t0 += Tc
    y = np.concatenate([ch[-1] for ch in chunks], 1)
    dh = dev(dhn)
    dc = None
    dx = np.zeros((B, T, F))
    Gsum = [np.zeros_like(P[n]) for n in names]
    for rnn, xc, hx, cx, t0, Tc, _ in reversed(chunks):
        Gd = [torch.full_like(w, NAN) for w in Wd]
        dxd, dhx = nans(B, Tc, F), nans(Lyr, B, H)
        dcx = None if gru else nans(Lyr, B, H)
        rnn.backward(xc, Wd, Gd, dy=dev(dy[:, t0:t0 + Tc]), dh_n=dh, dx=dxd, hx=hx, cx=cx, dc_n=dc, dhx=dhx, dcx=dcx)
        dx[:, t0:t0 + Tc] = host(dxd)
        for i, g in enumerate(Gd):
            Gsum[i] += host(g)
        dh, dc = dhx, dcx
    compare('B', f'{cell} H={H} impl={impl}', [('y', y, ref['y'])] + [(f'h_n[{i}]', host(h)[i], ref['h_n'][i]) for i in range(Lyr)],
            [(n, g, ref['G'][n]) for n, g in zip(names, Gsum)] + [('dx', dx, ref['dx'])])


# ----------------------------------------------------------------------------- C. no state is the plain call
def raw_forward(rnn, x, Wd, st, y=None, pooled=None, h_n=None, seed=0):
    """dep_rnn_forward_state called directly: st is None (NULL) or an L.RnnState."""
    for i, w in enumerate(Wd):
        rnn._warr[i] = w.data_ptr()
    rnn.desc.seed = seed
    p = lambda t: None if t is None else t.data_ptr()
    L.check(rnn.lib.dep_rnn_forward_state(C.byref(rnn.desc), p(x), rnn._warr, p(y), p(pooled), p(h_n), None if st is None else C.byref(st),
                                          p(rnn.reserve), rnn.reserve.numel() * 4, p(rnn.workspace), rnn.workspace.numel() * 4, L.stream()),
            'dep_rnn_forward_state')


def raw_backward(rnn, x, Wd, Gd, st, dy=None, dpooled=None, dh_n=None, dx=None):
    for i, (w, g) in enumerate(zip(Wd, Gd)):
        rnn._warr[i] = w.data_ptr(); rnn._garr[i] = g.data_ptr()
    p = lambda t: None if t is None else t.data_ptr()
    L.check(rnn.lib.dep_rnn_backward_state(C.byref(rnn.desc), p(x), rnn._warr, p(dy), p(dpooled), p(dh_n), None if st is None else C.byref(st),
                                           rnn._garr, p(dx), p(rnn.reserve), rnn.reserve.numel() * 4, p(rnn.workspace),
                                           rnn.workspace.numel() * 4, L.stream(), None), 'dep_rnn_backward_state')


PLAIN_CASES = [('gru', 1, 19, 5, 12, 48, 2, 2), ('gru', 1, 5, 5, 7, 20, 2, 1), ('lstm', 2, 19, 5, 12, 32, 2, 2), ('lstm', 2, 5, 5, 7, 20, 2, 1),
               ('gru', 1, 20, 6, 12, 128, 2, 3)]       # the last one: a cluster descriptor, where only the call without state is accepted


@pytest.mark.parametrize('case', PLAIN_CASES, ids=ident)
def test_no_state_is_the_plain_call(case, gemm_mode):
    """st = NULL and a struct of NULLs give the bits of dep_rnn_forward / dep_rnn_backward; a zero-filled hx (cx) gives the plain
    call's forward bits, and its gradients stay within the bars."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    gru = cell == 'gru'
    W, K = H * dirs, Lyr * dirs
    rng = case_rng(dirs, B, T, F, H, impl)
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    x = f32(rng.standard_normal((B, T, F)))
    dy = f32(rng.standard_normal((B, T, W)) * 0.3)
    dpool = f32(rng.standard_normal((B, W)))
    dhn = f32(rng.standard_normal((K, B, H)) * 0.3)
    Wd = [dev(P[n]) for n in names]
    xd, dyd, dhnd = dev(x), dev(dy), dev(dhn)
    dpd = dev(dpool) if gru else None
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl)

    def run(fwd, bwd):
        rnn.reserve.fill_(NAN)
        y, pooled, h_n = nans(B, T, W), nans(B, W) if gru else None, nans(K, B, H)
        Gd = [torch.full_like(w, NAN) for w in Wd]
        dx = nans(B, T, F)
        fwd(y, pooled, h_n)
        bwd(Gd, dx)
        rnn.check()
        return [('y', y), ('pooled', pooled), ('h_n', h_n), ('dx', dx)] + list(zip(names, Gd))

    plain = run(lambda y, pooled, h_n: rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, y=y),
                lambda Gd, dx: rnn.backward(xd, Wd, Gd, dy=dyd, dpooled=dpd, dh_n=dhnd, dx=dx))
    variants = [('st = NULL', None, None), ('a struct of NULLs', L.RnnState(None, None, None), L.RnnStateGrad(None, None, None, None, None))]
    for what, sf, sb in variants:
        got = run(lambda y, pooled, h_n: raw_forward(rnn, xd, Wd, sf, y=y, pooled=pooled, h_n=h_n),
                  lambda Gd, dx: raw_backward(rnn, xd, Wd, Gd, sb, dy=dyd, dpooled=dpd, dh_n=dhnd, dx=dx))
        for (n, a), (_, b) in zip(plain, got):
            if a is not None:
                assert torch.isfinite(a).all(), n
                assert np.array_equal(bits(a), bits(b)), f'{what}: {n} differs from the plain call'
    if impl == 3:
        return
    zh = torch.zeros(K, B, H, device=DEV)
    zc = None if gru else torch.zeros(K, B, H, device=DEV)
    dhx = nans(K, B, H)
    got = run(lambda y, pooled, h_n: rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, y=y, hx=zh, cx=zc),
              lambda Gd, dx: rnn.backward(xd, Wd, Gd, dy=dyd, dpooled=dpd, dh_n=dhnd, dx=dx, hx=zh, cx=zc, dhx=dhx))
    for (n, a), (_, b) in zip(plain[:3], got[:3]):
        if a is not None:
            assert np.array_equal(bits(a), bits(b)), f'a zero-filled hx: {n} differs from the plain call'
    ref = oracle_stack(x, P, PREFIX, cell, dirs, Lyr, pool='mean' if gru else 'none', dy=dy, dpooled=dpool if gru else None, dhn=dhn)
    compare('C', ident(case) + ' zero hx', [], [(n, host(g), ref['G'][n] if n in ref['G'] else ref['dx']) for n, g in got[3:]])
    assert torch.isfinite(dhx).all()


# ----------------------------------------------------------------------------- D. h_n aliasing hx, c_n aliasing cx
@pytest.mark.parametrize('case', [('gru', 2, 19, 5, 12, 48, 3, 2), ('gru', 1, 5, 5, 7, 20, 3, 1), ('lstm', 2, 19, 5, 12, 16, 3, 2),
                                  ('lstm', 2, 5, 5, 7, 20, 3, 1)], ids=ident)
def test_h_n_may_alias_hx(case):
    cell, dirs, B, T, F, H, Lyr, impl = case
    gru = cell == 'gru'
    K = Lyr * dirs
    rng = case_rng(dirs, B, T, F, H, 9)
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    hx = dev(rng.standard_normal((K, B, H)) * 0.6)
    cx = None if gru else dev(rng.standard_normal((K, B, H)) * 0.6)
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl)
    h_n, c_n = nans(K, B, H), None if gru else nans(K, B, H)
    rnn.forward(xd, Wd, h_n=h_n, hx=hx, cx=cx, c_n=c_n)
    y = rnn.layer_output().clone()
    rnn.reserve.fill_(NAN)
    h2, c2 = hx.clone(), None if gru else cx.clone()
    rnn.forward(xd, Wd, h_n=h2, hx=h2, cx=c2, c_n=c2)
    assert torch.isfinite(h_n).all() and not torch.equal(h_n, hx)
    assert np.array_equal(bits(y), bits(rnn.layer_output())), 'y'
    assert np.array_equal(bits(h_n), bits(h2)), 'h_n written over hx'
    if not gru:
        assert torch.isfinite(c_n).all() and np.array_equal(bits(c_n), bits(c2)), 'c_n written over cx'


# ----------------------------------------------------------------------------- E. the launch-instance log
@pytest.mark.parametrize('case', [('gru', 1, 19, 5, 12, 48, 2, 2), ('gru', 2, 19, 5, 12, 16, 2, 2), ('gru', 1, 5, 5, 7, 20, 2, 1),
                                  ('lstm', 2, 19, 5, 12, 16, 2, 2), ('lstm', 2, 5, 5, 7, 20, 2, 1)], ids=ident)
def test_a_state_call_launches_the_plain_calls_instances(case):
    """A state call launches only (gru|lstm)_(fwd|bwd)_(mfma|generic) sweeps, and the set of sweep instances it logs is the set the
    same descriptor's plain call logs: no instance was added."""
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
    rnn = make_rnn(cell, dirs, B, T, F, H, Lyr, impl)
    h_n, dx = nans(K, B, H), nans(B, T, F)
    L.instance_log_read(reset=True)
    rnn.forward(xd, Wd, h_n=h_n, hx=hx, cx=cx, c_n=None if gru else nans(K, B, H))
    rnn.backward(xd, Wd, Gd, dy=dyd, dx=dx, hx=hx, cx=cx, dhx=nans(K, B, H), dcx=None if gru else nans(K, B, H))
    torch.cuda.synchronize()
    with_state = L.instance_log_read(reset=True)
    rnn.forward(xd, Wd, h_n=h_n)
    rnn.backward(xd, Wd, Gd, dy=dyd, dx=dx)
    torch.cuda.synchronize()
    plain = L.instance_log_read()
    sw = sweep_instances(with_state)
    assert sw and all(re.fullmatch(STATE_SWEEP, s) for s in sw), sorted(sw)
    assert sw == sweep_instances(plain), (sorted(sw), sorted(sweep_instances(plain)))


# ----------------------------------------------------------------------------- F. the streamed AudioGRU
def make_audio(variant, F, H, seed):
    from icassp2022_depression_amd import audio_bilstm_perm, audio_gru_whole
    mod = audio_gru_whole if variant == 'clf' else audio_bilstm_perm
    cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0)
    model = mod.AudioBiLSTM(cfg, seed=seed)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    if variant == 'clf':                                               # a LayerNorm affine that is not the identity
        rng = np.random.default_rng(seed)
        sd['ln.weight'] = (1.0 + 0.3 * rng.standard_normal(F)).astype(np.float32)
        sd['ln.bias'] = (0.2 * rng.standard_normal(F)).astype(np.float32)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return model, sd, cfg


def oracle_audio(sd, x, cfg, variant):
    from oracle import ref_numpy as R
    P = R.to_f64({k: v for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'})
    out, cache = R.audio_forward(P, x.astype(np.float64), {'rnn_layers': cfg['rnn_layers']}, variant)
    return out, cache['z']


@pytest.mark.parametrize('H', [32, 48])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_stream_equals_whole_and_oracle(variant, H):
    B, F, cuts = 5, 12, (1, 4, 2)
    model, sd, cfg = make_audio(variant, F, H, seed=21 + H)
    x = np.random.default_rng(H).standard_normal((B, sum(cuts), F)).astype(np.float32)
    model.eval()
    s = model.stream()
    t0 = 0
    for i, Tc in enumerate(cuts):
        chunk = x[:, t0:t0 + Tc]
        s.push(torch.from_numpy(chunk).to(DEV) if i == 1 else chunk)    # host or device
        t0 += Tc
    got = s.output()
    whole = model(x)
    o, z = oracle_audio(sd, x, cfg, variant)
    ez = [float(np.abs(host(got._z) - host(whole._z)).max()), float(np.abs(host(got._z) - z).max())]
    eo = [float(np.abs(host(got.data) - host(whole.data)).max()), float(np.abs(host(got.data) - o).max())]
    print(f'rnn-state F {variant} H={H}: z vs model {ez[0]:.3e} vs oracle {ez[1]:.3e}; out vs model {eo[0]:.3e} vs oracle {eo[1]:.3e}')
    assert max(ez) < ATOL and max(eo) < ATOL


def test_stream_at_h256_equals_oracle():
    B, T, F, H = 3, 4, 12, 256
    model, sd, cfg = make_audio('clf', F, H, seed=5)
    x = np.random.default_rng(256).standard_normal((B, T, F)).astype(np.float32)
    model.eval()
    s = model.stream()
    for t0, t1 in ((0, 1), (1, 3), (3, 4)):
        s.push(x[:, t0:t1])
    got = s.output()
    o, z = oracle_audio(sd, x, cfg, 'clf')
    ez, eo = float(np.abs(host(got._z) - z).max()), float(np.abs(host(got.data) - o).max())
    print(f'rnn-state F clf H=256: z vs oracle {ez:.3e}; out vs oracle {eo:.3e}')
    assert ez < ATOL and eo < ATOL


def test_stream_refusals():
    model, _, _ = make_audio('clf', 12, 32, seed=3)
    model.train()
    with pytest.raises(L.DepError, match='eval'):
        model.stream()
    model.eval()
    s = model.stream()
    s.push(np.zeros((5, 2, 12), np.float32))
    with pytest.raises(L.DepError, match='batch size'):
        s.push(np.zeros((4, 2, 12), np.float32))


# ----------------------------------------------------------------------------- G. refusals of the binding (made before any launch)
def test_rnn_forward_refuses_state_on_a_cluster_descriptor_and_with_lengths():
    B, T, F, H, Lyr = 4, 3, 8, 256, 2
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, Lyr, 1, False, 0.0, L.POOL_MEAN, DEV, impl=0)
    assert rnn.status_word() is not None                               # a cluster descriptor
    P, names = make_params(np.random.default_rng(0), 'gru', F, H, Lyr, 1)
    Wd = [dev(P[n]) for n in names]
    xd = dev(np.zeros((B, T, F)))
    hx = torch.zeros(Lyr, B, H, device=DEV)
    with pytest.raises(L.DepError, match='cluster exchange buffer'):
        rnn.forward(xd, Wd, h_n=hx, hx=hx)
    tile = L.Rnn(L.CELL_GRU, B, T, F, 16, Lyr, 1, False, 0.0, L.POOL_MEAN, DEV, impl=2)
    P, names = make_params(np.random.default_rng(0), 'gru', F, 16, Lyr, 1)
    Wd = [dev(P[n]) for n in names]
    hx = torch.zeros(Lyr, B, 16, device=DEV)
    lengths = torch.full((B,), T, dtype=torch.int32, device=DEV)
    with pytest.raises(L.DepError, match='lengths'):
        tile.forward(xd, Wd, h_n=hx, hx=hx, lengths=lengths)
    with pytest.raises(L.DepError, match='lengths'):
        tile.backward(xd, Wd, [torch.empty_like(w) for w in Wd], dh_n=hx, hx=hx, lengths=lengths)
