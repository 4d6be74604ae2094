"""GPU parity of impl = 4, the per-layer cluster sweeps, and of the recurrent state its forward takes (hx on gru_fwd_cluster_r1 in
DEP_RUN_EVAL / DEP_RUN_DROPOUT_ONLY), dense and ragged, and of the streamed AudioGRU on it.

The expectation for a non-zero state is tests/hx_ref.py (tests/state_varlen_ref.py for ragged calls); chunked-equals-whole and the plain
calls are held against tests/stack_ref.py, the composition of the unchanged oracle.  Bars are the project's
(tests/test_rnn_state_gpu.py): 1e-4 absolute on y, pooled, h_n; 1e-4 relerr on gradients.  Both parity GEMM modes: mode 0 launches the
exact-fp32 instances, mode 1 the split-precision (SPLIT) ones.  Outputs and the reserve are pre-filled with NaN.
Every check prints its worst figures ('state-cluster <section> ...'; pytest -s shows them).
Run on the MI355X box:  python -m pytest tests/test_state_cluster_gpu.py -m gpu -q"""
import ctypes as C
import re

import numpy as np
import pytest

import hx_ref
import state_varlen_ref as svr
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
FWD_CLUSTER = r'gru_fwd_cluster_r1<\d+, (true|false)(, true)?>'
BWD_CLUSTER = r'gru_bwd_cluster_r1<.*>'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def make_params(rng, F, H, Lyr):
    P = {}; names = []
    k = 1.0 / np.sqrt(H)
    for l in range(Lyr):
        inp = F if l == 0 else H
        for nm, shp in (('weight_ih', (3 * H, inp)), ('weight_hh', (3 * H, H)), ('bias_ih', (3 * H,)), ('bias_hh', (3 * H,))):
            key = f'{PREFIX}.{nm}_l{l}'
            P[key] = f32(rng.uniform(-k, k, shp))
            names.append(key)
    return P, names


@pytest.fixture(params=['f32', 'bf16x3'])
def gemm_mode(request):
    """Both precision modes of the parity path (forced on every contraction size), as in tests/test_rnn_state_gpu.py."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


def sweep_instances(log):
    return {re.sub(r'^\(|\)$', '', re.sub(r' @ .*$', '', s)) for s in log if re.search(r'(gru|lstm)2?_(fwd|bwd)_', s)}


def case_rng(*v):
    return np.random.default_rng(1000 + sum(int(a) * 7 ** i for i, a in enumerate(v)))


ident = lambda c: '-'.join(str(v) for v in c)
POOLS = {'mean': 1, 'sum': 2}          # DEP_POOL_*


def make_rnn(B, T, F, H, Lyr, run, p=0.0, pool='mean', impl=4):
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, Lyr, 1, run, p, POOLS[pool], DEV, impl=impl)
    rnn.reserve.fill_(NAN)
    assert rnn.status_word() is not None                               # a cluster descriptor
    return rnn


def worst(e):
    return max(e, key=lambda v: float('inf') if v[0] != v[0] else v[0])


def compare(section, what, outs, grads=()):
    """outs / grads: lists of (name, device value as float64, reference).  The worst figures are printed before any assertion."""
    ea = [(float(np.abs(a - b).max()) if np.isfinite(a).all() else NAN, n) for n, a, b in outs]
    er = [(float(relerr(a, b)) if np.isfinite(a).all() else NAN, n) for n, a, b in grads]
    print(f'state-cluster {section} {what}:' + (f' worst abs {worst(ea)[0]:.3e} ({worst(ea)[1]})' if ea else '') +
          (f' worst rel {worst(er)[0]:.3e} ({worst(er)[1]})' if er else ''))
    for e, n in ea:
        assert e < ATOL, f'{n}: {e:.3e}'
    for (e, n), (_, _, b) in zip(er, grads):
        assert np.abs(b).max() > 0, f'{n}: the reference gradient is trivially zero'
        assert e < RTOL, f'{n}: {e:.3e}'


def check_forward_instances(inst, H, split, ragged):
    """Only gru_fwd_cluster_r1 sweeps, and the instance of this H / precision / raggedness."""
    assert inst and all(re.fullmatch(FWD_CLUSTER, s) for s in inst), sorted(inst)
    want = 'gru_fwd_cluster_r1<%d, %s%s>' % (H // 32, 'true' if split else 'false', ', true' if ragged else '')
    assert inst == {want}, (sorted(inst), want)


# ----------------------------------------------------------------------------- A. dense parity with a random non-zero hx
# (H, L, B, T): two members | a second tile with one live row | no exchange at all | sixteen members, the largest LDS image
DENSE = [(64, 1, 3, 5), (256, 2, 17, 2), (128, 3, 5, 1), (512, 1, 3, 3)]


@pytest.mark.parametrize('case', DENSE, ids=ident)
def test_dense_parity_with_a_random_state(case, gemm_mode):
    H, Lyr, B, T = case
    F = 12
    rng = case_rng(H, Lyr, B, T)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    hx = f32(rng.standard_normal((Lyr, B, H)) * 0.6)
    Wd = [dev(P[n]) for n in names]
    xd, hxd = dev(x), dev(hx)
    for pool in ('mean', 'sum'):
        rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL, pool=pool)
        pooled, h_n, y = nans(B, H), nans(Lyr, B, H), nans(B, T, H)
        L.instance_log_read(reset=True)
        rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, y=y, hx=hxd)
        rnn.check()
        inst = sweep_instances(L.instance_log_read(reset=True))
        ref = hx_ref.stack(x, P, PREFIX, 'gru', 1, Lyr, hx=hx, pool=pool)
        outs = [(f'layer {l} output', host(rnn.layer_output(l)), yl) for l, yl in enumerate(ref['ys'])]
        outs += [('y', host(y), ref['y']), ('pooled', host(pooled), ref['pooled'])]
        outs += [(f'h_n[{i}]', host(h_n)[i], ref['h_n'][i]) for i in range(Lyr)]
        compare('A', f'{ident(case)} {gemm_mode} pool={pool}', outs)
        check_forward_instances(inst, H, gemm_mode == 'bf16x3', False)
        assert np.abs(ref['h_n'] - hx_ref.stack(x, P, PREFIX, 'gru', 1, Lyr)['h_n']).max() > 100 * ATOL      # the state matters to the result


def test_dropout_only_parity_with_masks(gemm_mode):
    H, Lyr, B, T, F, p, seed = 256, 2, 17, 4, 12, 0.5, 77
    rng = case_rng(H, Lyr, B, T, 5)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    hx = f32(rng.standard_normal((Lyr, B, H)) * 0.6)
    Wd = [dev(P[n]) for n in names]
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_DROPOUT_ONLY, p=p)
    pooled, h_n, y = nans(B, H), nans(Lyr, B, H), nans(B, T, H)
    rnn.forward(dev(x), Wd, seed=seed, pooled=pooled, h_n=h_n, y=y, hx=dev(hx))
    rnn.check()
    masks = [host(L.dropout_mask(B * T * H, p, seed, 16 + l, DEV)).reshape(B, T, H) for l in range(Lyr - 1)]      # site = DEP_SITE_RNN0 + l
    assert 0.3 < (masks[0] == 0).mean() < 0.7
    ref = hx_ref.stack(x, P, PREFIX, 'gru', 1, Lyr, hx=hx, pool='mean', masks=masks)
    compare('A', f'dropout-only {gemm_mode}', [('y', host(y), ref['y']), ('pooled', host(pooled), ref['pooled'])] +
            [(f'h_n[{i}]', host(h_n)[i], ref['h_n'][i]) for i in range(Lyr)])


# ----------------------------------------------------------------------------- B. ragged parity
def test_ragged_parity_with_a_random_state(gemm_mode):
    H, Lyr, B, T, F = 256, 2, 5, 4, 12
    lengths = np.array([0, 1, 4, 2, 4])
    rng = case_rng(H, Lyr, B, T, 3)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    for b in range(B):
        x[b, lengths[b]:] = 0.0
    hx = f32(rng.standard_normal((Lyr, B, H)) * 0.6)
    Wd = [dev(P[n]) for n in names]
    hxd = dev(hx)
    ld = torch.from_numpy(lengths.astype(np.int32)).to(DEV)
    for pool in ('mean', 'sum'):
        rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL, pool=pool)
        pooled, h_n, y = nans(B, H), nans(Lyr, B, H), nans(B, T, H)
        L.instance_log_read(reset=True)
        rnn.forward_state_varlen(dev(x), Wd, ld, pooled=pooled, h_n=h_n, y=y, hx=hxd)
        rnn.check()
        inst = sweep_instances(L.instance_log_read(reset=True))
        ref = svr.stack(x, lengths, P, PREFIX, 'gru', 1, Lyr, hx=hx, pool=pool)
        yh, ph, hh = host(y), host(pooled), host(h_n)
        compare('B', f'{gemm_mode} pool={pool}', [('y', yh, ref['y']), ('pooled', ph, ref['pooled'])] +
                [(f'h_n[{i}]', hh[i], ref['h_n'][i]) for i in range(Lyr)])
        check_forward_instances(inst, H, gemm_mode == 'bf16x3', True)
        assert np.array_equal(bits(h_n)[:, 0], bits(hxd)[:, 0]), 'len 0: h_n is hx bit for bit'
        assert not yh[0].any() and not ph[0].any(), 'len 0: y and pooled are exactly 0'
        for b in range(B):
            assert not yh[b, lengths[b]:].any(), f'row {b}: padded positions of y are exactly 0'
            for l in range(Lyr):
                assert not host(rnn.layer_output(l))[b, lengths[b]:].any(), (b, l)


# ----------------------------------------------------------------------------- C. h_n written over hx
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_h_n_may_alias_hx(T, ragged, gemm_mode):
    H, Lyr, B, F = 256, 2, 17, 12
    rng = case_rng(H, Lyr, B, T, 9)
    P, names = make_params(rng, F, H, Lyr)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    hx = dev(rng.standard_normal((Lyr, B, H)) * 0.6)
    ld = torch.from_numpy(rng.integers(0, T + 1, B).astype(np.int32)).to(DEV) if ragged else None
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL)

    def run(h_in, h_out, pooled):
        rnn.reserve.fill_(NAN)
        if ragged:
            rnn.forward_state_varlen(xd, Wd, ld, pooled=pooled, h_n=h_out, hx=h_in)
        else:
            rnn.forward(xd, Wd, pooled=pooled, h_n=h_out, hx=h_in)
        rnn.check()
        return rnn.layer_output().clone()

    h_n, p1 = nans(Lyr, B, H), nans(B, H)
    y1 = run(hx, h_n, p1)
    h2, p2 = hx.clone(), nans(B, H)
    y2 = run(h2, h2, p2)
    assert torch.isfinite(h_n).all() and not torch.equal(h_n, hx)
    assert np.array_equal(bits(y1), bits(y2)), 'y'
    assert np.array_equal(bits(p1), bits(p2)), 'pooled'
    assert np.array_equal(bits(h_n), bits(h2)), 'h_n written over hx'


# ----------------------------------------------------------------------------- D. chunks compose
@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_chunked_equals_whole_against_the_oracle(ragged, gemm_mode):
    """T = 7 cut as 1 + 4 + 2 with the state carried in place (the T = 1 chunk takes the staging copy).  Ragged: recording 1 ends inside
    the second chunk and pushes 0 afterwards, recording 2 has no frame at all."""
    H, Lyr, B, T, F, cuts = 128, 2, 3, 7, 12, (1, 4, 2)
    n = np.array([7, 3, 0]) if ragged else np.array([T] * B)
    rng = case_rng(H, Lyr, B, T, 4)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    for b in range(B):
        x[b, n[b]:] = 0.0
    ref = oracle_stack(x, P, PREFIX, 'gru', 1, Lyr, lengths=n if ragged else None)
    Wd = [dev(P[k]) for k in names]
    h = torch.zeros(Lyr, B, H, device=DEV)
    ys = []
    t0 = 0
    for Tc in cuts:
        rnn = make_rnn(B, Tc, F, H, Lyr, L.RUN_EVAL)
        xc = dev(x[:, t0:t0 + Tc])
        if ragged:
            nc = torch.from_numpy(np.clip(n - t0, 0, Tc).astype(np.int32)).to(DEV)
            rnn.forward_state_varlen(xc, Wd, nc, h_n=h, hx=h)
        else:
            rnn.forward(xc, Wd, h_n=h, hx=h)
        rnn.check()
        ys.append(host(rnn.layer_output()))
        t0 += Tc
    y = np.concatenate(ys, 1)
    compare('D', f'{"ragged" if ragged else "dense"} {gemm_mode}', [('y', y, ref['y'])] + [(f'h_n[{i}]', host(h)[i], ref['h_n'][i]) for i in range(Lyr)])
    for b in range(B):
        assert not y[b, n[b]:].any(), b


# ----------------------------------------------------------------------------- E. a batch beyond one co-resident launch
def test_batch_chunks_with_state(gemm_mode):
    """B = 517 at H = 256: eight members per tile, so a 256-CU device holds 32 tiles = 512 rows per launch and rows 512 .. 516 run in a
    second launch, which must index hx / h_n by the global row."""
    H, Lyr, B, T, F = 256, 1, 517, 2, 8
    rng = case_rng(H, Lyr, B, T)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    hx = f32(rng.standard_normal((Lyr, B, H)) * 0.6)
    Wd = [dev(P[n]) for n in names]
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL)
    pooled, h_n, y = nans(B, H), nans(Lyr, B, H), nans(B, T, H)
    rnn.forward(dev(x), Wd, pooled=pooled, h_n=h_n, y=y, hx=dev(hx))
    rnn.check()
    ref = hx_ref.stack(x, P, PREFIX, 'gru', 1, Lyr, hx=hx, pool='mean')
    yh, ph, hh = host(y), host(pooled), host(h_n)[0]
    for what, sl in (('first launch', slice(0, 512)), ('second launch', slice(512, B))):
        compare('E', f'{what} {gemm_mode}', [('y', yh[sl], ref['y'][sl]), ('pooled', ph[sl], ref['pooled'][sl]), ('h_n', hh[sl], ref['h_n'][0][sl])])


# ----------------------------------------------------------------------------- F. the plan, through the launch-instance log
def raw_forward(rnn, x, Wd, st, lengths=None, y=None, pooled=None, h_n=None, seed=0):
    """dep_rnn_forward_state[_varlen] called directly: st is None (NULL) or an L.RnnState."""
    for i, w in enumerate(Wd):
        rnn._warr[i] = w.data_ptr()
    rnn.desc.seed = seed
    p = lambda t: None if t is None else t.data_ptr()
    s = None if st is None else C.byref(st)
    tail = (p(rnn.reserve), rnn.reserve.numel() * 4, p(rnn.workspace), rnn.workspace.numel() * 4, L.stream())
    if lengths is None:
        L.check(rnn.lib.dep_rnn_forward_state(C.byref(rnn.desc), p(x), rnn._warr, p(y), p(pooled), p(h_n), s, *tail), 'dep_rnn_forward_state')
    else:
        L.check(rnn.lib.dep_rnn_forward_state_varlen(C.byref(rnn.desc), p(x), p(lengths), rnn._warr, p(y), p(pooled), p(h_n), s, *tail),
                'dep_rnn_forward_state_varlen')


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_forward_plan_and_null_state_is_the_plain_call(ragged, gemm_mode):
    """H = 256, L = 2, B = 64: the shape at which impl 0 / 3 take the fused two-layer forward (mode 1) or the 16-unit members."""
    H, Lyr, B, T, F = 256, 2, 64, 4, 12
    rng = case_rng(H, Lyr, B, T, 6)
    P, names = make_params(rng, F, H, Lyr)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    hx = dev(rng.standard_normal((Lyr, B, H)) * 0.6)
    ld = torch.from_numpy(rng.integers(0, T + 1, B).astype(np.int32)).to(DEV) if ragged else None
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL)

    def run(call):
        rnn.reserve.fill_(NAN)
        y, pooled, h_n = nans(B, T, H), nans(B, H), nans(Lyr, B, H)
        L.instance_log_read(reset=True)
        call(y, pooled, h_n)
        rnn.check()
        return [y, pooled, h_n], L.instance_log_read()

    plain, log_plain = run(lambda y, pooled, h_n: rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, y=y, lengths=ld))
    check_forward_instances(sweep_instances(log_plain), H, gemm_mode == 'bf16x3', ragged)
    for what, st in (('st = NULL', None), ('a struct of NULLs', L.RnnState(None, None, None))):
        got, log = run(lambda y, pooled, h_n: raw_forward(rnn, xd, Wd, st, lengths=ld, y=y, pooled=pooled, h_n=h_n))
        assert log == log_plain, (what, sorted(log ^ log_plain))
        for a, b in zip(plain, got):
            assert torch.isfinite(a).all() and np.array_equal(bits(a), bits(b)), what
    state, log = run(lambda y, pooled, h_n: raw_forward(rnn, xd, Wd, L.RnnState(hx.data_ptr(), None, None), lengths=ld, y=y, pooled=pooled, h_n=h_n))
    check_forward_instances(sweep_instances(log), H, gemm_mode == 'bf16x3', ragged)
    assert sweep_instances(log) == sweep_instances(log_plain)
    assert not torch.equal(state[2], plain[2])
    zero, _ = run(lambda y, pooled, h_n: raw_forward(rnn, xd, Wd, L.RnnState(torch.zeros_like(hx).data_ptr(), None, None), lengths=ld, y=y,
                                                     pooled=pooled, h_n=h_n))
    for a, b in zip(plain, zero):
        assert np.array_equal(bits(a), bits(b)), 'a zero-filled hx gives the plain call bits'


# (H, L, B, T): the fused backward's shape, T even (PK gate gradients) | one layer at H = 256, T odd | H = 128 | H = 512 (no burst streams)
TRAIN = [(256, 2, 17, 4), (256, 1, 5, 3), (128, 2, 3, 4), (512, 1, 3, 2)]


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('case', TRAIN, ids=ident)
def test_train_mode_runs_the_per_layer_plan_and_matches_the_oracle(case, ragged, gemm_mode):
    H, Lyr, B, T = case
    F = 12
    rng = case_rng(H, Lyr, B, T, 8)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    n = rng.integers(0, T + 1, B) if ragged else None
    if ragged:
        n[0] = T
        for b in range(B):
            x[b, n[b]:] = 0.0
    dy = f32(rng.standard_normal((B, T, H)) * 0.3)
    dpool = f32(rng.standard_normal((B, H)))
    dhn = f32(rng.standard_normal((Lyr, B, H)) * 0.3)
    Wd = [dev(P[k]) for k in names]
    Gd = [torch.full_like(w, NAN) for w in Wd]
    xd = dev(x)
    ld = None if n is None else torch.from_numpy(n.astype(np.int32)).to(DEV)
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_TRAIN)
    pooled, h_n, dx = nans(B, H), nans(Lyr, B, H), nans(B, T, F)
    L.instance_log_read(reset=True)
    rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, lengths=ld)
    rnn.backward(xd, Wd, Gd, dy=dev(dy), dpooled=dev(dpool), dh_n=dev(dhn), dx=dx, lengths=ld)
    rnn.check()
    inst = sweep_instances(L.instance_log_read())
    fwd_i, bwd_i = {s for s in inst if '_fwd_' in s}, {s for s in inst if '_bwd_' in s}
    check_forward_instances(fwd_i, H, gemm_mode == 'bf16x3', ragged)
    assert len(bwd_i) == 1 and all(re.fullmatch(BWD_CLUSTER, s) for s in bwd_i), sorted(bwd_i)
    ref = oracle_stack(x, P, PREFIX, 'gru', 1, Lyr, lengths=n, pool='mean', dy=dy, dpooled=dpool, dhn=dhn)
    outs = [(f'layer {l} output', host(rnn.layer_output(l)), yl) for l, yl in enumerate(ref['ys'])]
    outs += [('pooled', host(pooled), ref['pooled'])] + [(f'h_n[{i}]', host(h_n)[i], ref['h_n'][i]) for i in range(Lyr)]
    gr = []
    for l in range(Lyr - 1, -1, -1):
        gr += [(k, host(g), ref['G'][k]) for k, g in zip(names, Gd) if k.endswith(f'_l{l}')]
    gr.append(('dx', host(dx), ref['dx']))
    compare('F', f'{ident(case)} {"ragged" if ragged else "dense"} {gemm_mode}', outs, gr)


def test_state_refusals_through_the_binding():
    H, Lyr, B, T, F = 64, 1, 3, 2, 8
    P, names = make_params(np.random.default_rng(0), F, H, Lyr)
    Wd = [dev(P[n]) for n in names]
    xd, hx = dev(np.zeros((B, T, F))), torch.zeros(Lyr, B, H, device=DEV)
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_TRAIN)
    with pytest.raises(L.DepError, match='impl = 4'):
        rnn.forward(xd, Wd, h_n=hx, hx=hx)
    rnn.forward(xd, Wd)
    with pytest.raises(L.DepError, match='cluster backward takes no state'):
        rnn.backward(xd, Wd, [torch.empty_like(w) for w in Wd], dh_n=hx, dhx=torch.empty_like(hx))


# ----------------------------------------------------------------------------- G. the consumer: AudioGRU.stream()
def make_audio(F, H, seed):
    from icassp2022_depression_amd import audio_gru_whole
    cfg = dict(audio_gru_whole.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0)
    model = audio_gru_whole.AudioBiLSTM(cfg, seed=seed)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    rng = np.random.default_rng(seed)                                  # a LayerNorm affine that is not the identity
    sd['ln.weight'] = (1.0 + 0.3 * rng.standard_normal(F)).astype(np.float32)
    sd['ln.bias'] = (0.2 * rng.standard_normal(F)).astype(np.float32)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.eval()
    return model, sd, cfg


def oracle_audio(sd, x, cfg):
    from oracle import ref_numpy as R
    P = R.to_f64({k: v for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'})
    out, cache = R.audio_forward(P, x.astype(np.float64), {'rnn_layers': cfg['rnn_layers']}, 'clf')
    return out, cache['z']


def test_stream_at_h256_runs_the_cluster_sweeps_and_equals_the_oracle():
    """The inputs of tests/test_rnn_state_gpu.py::test_stream_at_h256_equals_oracle: pushes of 1, 2 and 1 steps."""
    B, T, F, H = 3, 4, 12, 256
    model, sd, cfg = make_audio(F, H, seed=5)
    x = np.random.default_rng(256).standard_normal((B, T, F)).astype(np.float32)
    s = model.stream()
    L.instance_log_read(reset=True)
    for t0, t1 in ((0, 1), (1, 3), (3, 4)):
        s.push(x[:, t0:t1])
    inst = sweep_instances(L.instance_log_read())
    got = s.output()
    s.check_health()
    o, z = oracle_audio(sd, x, cfg)
    ez, eo = float(np.abs(host(got._z) - z).max()), float(np.abs(host(got.data) - o).max())
    print(f'state-cluster G clf H=256: z vs oracle {ez:.3e}; out vs oracle {eo:.3e}')
    assert ez < ATOL and eo < ATOL
    assert inst and all(re.fullmatch(r'gru_fwd_cluster_r1<8, (true|false)>', i) for i in inst), sorted(inst)
    assert s.health is not None and float(s.health[1].item()) == 0


def test_ragged_stream_at_h256_runs_the_cluster_sweeps_and_equals_the_oracle():
    """The inputs of tests/test_state_varlen_gpu.py::test_ragged_stream_at_h256_equals_oracle."""
    from oracle import ref_numpy as R
    B, F, H, totals, cuts = 3, 12, 256, [4, 0, 2], (1, 2, 1)
    model, sd, cfg = make_audio(F, H, seed=5)
    x = np.random.default_rng(H + B).standard_normal((B, sum(cuts), F)).astype(np.float32)
    for b in range(B):
        x[b, totals[b]:] = 0.0
    s = model.stream()
    L.instance_log_read(reset=True)
    t0 = 0
    for Tc in cuts:
        s.push(x[:, t0:t0 + Tc], np.clip(np.asarray(totals) - t0, 0, Tc).astype(np.int32))
        t0 += Tc
    inst = sweep_instances(L.instance_log_read())
    got = s.output()
    s.check_health()
    gz, go = host(got._z), host(got.data)
    whole = model(x, lengths=np.asarray(totals, dtype=np.int32))
    Pm = R.to_f64({k: v for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'})
    ez = eo = 0.0
    for b, nb in enumerate(totals):
        if nb > 0:
            out, cache = R.audio_forward(Pm, x[b:b + 1, :nb].astype(np.float64), {'rnn_layers': cfg['rnn_layers']}, 'clf')
            ez, eo = max(ez, float(np.abs(gz[b] - cache['z'][0]).max())), max(eo, float(np.abs(go[b] - out[0]).max()))
        else:
            assert np.array_equal(gz[b], host(whole._z)[b]) and np.array_equal(go[b], host(whole.data)[b]), b
    print(f'state-cluster G ragged clf H=256: z vs oracle rows {ez:.3e}; out vs oracle rows {eo:.3e}')
    assert np.isfinite(gz).all() and ez < ATOL and eo < ATOL
    assert inst and all(re.fullmatch(r'gru_fwd_cluster_r1<8, (true|false), true>', i) for i in inst), sorted(inst)


def test_stream_at_h32_stays_on_the_tile_sweeps_and_impl_is_the_callers_choice():
    model, _, _ = make_audio(12, 32, seed=3)
    s = model.stream()
    L.instance_log_read(reset=True)
    s.push(np.zeros((5, 2, 12), np.float32))
    inst = sweep_instances(L.instance_log_read())
    assert inst and all(re.fullmatch(r'gru_fwd_mfma<.*>', i) for i in inst), sorted(inst)
    s.check_health()
    assert s.health is None                                            # no status word on the tile sweeps
    with pytest.raises(L.DepError, match='impl = 4'):
        model.stream(impl=L.IMPL_CLUSTER_PER_LAYER).push(np.zeros((5, 2, 12), np.float32))
    model256, _, _ = make_audio(12, 256, seed=3)
    s = model256.stream(impl=L.IMPL_TILE)
    L.instance_log_read(reset=True)
    s.push(np.zeros((3, 2, 12), np.float32))
    inst = sweep_instances(L.instance_log_read())
    assert inst and all(re.fullmatch(r'gru_fwd_mfma<.*>', i) for i in inst), sorted(inst)
