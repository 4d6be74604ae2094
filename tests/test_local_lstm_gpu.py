"""GPU parity of impl = 8, the exchange-free per-layer LSTM forward: lstm_fwd_local<SPLIT, RAG> (csrc/rnn_local_lstm.hip) runs every
forward, one workgroup per (direction, 16-utterance tile), with the recurrent state going in (hx, cx) and out (h_n, c_n).

The expectation is tests/hx_ref.py (dense) and tests/state_varlen_ref.py (lengths), both float64.  Tolerance is the project's own for
every recurrent path: 1e-4 absolute on y / h_n / c_n / layer outputs, in both parity modes (GEMM modes 0 and 1, forced on every
contraction size): the exact instances in mode 0, the three-term split instances in mode 1.  Outputs are pre-filled with NaN; every
test asserts from the enqueue-order log that the only forward sweep launched was the expected lstm_fwd_local instance.
Run on the MI355X box:  python -m pytest tests/test_local_lstm_gpu.py -m gpu -q"""
import os
import re

import numpy as np
import pytest

import hx_ref
import state_varlen_ref as svr

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-4
PREFIX = 'lstm'
NAN = float('nan')
H = 128


def prefetch_depth():
    """Steps the kernel requests its input projection ahead (the register ring of lstm_fwd_local), read from its source."""
    src = open(os.path.join(ROOT, 'icassp2022-depression_amd', 'csrc', 'rnn_local_lstm.hip')).read()
    return int(re.search(r'constexpr int LL_PF = (\d+);', src).group(1))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def idev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


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


def pad_mask(lengths, T):
    return np.arange(T)[None, :] >= np.asarray(lengths)[:, None]


def make_params(rng, F, Lyr, dirs):
    """Weights in the order the header documents: l0 [, l0_reverse], l1, ...; layer l > 0 has weight_ih (4H, dirs*H)."""
    P = {}; names = []
    k = 1.0 / np.sqrt(H)
    for l in range(Lyr):
        for d in range(dirs):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else dirs * H
            for nm, shp in (('weight_ih', (4 * H, inp)), ('weight_hh', (4 * H, H)), ('bias_ih', (4 * H,)), ('bias_hh', (4 * H,))):
                key = f'{PREFIX}.{nm}_{sfx}'
                P[key] = f32(rng.uniform(-k, k, shp))
                names.append(key)
    return P, names


@pytest.fixture(params=['f32', 'bf16x3'])
def gemm_mode(request):
    """Both precision modes of the parity path (forced on every contraction size), as in tests/test_bigru_cluster_gpu.py."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


class launched:
    """The sweeps enqueued inside the block, from the enqueue-order log (the instance log is left alone: it keeps recording for
    tests/conftest.py)."""

    def __enter__(self):
        L.order_log_enable(True)
        L.order_log_read(reset=True)
        return self

    def __exit__(self, *exc):
        log = L.order_log_read(reset=True)
        L.order_log_enable(False)
        self.sweeps = [re.sub(r'^\(|\)$', '', e[2:]) for e in log if e.startswith('K ') and re.search(r'(gru|lstm)2?_(fwd|bwd)_', e)]


def case_rng(*v):
    return np.random.default_rng(800 + sum(int(a) * 7 ** i for i, a in enumerate(v)))


ident = lambda c: '-'.join(str(v) for v in c)


def make_rnn(B, T, F, Lyr, dirs, run=None, p=0.0, impl=8):
    run = L.RUN_EVAL if run is None else run
    rnn = L.Rnn(L.CELL_LSTM, B, T, F, H, Lyr, dirs, run, p, L.POOL_NONE, DEV, impl=impl)
    rnn.reserve.fill_(NAN)
    assert (rnn.status_word() is None) == (impl == 8)                  # impl = 8 has no exchange buffer
    return rnn


def check_instances(sweeps, Lyr, split, ragged):
    """One launch per layer of the lstm_fwd_local instance of this precision / raggedness, and no other sweep."""
    want = 'lstm_fwd_local<%s, %s>' % ('true' if split else 'false', 'true' if ragged else 'false')
    assert sweeps == [want] * Lyr, sweeps


def close(what, pairs, tol=ATOL):
    """pairs: (name, device value as float64, expectation).  Every figure is printed before any assertion."""
    errs = [(float(np.abs(a - b).max()) if np.isfinite(a).all() else NAN, n) for n, a, b in pairs]
    print(f'local-lstm {what}: ' + ', '.join(f'{n} {e:.2e}' for e, n in errs))
    for e, n in errs:
        assert e < tol, f'{what}: {n}: {e:.3e}'


def forward(rnn, xd, Wd, B, T, Lyr, dirs, lengths=None, hx=None, cx=None, want_c=False, seed=0):
    """One forward with every output NaN-filled; the sweeps it launched."""
    out = dict(h_n=nans(dirs * Lyr, B, H), y=nans(B, T, dirs * H))
    c_n = nans(dirs * Lyr, B, H) if (want_c or hx is not None or cx is not None) else None
    with launched() as k:
        if lengths is not None and c_n is not None:
            rnn.forward_state_varlen(xd, Wd, lengths, seed=seed, hx=hx, cx=cx, c_n=c_n, **out)
        else:
            rnn.forward(xd, Wd, seed=seed, lengths=lengths, hx=hx, cx=cx, c_n=c_n, **out)
    rnn.check()
    out['c_n'], out['sweeps'] = c_n, k.sweeps
    return out


def forward_pairs(out, rnn, ref, Lyr, layers=True):
    p = [('y', host(out['y']), ref['y']), ('h_n', host(out['h_n']), ref['h_n'])]
    if out['c_n'] is not None:
        p.append(('c_n', host(out['c_n']), ref['c_n']))
    if layers:
        p += [(f'layer {l} output', host(rnn.layer_output(l)), ref['ys'][l]) for l in range(Lyr)]
    return p


# ----------------------------------------------------------------------------- forward parity, dense
# (B, T, F, H, layers, dirs): one step, the zero initial fragment | exactly one full tile, unidirectional | a second tile with one live
# row, both LDS parities, layer 1 reading 2H-wide rows | every slot of the projection ring wraps, a middle layer | the workload's T:
# drift over 300 dependent steps | 34 tiles in one launch, past the cluster path's 512 chunk
def dense_cases():
    return [(3, 1, 8, H, 1, 2), (16, 5, 8, H, 1, 1), (17, 3, 12, H, 2, 2), (33, 2 * prefetch_depth() + 1, 8, H, 3, 2), (16, 300, 8, H, 1, 2),
            (530, 2, 8, H, 1, 2)]


@pytest.mark.parametrize('case', dense_cases(), ids=ident)
def test_dense_forward_parity(case, gemm_mode):
    B, T, F, _, Lyr, dirs = case
    rng = case_rng(*case)
    P, names = make_params(rng, F, Lyr, dirs)
    x = f32(rng.standard_normal((B, T, F)))
    ref = hx_ref.stack(x, P, PREFIX, 'lstm', dirs, Lyr)
    rnn = make_rnn(B, T, F, Lyr, dirs)
    out = forward(rnn, dev(x), [dev(P[n]) for n in names], B, T, Lyr, dirs, want_c=True)
    close(f'dense {ident(case)} {gemm_mode}', forward_pairs(out, rnn, ref, Lyr))
    check_instances(out['sweeps'], Lyr, gemm_mode == 'bf16x3', False)


# ----------------------------------------------------------------------------- ragged
def ragged_lengths(B, T, rng):
    """T, 1, and a tile whose rows differ as far as T < 16 allows: rows 0 .. 7 and rows 8 .. 15 each hold every length 0 .. T once, in
    a shuffled order; the second tile has a full row, a one-step row and an empty one."""
    assert T + 1 == 8
    first = np.concatenate([rng.permutation(T + 1), rng.permutation(T + 1)])
    lengths = np.concatenate([first, [T, 1, 0]])[:B]
    assert len(lengths) == B and (lengths == T).any() and (lengths == 1).any() and (lengths == 0).any()
    assert len(set(lengths[:8].tolist())) == 8 == len(set(lengths[8:16].tolist()))
    return lengths.astype(np.int64)


@pytest.mark.parametrize('dirs', [2, 1])
def test_ragged_forward_parity(dirs, gemm_mode):
    """live = t < len: the reverse direction of a row meets its dead steps first and carries its (zero) state through them; y and the
    layer outputs are exactly 0.0 at dead positions, h_n and c_n of an empty row are exactly 0.0."""
    B, T, F, Lyr = 19, 7, 8, 2
    rng = case_rng(B, T, F, dirs, 1)
    lengths = ragged_lengths(B, T, rng)
    P, names = make_params(rng, F, Lyr, dirs)
    x = f32(rng.standard_normal((B, T, F)))
    pad = pad_mask(lengths, T)
    x[pad] = 0.0
    ref = svr.stack(x, lengths, P, PREFIX, 'lstm', dirs, Lyr)
    rnn = make_rnn(B, T, F, Lyr, dirs)
    out = forward(rnn, dev(x), [dev(P[n]) for n in names], B, T, Lyr, dirs, lengths=idev(lengths), want_c=True)
    close(f'ragged dirs={dirs} {gemm_mode}', forward_pairs(out, rnn, ref, Lyr))
    check_instances(out['sweeps'], Lyr, gemm_mode == 'bf16x3', True)
    assert not bits(out['y'])[pad].any(), 'y is not exactly 0.0 at padded positions'
    assert not bits(rnn.layer_output(0))[pad].any(), 'layer 0 output is not exactly 0.0 at padded positions'
    assert not bits(out['h_n'])[:, lengths == 0].any() and not bits(out['c_n'])[:, lengths == 0].any(), 'the state of an empty row is not 0'


@pytest.mark.parametrize('dirs', [2, 1])
def test_all_lengths_T_gives_the_dense_calls_bits(dirs, gemm_mode):
    B, T, F, Lyr = 19, 7, 8, 2
    rng = case_rng(B, T, F, dirs, 2)
    P, names = make_params(rng, F, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    res = []
    for lengths in (None, idev(np.full(B, T))):
        rnn = make_rnn(B, T, F, Lyr, dirs)
        out = forward(rnn, xd, Wd, B, T, Lyr, dirs, lengths=lengths, want_c=True)
        check_instances(out['sweeps'], Lyr, gemm_mode == 'bf16x3', lengths is not None)
        res.append([out['y'], out['h_n'], out['c_n'], rnn.layer_output(0).clone()])
    for nm, a, b in zip(('y', 'h_n', 'c_n', 'layer 0 output'), *res):
        assert torch.isfinite(a).all(), nm
        assert torch.equal(a, b), nm


# ----------------------------------------------------------------------------- state
def state_masks(B, T, Lyr, dirs, p, seed):
    return [host(L.dropout_mask(B * T * dirs * H, p, seed, 16 + l, DEV)).reshape(B, T, dirs * H) for l in range(Lyr - 1)]      # site = DEP_SITE_RNN0 + l


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('run', ['eval', 'dropout_only'])
@pytest.mark.parametrize('dirs', [2, 1])
def test_forward_with_a_random_state(dirs, run, ragged, gemm_mode):
    """hx and cx in, h_n and c_n out: each (layer, direction) starts from its own slice, ordered like h_n (l * dirs + d).  A ragged row of
    length 0 returns its state bit for bit."""
    B, T, F, Lyr, p, seed = 5, 4, 8, 2, 0.5, 4321
    rng = case_rng(B, T, dirs, 3)
    P, names = make_params(rng, F, Lyr, dirs)
    x = f32(rng.standard_normal((B, T, F)))
    lengths = np.array([T, 0, 2, 1, 3]) if ragged else None
    if ragged:
        x[pad_mask(lengths, T)] = 0.0
    hx = f32(rng.standard_normal((dirs * Lyr, B, H)) * 0.6); cx = f32(rng.standard_normal((dirs * Lyr, B, H)) * 0.6)
    hxd, cxd = dev(hx), dev(cx)
    donly = run == 'dropout_only'
    rnn = make_rnn(B, T, F, Lyr, dirs, L.RUN_DROPOUT_ONLY if donly else L.RUN_EVAL, p=p if donly else 0.0)
    out = forward(rnn, dev(x), [dev(P[n]) for n in names], B, T, Lyr, dirs, lengths=None if lengths is None else idev(lengths), hx=hxd, cx=cxd, seed=seed)
    masks = state_masks(B, T, Lyr, dirs, p, seed) if donly else None
    if donly:
        assert 0.35 < (masks[0] == 0).mean() < 0.65
    if ragged:
        ref = svr.stack(x, lengths, P, PREFIX, 'lstm', dirs, Lyr, hx=hx, cx=cx, masks=masks)
        plain = svr.stack(x, lengths, P, PREFIX, 'lstm', dirs, Lyr, masks=masks)
    else:
        ref = hx_ref.stack(x, P, PREFIX, 'lstm', dirs, Lyr, hx=hx, cx=cx, masks=masks)
        plain = hx_ref.stack(x, P, PREFIX, 'lstm', dirs, Lyr, masks=masks)
    assert np.abs(ref['h_n'] - plain['h_n']).max() > 100 * ATOL and np.abs(ref['y'] - plain['y']).max() > 100 * ATOL      # the state matters
    close(f'state dirs={dirs} {run} {"ragged" if ragged else "dense"} {gemm_mode}', forward_pairs(out, rnn, ref, Lyr, layers=not donly))
    check_instances(out['sweeps'], Lyr, gemm_mode == 'bf16x3', ragged)
    if ragged:
        empty = lengths == 0
        assert np.array_equal(bits(out['h_n'])[:, empty], bits(hxd)[:, empty]), 'len 0: h_n is hx bit for bit'
        assert np.array_equal(bits(out['c_n'])[:, empty], bits(cxd)[:, empty]), 'len 0: c_n is cx bit for bit'
        assert not bits(out['y'])[pad_mask(lengths, T)].any()


def test_two_chained_calls_reproduce_one(gemm_mode):
    """T = 3 then T = 4, the state carried in place (h_n over hx, c_n over cx), against one call of T = 7 (unidirectional)."""
    B, F, Lyr, dirs, Ta, Tb = 5, 8, 2, 1, 3, 4
    rng = case_rng(B, Ta, Tb, 4)
    P, names = make_params(rng, F, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    x = f32(rng.standard_normal((B, Ta + Tb, F)))
    whole = forward(make_rnn(B, Ta + Tb, F, Lyr, dirs), dev(x), Wd, B, Ta + Tb, Lyr, dirs, want_c=True)
    h = torch.zeros(Lyr, B, H, device=DEV); c = torch.zeros(Lyr, B, H, device=DEV)
    ys = []
    for t0, Tc in ((0, Ta), (Ta, Tb)):
        rnn = make_rnn(B, Tc, F, Lyr, dirs)
        y = nans(B, Tc, H)
        with launched() as k:
            rnn.forward(dev(x[:, t0:t0 + Tc]), Wd, y=y, h_n=h, hx=h, cx=c, c_n=c)
        check_instances(k.sweeps, Lyr, gemm_mode == 'bf16x3', False)
        ys.append(host(y))
    ref = hx_ref.stack(x, P, PREFIX, 'lstm', dirs, Lyr)
    close(f'chained {gemm_mode} against the oracle', [('y', np.concatenate(ys, 1), ref['y']), ('h_n', host(h), ref['h_n']), ('c_n', host(c), ref['c_n'])])
    close(f'chained {gemm_mode} against one call', [('y', np.concatenate(ys, 1), host(whole['y'])), ('h_n', host(h), host(whole['h_n'])),
                                                    ('c_n', host(c), host(whole['c_n']))])


# ----------------------------------------------------------------------------- dropout-only
def test_dropout_only_masks_are_the_cluster_sweeps(gemm_mode):
    """p = 0.5, L = 2: the dropped positions of dropout(y0) are those of the same call on impl = 3, bit for bit; parity with the oracle
    on the device's masks."""
    B, T, F, Lyr, dirs, p, seed = 19, 5, 12, 2, 2, 0.5, 777
    rng = case_rng(B, T, F, 5)
    P, names = make_params(rng, F, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    x = f32(rng.standard_normal((B, T, F)))
    r8 = make_rnn(B, T, F, Lyr, dirs, L.RUN_DROPOUT_ONLY, p=p)
    o8 = forward(r8, dev(x), Wd, B, T, Lyr, dirs, seed=seed)
    check_instances(o8['sweeps'], Lyr, gemm_mode == 'bf16x3', False)
    r3 = make_rnn(B, T, F, Lyr, dirs, L.RUN_DROPOUT_ONLY, p=p, impl=3)
    y3, h3 = nans(B, T, dirs * H), nans(dirs * Lyr, B, H)
    r3.forward(dev(x), Wd, seed=seed, y=y3, h_n=h3)
    r3.check()
    z8, z3 = host(r8.layer_output_dropped(0)) == 0, host(r3.layer_output_dropped(0)) == 0
    assert 0.35 < z8.mean() < 0.65
    assert np.array_equal(z8, z3)
    masks = state_masks(B, T, Lyr, dirs, p, seed)
    assert set(np.unique(masks[0])).issubset({0.0, 2.0}) and np.array_equal(masks[0] == 0, z8)
    ref = hx_ref.stack(x, P, PREFIX, 'lstm', dirs, Lyr, masks=masks)
    close(f'dropout-only {gemm_mode}', [('y', host(o8['y']), ref['y']), ('h_n', host(o8['h_n']), ref['h_n']),
                                        ('dropout(y0)', host(r8.layer_output_dropped(0)), ref['ys'][0] * masks[0]),
                                        ('top layer output', host(r8.layer_output()), ref['y'])])
    close(f'dropout-only {gemm_mode} against impl = 3', [('y', host(o8['y']), host(y3)), ('h_n', host(o8['h_n']), host(h3))])


# ----------------------------------------------------------------------------- agreement with the shipped path
def test_agrees_with_the_cluster_sweep(gemm_mode):
    B, T, F, Lyr, dirs = 70, 9, 64, 2, 2
    rng = case_rng(B, T, F, 6)
    P, names = make_params(rng, F, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    o8 = forward(make_rnn(B, T, F, Lyr, dirs), xd, Wd, B, T, Lyr, dirs)
    check_instances(o8['sweeps'], Lyr, gemm_mode == 'bf16x3', False)
    r3 = make_rnn(B, T, F, Lyr, dirs, impl=3)
    y3, h3 = nans(B, T, dirs * H), nans(dirs * Lyr, B, H)
    with launched() as k:
        r3.forward(xd, Wd, y=y3, h_n=h3)
    r3.check()
    assert k.sweeps and all(s.startswith('lstm_fwd_cluster<') for s in k.sweeps), k.sweeps
    close(f'against impl = 3 {gemm_mode}', [('y', host(o8['y']), host(y3)), ('h_n', host(o8['h_n']), host(h3))])


# ----------------------------------------------------------------------------- independence
def test_two_streams_give_the_bits_of_two_calls_in_turn(gemm_mode):
    """Two forwards on two streams, each with its own Rnn (workspace and reserve): nothing is shared, so what runs beside a sweep
    cannot change its result.  One run, no repetition."""
    B, T, F, Lyr, dirs = 40, 6, 16, 2, 2
    rng = case_rng(B, T, F, 7)
    P, names = make_params(rng, F, Lyr, dirs)
    Wd = [dev(P[n]) for n in names]
    xs = [dev(rng.standard_normal((B, T, F))) for _ in range(2)]
    rnns = [make_rnn(B, T, F, Lyr, dirs) for _ in range(2)]

    def run(i, outs):
        rnns[i].reserve.fill_(NAN)
        outs[i] = dict(y=nans(B, T, dirs * H), h_n=nans(dirs * Lyr, B, H), c_n=nans(dirs * Lyr, B, H))
        rnns[i].forward(xs[i], Wd, **outs[i])

    turn = [None, None]
    with launched() as k:
        for i in range(2):
            run(i, turn)
            torch.cuda.synchronize()
    check_instances(k.sweeps, 2 * Lyr, gemm_mode == 'bf16x3', False)
    turn = [{n: bits(v) for n, v in o.items()} for o in turn]
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    side = [None, None]
    for i in range(2):
        streams[i].wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(streams[i]):
            run(i, side)
    torch.cuda.synchronize()
    for i in range(2):
        rnns[i].check()
        for n, v in side[i].items():
            assert np.isfinite(host(v)).all(), (i, n)
            assert np.array_equal(bits(v), turn[i][n]), (i, n)
