"""GPU parity of impl = 5, "the per-layer cluster sweeps, state through training": hx in a DEP_RUN_TRAIN forward, hx as h_prev of step 0
and dhx in gru_bwd_cluster_r1 (dense and ragged instances, burst or not, reduce-scatter and all-gather), the hx term of dW_hh and the
recurrent term of dhx the call adds behind the sweep.

Expectations: tests/hx_ref.py (dense) and tests/state_varlen_ref.py (ragged), unchanged; chunked-equals-whole against tests/stack_ref.py,
the composition of the unchanged oracle.  Bars are the file-level ones of tests/test_state_cluster_gpu.py: 1e-4 absolute on outputs, 1e-4
relerr on gradients, init-scale weights.  Both parity GEMM modes: mode 0 launches the exact-fp32 instances, mode 1 the split ones.
Outputs, gradients and the reserve are pre-filled with NaN; every case asserts a zero status word.
Every check prints its worst figures ('state-cluster-bwd <section> ...'; pytest -s shows them).
Run on the MI355X box:  python -m pytest tests/test_state_cluster_bwd_gpu.py -m gpu -q"""
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
POOLS = {'mean': 1, 'sum': 2}          # DEP_POOL_*


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
    """Both precision modes of the parity path (forced on every contraction size), as in tests/test_state_cluster_gpu.py."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


def sweep_instances(log):
    return {re.sub(r'^\(|\)$', '', re.sub(r' @ .*$', '', s)) for s in log if re.search(r'(gru|lstm)2?_(fwd|bwd)_', s)}


def case_rng(*v):
    return np.random.default_rng(2000 + sum(int(a) * 7 ** i for i, a in enumerate(v)))


def worst(e):
    return max(e, key=lambda v: float('inf') if v[0] != v[0] else v[0])


def compare(section, what, outs, grads=()):
    """outs / grads: lists of (name, device value as float64, reference).  The worst figures are printed before any assertion."""
    ea = [(float(np.abs(a - b).max()) if np.isfinite(a).all() else NAN, n) for n, a, b in outs]
    er = [(float(relerr(a, b)) if np.isfinite(a).all() else NAN, n) for n, a, b in grads]
    print(f'state-cluster-bwd {section} {what}:' + (f' worst abs {worst(ea)[0]:.3e} ({worst(ea)[1]})' if ea else '') +
          (f' worst rel {worst(er)[0]:.3e} ({worst(er)[1]})' if er else ''))
    for e, n in ea:
        assert e < ATOL, f'{n}: {e:.3e}'
    for (e, n), (_, _, b) in zip(er, grads):
        assert np.abs(b).max() > 0, f'{n}: the reference gradient is trivially zero'
        assert e < RTOL, f'{n}: {e:.3e}'


def make_rnn(B, T, F, H, Lyr, run=None, p=0.0, pool='mean', impl=5):
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, Lyr, 1, L.RUN_TRAIN if run is None else run, p, POOLS[pool], DEV, impl=impl)
    rnn.reserve.fill_(NAN)
    assert rnn.status_word() is not None                               # a cluster descriptor
    return rnn


def clean(rnn):
    rnn.check()
    assert int(rnn.status_word().item()) == 0


class Case:
    """One stack with random weights, input, state and gradient inputs; lengths: the ragged call (a numpy int vector) or None."""

    def __init__(self, rng, B, T, F, H, Lyr, lengths=None, p=0.0, seed=0, pool='mean', impl=5):
        self.B, self.T, self.F, self.H, self.Lyr, self.n, self.p, self.seed, self.pool = B, T, F, H, Lyr, lengths, p, seed, pool
        self.P, self.names = make_params(rng, F, H, Lyr)
        self.x = f32(rng.standard_normal((B, T, F)))
        if lengths is not None:
            for b in range(B):
                self.x[b, lengths[b]:] = 0.0
        self.hx = f32(rng.standard_normal((Lyr, B, H)))
        self.dy = f32(rng.standard_normal((B, T, H)) * 0.3)
        self.dpool = f32(rng.standard_normal((B, H)))
        self.dhn = f32(rng.standard_normal((Lyr, B, H)) * 0.3)
        self.Wd = [dev(self.P[k]) for k in self.names]
        self.xd, self.hxd = dev(self.x), dev(self.hx)
        self.ld = None if lengths is None else torch.from_numpy(np.asarray(lengths).astype(np.int32)).to(DEV)
        self.rnn = make_rnn(B, T, F, H, Lyr, p=p, pool=pool, impl=impl)
        self.masks = None
        if p > 0:
            self.masks = [host(L.dropout_mask(B * T * H, p, seed, 16 + l, DEV)).reshape(B, T, H) for l in range(Lyr - 1)]      # site = DEP_SITE_RNN0 + l

    def forward(self, hx='own'):
        hxd = self.hxd if isinstance(hx, str) else hx
        self.pooled, self.h_n = nans(self.B, self.H), nans(self.Lyr, self.B, self.H)
        self.rnn.reserve.fill_(NAN)
        if self.ld is not None:
            self.rnn.forward_state_varlen(self.xd, self.Wd, self.ld, seed=self.seed, pooled=self.pooled, h_n=self.h_n, hx=hxd)
        else:
            self.rnn.forward(self.xd, self.Wd, seed=self.seed, pooled=self.pooled, h_n=self.h_n, hx=hxd)

    def backward(self, dy=True, dhn=True, hx='own', dhx='new', dh_n_t=None):
        """Returns (weight gradients, dx, dhx)."""
        hxd = self.hxd if isinstance(hx, str) else hx
        Gd = [torch.full_like(w, NAN) for w in self.Wd]
        dx = nans(self.B, self.T, self.F)
        dhxd = nans(self.Lyr, self.B, self.H) if isinstance(dhx, str) else dhx
        dhnd = dh_n_t if dh_n_t is not None else (dev(self.dhn) if dhn else None)
        kw = dict(dy=dev(self.dy) if dy else None, dpooled=dev(self.dpool), dh_n=dhnd, dx=dx, hx=hxd, dhx=dhxd)
        if self.ld is not None:
            self.rnn.backward_state_varlen(self.xd, self.Wd, Gd, self.ld, **kw)
        else:
            self.rnn.backward(self.xd, self.Wd, Gd, **kw)
        clean(self.rnn)
        return Gd, dx, dhxd

    def ref(self, dy=True, dhn=True, hx=True):
        kw = dict(hx=self.hx if hx else None, pool=self.pool, dy=self.dy if dy else None, dpooled=self.dpool, dhn=self.dhn if dhn else None,
                  masks=self.masks)
        if self.n is not None:
            return svr.stack(self.x, self.n, self.P, PREFIX, 'gru', 1, self.Lyr, **kw)
        return hx_ref.stack(self.x, self.P, PREFIX, 'gru', 1, self.Lyr, **kw)

    def state_matters(self, dy=True, dhn=True):
        """What every case asserts first: with hx = 0 the reference's h_n (live rows) and dW_hh of layer 0 are clearly others."""
        ref, ref0 = self.ref(dy, dhn), self.ref(dy, dhn, hx=False)
        live = slice(None) if self.n is None else np.asarray(self.n) > 0
        assert np.abs(ref['h_n'][:, live] - ref0['h_n'][:, live]).max() > 100 * ATOL, 'the state matters to h_n'
        k = f'{PREFIX}.weight_hh_l0'
        assert relerr(ref['G'][k], ref0['G'][k]) > 100 * RTOL, 'the state matters to dW_hh'
        return ref

    def check(self, section, what, variants=((True, True), (True, False), (False, True))):
        """Forward once, one backward per (dy, dh_n) variant, each against the reference; first: the state matters to the result."""
        ref0 = self.ref(hx=False)
        self.forward()
        clean(self.rnn)
        for dy, dhn in variants:
            ref = self.ref(dy, dhn)
            live = slice(None) if self.n is None else np.asarray(self.n) > 0
            assert np.abs(ref['h_n'][:, live] - ref0['h_n'][:, live]).max() > 100 * ATOL, 'the state matters to h_n'
            k = f'{PREFIX}.weight_hh_l0'
            assert relerr(ref['G'][k], self.ref(dy, dhn, hx=False)['G'][k]) > 100 * RTOL, 'the state matters to dW_hh'
            Gd, dx, dhx = self.backward(dy, dhn)
            outs = [(f'layer {l} output', host(self.rnn.layer_output(l)), yl) for l, yl in enumerate(ref['ys'])]
            outs += [('pooled', host(self.pooled), ref['pooled'])] + [(f'h_n[{i}]', host(self.h_n)[i], ref['h_n'][i]) for i in range(self.Lyr)]
            gr = []
            for l in range(self.Lyr - 1, -1, -1):
                gr += [(k, host(g), ref['G'][k]) for k, g in zip(self.names, Gd) if k.endswith(f'_l{l}')]
            gr.append(('dx', host(dx), ref['dx']))
            gr += [(f'dhx[{i}]', host(dhx)[i], ref['dhx'][i]) for i in range(self.Lyr)]
            compare(section, f'{what} dy={int(dy)} dh_n={int(dhn)}', outs, gr)


# ----------------------------------------------------------------------------- A. dense parity of one forward + backward
# H: 64 two members | 128 four | 256 eight, the all-gather burst instance in mode 1 | 512 sixteen, no burst
# B = 17: a second tile with one live row.  T: no exchange (1), t = 0 inside the burst prologue (2 .. 4), just past it (5), across two
# dirty steps (9).
@pytest.mark.parametrize('B', [5, 17])
@pytest.mark.parametrize('H', [64, 128, 256, 512])
def test_dense_parity_with_a_random_state(H, B, gemm_mode):
    for Lyr in (1, 2, 3):
        for T in (1, 2, 3, 4, 5, 9):
            # the grid is kept to a few seconds per test: every (dy, dh_n) variant -- together and each alone -- at two layers (the depth
            # with a layer above and below the inter-layer gradient); depths 1 and 3 run both gradients together only
            variants = ((True, True), (True, False), (False, True)) if Lyr == 2 else ((True, True),)
            Case(case_rng(H, B, T, Lyr), B, T, 12, H, Lyr).check('A', f'H={H} B={B} T={T} L={Lyr} {gemm_mode}', variants)


@pytest.mark.parametrize('pool', ['mean', 'sum'])
def test_dropout_masks_and_both_pools(pool, gemm_mode):
    c = Case(case_rng(256, 17, 4, 2, 1), 17, 4, 12, 256, 2, p=0.5, seed=77, pool=pool)
    assert 0.3 < (c.masks[0] == 0).mean() < 0.7
    c.check('A', f'dropout 0.5 pool={pool} {gemm_mode}')
    c = Case(case_rng(64, 5, 5, 2, 2), 5, 5, 12, 64, 2, p=0.5, seed=78, pool=pool)
    c.check('A', f'dropout 0.5 H=64 pool={pool} {gemm_mode}', ((True, True),))


def test_all_four_burst_phases(gemm_mode):
    """26 tiles: phi = (tile / 8) % 4 = 0 .. 3, the t = 0 request is issued at a different point of the service waves' life in each."""
    B, T, F, H = 416, 6, 64, 256
    Case(case_rng(B, T, F, H), B, T, F, H, 1).check('B', f'{gemm_mode}', ((True, True),))


# ----------------------------------------------------------------------------- C. a shape whose plain call takes the PK image
def test_state_call_at_a_pk_shape(gemm_mode):
    B, T, F, H, Lyr = 40, 2, 256, 256, 2
    c = Case(case_rng(B, T, F, H, Lyr), B, T, F, H, Lyr)
    c.check('C', f'{gemm_mode}', ((True, True),))


def test_zero_state_call_gives_the_plain_calls_bits(gemm_mode):
    """hx all zero and dhx requested: fp32 gate-gradient rows and unpaired contractions against the plain call's plan (the PK image and
    the paired launch in mode 1) on the same descriptor -- every dW, db and dx bit for bit."""
    B, T, F, H, Lyr = 40, 2, 256, 256, 2
    c = Case(case_rng(B, T, F, H, Lyr, 1), B, T, F, H, Lyr)
    c.forward(hx=None)
    Gd = [torch.full_like(w, NAN) for w in c.Wd]
    dx = nans(B, T, F)
    L.instance_log_read(reset=True)
    c.rnn.backward(c.xd, c.Wd, Gd, dy=dev(c.dy), dpooled=dev(c.dpool), dh_n=dev(c.dhn), dx=dx)
    clean(c.rnn)
    log_plain = L.instance_log_read(reset=True)
    zero = torch.zeros(Lyr, B, H, device=DEV)
    c.forward(hx=zero)
    L.instance_log_read(reset=True)
    G2, dx2, dhx = c.backward(hx=zero)
    log_state = L.instance_log_read(reset=True)
    assert torch.isfinite(dhx).all() and torch.isfinite(dx).all()
    for k, a, b in zip(c.names, Gd, G2):
        assert torch.isfinite(a).all() and np.array_equal(bits(a), bits(b)), k
    assert np.array_equal(bits(dx), bits(dx2)), 'dx'
    assert sweep_instances(log_plain) == sweep_instances(log_state)
    # (the gate-gradient format is a run-time argument of the sweep and of the contractions: the instance log cannot tell the two plans apart)


# ----------------------------------------------------------------------------- D. ragged
# every vector: a full, an empty and a one-step row, and in every tile a row that ends inside the sequence
def ragged_lengths(B, T):
    n = np.array([T, 0, 1, max(T - 1, 0), max(T // 2, 1)] + [T] * (B - 5))
    if B > 16:
        n[16:] = [max(T - 2, 1), T, 0, 1][:B - 16]
    return n


RAGGED = [(64, 1, 5, 3), (128, 2, 5, 5), (256, 2, 20, 4), (256, 1, 20, 9), (512, 2, 5, 3)]


@pytest.mark.parametrize('case', RAGGED, ids=lambda c: '-'.join(map(str, c)))
def test_ragged_parity_and_the_pass_through(case, gemm_mode):
    H, Lyr, B, T = case
    n = ragged_lengths(B, T)
    c = Case(case_rng(H, Lyr, B, T, 3), B, T, 12, H, Lyr, lengths=n)
    c.check('D', f'{"-".join(map(str, case))} {gemm_mode}', ((True, True), (True, False), (False, True)))
    # an empty row: the state and its gradient pass through bit for bit (random inputs)
    dhn = dev(c.dhn)
    _, _, dhx = c.backward(dh_n_t=dhn)
    empty = np.flatnonzero(n == 0)
    assert len(empty)
    assert np.array_equal(bits(dhx)[:, empty], bits(dhn)[:, empty]), 'len 0: dhx is dh_n bit for bit'
    assert np.array_equal(bits(c.h_n)[:, empty], bits(c.hxd)[:, empty]), 'len 0: h_n is hx bit for bit'


@pytest.mark.parametrize('H', [64, 256, 512])
def test_ragged_with_full_lengths_is_the_dense_state_call(H, gemm_mode):
    B, T, Lyr = 17, 4, 2
    d = Case(case_rng(H, 1), B, T, 12, H, Lyr)
    r = Case(case_rng(H, 1), B, T, 12, H, Lyr, lengths=np.array([T] * B))
    d.forward(); r.forward()
    Gd, dxd, dhd = d.backward()
    Gr, dxr, dhr = r.backward()
    ref = d.ref()
    compare('D', f'full lengths H={H} {gemm_mode}', [('h_n', host(r.h_n), host(d.h_n)), ('pooled', host(r.pooled), host(d.pooled))],
            [(k, host(a), host(b)) for k, a, b in zip(d.names, Gr, Gd)] + [('dx', host(dxr), host(dxd)), ('dhx', host(dhr), host(dhd))])
    compare('D', f'full lengths vs oracle H={H} {gemm_mode}', [], [('dhx', host(dhr), ref['dhx']), ('dx', host(dxr), ref['dx'])])


# ----------------------------------------------------------------------------- E. dhx written over dh_n
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_dhx_may_alias_dh_n(T, ragged, gemm_mode):
    H, Lyr, B = 256, 2, 17
    rng = case_rng(H, Lyr, B, T, 9)
    n = rng.integers(0, T + 1, B) if ragged else None
    if ragged:
        n[:3] = (T, 0, 1)                                              # (a live row for the assertion below; an empty and a one-step row)
    c = Case(rng, B, T, 12, H, Lyr, lengths=n)
    c.state_matters()
    c.forward()
    G1, dx1, dhx1 = c.backward()
    buf = dev(c.dhn)
    G2, dx2, dhx2 = c.backward(dhx=buf, dh_n_t=buf)
    assert dhx2 is buf and torch.isfinite(dhx1).all() and not torch.equal(dhx1, dev(c.dhn))
    assert np.array_equal(bits(dhx1), bits(dhx2)), 'dhx written over dh_n'
    assert np.array_equal(bits(dx1), bits(dx2)), 'dx'
    for k, a, b in zip(c.names, G1, G2):
        assert np.array_equal(bits(a), bits(b)), k


# ----------------------------------------------------------------------------- F. chunks compose, forward and backward
@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_chunked_train_step_equals_whole_against_the_oracle(ragged, gemm_mode):
    """T = 7 cut as 1 + 4 + 2 at p = 0: RUN_TRAIN forwards with the state carried, backwards in reverse with dhx fed back as dh_n in
    place; summed dW / db and the first chunk's dx against the unchanged oracle on the whole sequence."""
    H, Lyr, B, T, F, cuts = 128, 2, 3, 7, 12, (1, 4, 2)
    n = np.array([7, 3, 0]) if ragged else np.array([T] * B)
    rng = case_rng(H, Lyr, B, T, 4)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    for b in range(B):
        x[b, n[b]:] = 0.0
    dy = f32(rng.standard_normal((B, T, H)) * 0.3)
    for b in range(B):
        dy[b, n[b]:] = 0.0
    dhn = f32(rng.standard_normal((Lyr, B, H)) * 0.3)
    ref = oracle_stack(x, P, PREFIX, 'gru', 1, Lyr, lengths=n if ragged else None, dy=dy, dhn=dhn)
    Wd = [dev(P[k]) for k in names]
    h = torch.zeros(Lyr, B, H, device=DEV)
    chunks, t0 = [], 0
    for Tc in cuts:
        rnn = make_rnn(B, Tc, F, H, Lyr, pool='mean')
        xc, hin = dev(x[:, t0:t0 + Tc]), h.clone()
        nc = torch.from_numpy(np.clip(n - t0, 0, Tc).astype(np.int32)).to(DEV) if ragged else None
        if ragged:
            rnn.forward_state_varlen(xc, Wd, nc, h_n=h, hx=hin)
        else:
            rnn.forward(xc, Wd, h_n=h, hx=hin)
        clean(rnn)
        chunks.append((rnn, xc, hin, nc, t0, Tc))
        t0 += Tc
    compare('F', f'forward {"ragged" if ragged else "dense"} {gemm_mode}', [(f'h_n[{i}]', host(h)[i], ref['h_n'][i]) for i in range(Lyr)])
    dh = dev(dhn)
    acc = [torch.zeros_like(w) for w in Wd]
    dx0 = None
    for rnn, xc, hin, nc, t0, Tc in reversed(chunks):
        Gd = [torch.full_like(w, NAN) for w in Wd]
        dx = nans(B, Tc, F)
        kw = dict(dy=dev(dy[:, t0:t0 + Tc]), dh_n=dh, dx=dx, hx=hin, dhx=dh)
        if ragged:
            rnn.backward_state_varlen(xc, Wd, Gd, nc, **kw)
        else:
            rnn.backward(xc, Wd, Gd, **kw)
        clean(rnn)
        for a, g in zip(acc, Gd):
            a += g
        dx0 = dx
    gr = [(k, host(a), ref['G'][k]) for k, a in zip(names, acc)]
    gr.append(('dx of chunk 0', host(dx0), ref['dx'][:, :cuts[0]]))
    compare('F', f'backward {"ragged" if ragged else "dense"} {gemm_mode}', [], gr)


# ----------------------------------------------------------------------------- G. batch chunks, the plan, plain calls
def test_batch_chunks_with_state(gemm_mode):
    """B = 517 at H = 256: rows 512 .. 516 run in a second launch, which must index hx / dhx by the global row."""
    c = Case(case_rng(517, 3), 517, 3, 8, 256, 1)
    ref = c.state_matters()
    c.forward()
    Gd, dx, dhx = c.backward()
    for what, sl in (('first launch', slice(0, 512)), ('second launch', slice(512, 517))):
        compare('G', f'{what} {gemm_mode}', [('h_n', host(c.h_n)[0][sl], ref['h_n'][0][sl])],
                [('dx', host(dx)[sl], ref['dx'][sl]), ('dhx', host(dhx)[0][sl], ref['dhx'][0][sl])])
    compare('G', f'weights {gemm_mode}', [], [(k, host(g), ref['G'][k]) for k, g in zip(c.names, Gd)])


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('H,T', [(64, 4), (256, 4), (256, 3), (512, 2)])
def test_state_call_launches_the_plain_impl4_instances_and_plain_calls_agree(H, T, ragged, gemm_mode):
    B, Lyr, F = 20, 2, 12
    rng = case_rng(H, T, 11)
    n = rng.integers(0, T + 1, B) if ragged else None
    c5 = Case(case_rng(H, T, 12), B, T, F, H, Lyr, lengths=n, impl=5)
    c4 = Case(case_rng(H, T, 12), B, T, F, H, Lyr, lengths=n, impl=4)

    def plain(c):
        c.rnn.reserve.fill_(NAN)
        pooled, h_n, dx = nans(B, H), nans(Lyr, B, H), nans(B, T, F)
        Gd = [torch.full_like(w, NAN) for w in c.Wd]
        L.instance_log_read(reset=True)
        c.rnn.forward(c.xd, c.Wd, pooled=pooled, h_n=h_n, lengths=c.ld)
        c.rnn.backward(c.xd, c.Wd, Gd, dy=dev(c.dy), dpooled=dev(c.dpool), dh_n=dev(c.dhn), dx=dx, lengths=c.ld)
        clean(c.rnn)
        return [pooled, h_n, dx] + Gd, L.instance_log_read(reset=True)

    r4, log4 = plain(c4)
    r5, log5 = plain(c5)
    assert log4 == log5, sorted(log4 ^ log5)
    for a, b in zip(r4, r5):
        assert torch.isfinite(a).all() and np.array_equal(bits(a), bits(b)), 'plain calls of impl 4 and 5: identical bits'
    L.instance_log_read(reset=True)
    c5.forward()
    c5.backward()
    inst = sweep_instances(L.instance_log_read(reset=True))
    assert inst == sweep_instances(log4), (sorted(inst), sorted(sweep_instances(log4)))
    assert any('gru_bwd_cluster_r1' in s for s in inst) and any('gru_fwd_cluster_r1' in s for s in inst)


def test_refusals_through_the_binding():
    c = Case(case_rng(1), 3, 2, 8, 64, 1)
    c.forward()
    with pytest.raises(L.DepError, match="LSTM's cell state"):
        c.rnn.backward(c.xd, c.Wd, [torch.empty_like(w) for w in c.Wd], dh_n=dev(c.dhn), hx=c.hxd, dcx=torch.empty_like(c.hxd))
    L.set_gemm_mode(2, 0)
    try:
        with pytest.raises(L.DepError, match='GEMM modes 0 and 1 only'):
            c.rnn.backward(c.xd, c.Wd, [torch.empty_like(w) for w in c.Wd], dh_n=dev(c.dhn), hx=c.hxd, dhx=torch.empty_like(c.hxd))
    finally:
        L.set_gemm_mode(1, 1 << 28)


# ----------------------------------------------------------------------------- H. the consumer: AudioGRU.forward_chunked()
def make_audio(variant, F, H, p, seed):
    from icassp2022_depression_amd import audio_bilstm_perm, audio_gru_whole
    mod = audio_gru_whole if variant == 'clf' else audio_bilstm_perm
    cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=p)
    model = mod.AudioBiLSTM(cfg, seed=seed)
    if variant == 'clf':                                               # a LayerNorm affine that is not the identity
        sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        rng = np.random.default_rng(seed)
        sd['ln.weight'] = (1.0 + 0.3 * rng.standard_normal(F)).astype(np.float32)
        sd['ln.bias'] = (0.2 * rng.standard_normal(F)).astype(np.float32)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.train()
    model.keep_chunk_states = True                                     # backward() keeps each recomputed chunk's h_n for the bit comparison
    return model


def train_step(model, variant, x, y, lengths, chunk_steps=None, impl=None):
    """One forward + loss + backward from dropout-seed counter 0; returns (output, z, {name: gradient}) as float64 host arrays."""
    from icassp2022_depression_amd import nn
    nn._seed_counter[0] = 0
    crit = nn.CrossEntropyLoss() if variant == 'clf' else nn.L1Loss()
    for p in model.parameters():
        if p.grad is not None:
            p.grad.fill_(NAN)
    out = model(x, lengths=lengths) if chunk_steps is None else model.forward_chunked(x, chunk_steps, lengths=lengths, impl=impl)
    crit(out, y if variant == 'clf' else y.reshape(-1, 1)).backward()
    model.check_health()
    return host(out.data), host(out._z), {k: host(p.grad) for k, p in model.named_parameters() if p.grad is not None}


def model_inputs(variant, B, T, F, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    y = rng.integers(0, 2, B) if variant == 'clf' else (rng.random(B) * 3 + 1).astype(np.float32)
    return x, y


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('H', [64, 256])
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_forward_chunked_is_the_whole_train_step(variant, H, ragged):
    B, T, F = 5, 11, 12
    model = make_audio(variant, F, H, 0.0, seed=7)
    x, y = model_inputs(variant, B, T, F, H + ragged)
    n = np.array([11, 0, 6, 3, 9], dtype=np.int32) if ragged else None      # an empty row; rows ending inside chunk 2 of 4-step chunks
    if ragged:
        for b in range(B):
            x[b, n[b]:] = 0.0
    out0, z0, g0 = train_step(model, variant, x, y, n)
    assert any(np.abs(v).max() > 0 for v in g0.values())
    for chunk in (4, 11, 20):
        for cache in model._chunk_rnns.values():
            cache.cache.clear()
        out, z, g = train_step(model, variant, x, y, n, chunk_steps=chunk)
        assert sorted(g) == sorted(g0)
        compare('H', f'{variant} H={H} {"ragged" if ragged else "dense"} chunk={chunk}', [('out', out, out0), ('z', z, z0)],
                [(k, g[k], g0[k]) for k in g0 if np.abs(g0[k]).max() > 0])
        # the plan: impl 5 descriptors, none longer than a chunk; the whole-call cache was not touched
        assert list(model._chunk_rnns) == [L.IMPL_CLUSTER_PER_LAYER_STATE]
        keys = list(model._chunk_rnns[L.IMPL_CLUSTER_PER_LAYER_STATE].cache)
        assert keys and all(k[1] <= min(chunk, T) for k in keys), keys
        assert {k[2] for k in keys} == {L.RUN_TRAIN, L.RUN_DROPOUT_ONLY}
        # each recomputed chunk's h_n is the state the first pass handed to the next chunk, bit for bit
        c = model._chunked
        nxt = c['hxs'][1:] + [c['h_end']]
        for k, (a, b) in enumerate(zip(c['h_n_recomputed'], nxt)):
            assert np.array_equal(bits(a), bits(b)), f'chunk {k}'


@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_forward_chunked_with_dropout_is_reproducible(variant):
    B, T, F, H = 5, 11, 12, 256
    model = make_audio(variant, F, H, 0.5, seed=9)
    x, y = model_inputs(variant, B, T, F, 3)
    a = train_step(model, variant, x, y, None, chunk_steps=4)
    b = train_step(model, variant, x, y, None, chunk_steps=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in a[2]:
        assert np.isfinite(a[2][k]).all() and np.array_equal(a[2][k], b[2][k]), k
    seeds = model._chunked['seeds']
    assert len(seeds) == 3 and len(set(seeds)) == 3                    # one dropout seed per chunk
    c = model._chunked
    for k, (u, v) in enumerate(zip(c['h_n_recomputed'], c['hxs'][1:] + [c['h_end']])):
        assert np.array_equal(bits(u), bits(v)), f'chunk {k}: the recompute draws the first pass\'s masks'


def test_forward_chunked_falls_back_to_the_tile_sweeps_and_an_optimizer_step_runs():
    from icassp2022_depression_amd import audio_gru_whole, nn
    B, T, F, H = 5, 11, 12, 48
    model = make_audio('clf', F, H, 0.0, seed=11)
    x, y = model_inputs('clf', B, T, F, 5)
    out0, z0, g0 = train_step(model, 'clf', x, y, None)
    L.instance_log_read(reset=True)
    out, z, g = train_step(model, 'clf', x, y, None, chunk_steps=4)
    inst = sweep_instances(L.instance_log_read(reset=True))
    assert list(model._chunk_rnns) == [L.IMPL_TILE]
    assert inst and not any('cluster' in s for s in inst), sorted(inst)
    compare('H', 'clf H=48 impl 2', [('out', out, out0), ('z', z, z0)], [(k, g[k], g0[k]) for k in g0 if np.abs(g0[k]).max() > 0])
    with pytest.raises(L.DepError, match='impl = 5'):
        model.forward_chunked(x, 4, impl=L.IMPL_CLUSTER_PER_LAYER_STATE)
    # an optimizer step on the chunked gradients, at a shape on impl 5
    model = make_audio('clf', F, 64, 0.0, seed=12)
    opt = nn.AdamW(audio_gru_whole.get_param_group(model), lr=1e-2)
    before = {k: host(p.data) for k, p in model.named_parameters()}
    opt.zero_grad()
    nn.CrossEntropyLoss()(model.forward_chunked(x, 4), y).backward()
    opt.step()
    model.check_health()
    after = {k: host(p.data) for k, p in model.named_parameters()}
    assert all(np.isfinite(v).all() for v in after.values())
    assert any(not np.array_equal(after[k], before[k]) for k in after)
