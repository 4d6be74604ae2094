"""GPU parity of impl = 6, the per-layer cluster forward of a bidirectional GRU: gru_fwd_cluster_r1<KCH, SPLIT, RAG, true> runs every
forward (both directions of a batch chunk in one launch), the tile-MFMA BiGRU backward (gru_bwd_mfma<.., true>) reads the reserve it
leaves.

The expectation is tests/bigru_ref.py; where a recurrent state comes in, tests/hx_ref.py (dense) and tests/state_varlen_ref.py (state
with lengths).  Tolerances are the project's own for every recurrent path: 1e-4 absolute on y / pooled / h_n / layer outputs, 1e-4
relerr on dx and every gradient.  Where the same call also runs on impl = 2 (H <= 256) the two results, each within 1e-4 of the
oracle, are held to 2e-4 of each other.  Outputs and gradient buffers are pre-filled with NaN; after every call rnn.check() passes
and the status word is 0.
Run on the MI355X box:  python -m pytest tests/test_bigru_cluster_gpu.py -m gpu -q"""
import os
import re

import numpy as np
import pytest

import hx_ref
import state_varlen_ref as svr
from bigru_ref import bigru
from varlen_ref import lengths_mix

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

ATOL = 1e-4
RTOL = 1e-4
PREFIX = 'gru'
NAN = float('nan')
POOLS = {'mean': 1, 'sum': 2}          # DEP_POOL_*


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


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def pad_mask(lengths, T):
    return np.arange(T)[None, :] >= np.asarray(lengths)[:, None]


def make_params(rng, F, H, Lyr):
    """Weights in the order the header documents for dirs = 2: l0, l0_reverse, l1, ...; layer l > 0 has weight_ih (3H, 2H)."""
    P = {}; names = []
    k = 1.0 / np.sqrt(H)
    for l in range(Lyr):
        for d in range(2):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else 2 * H
            for nm, shp in (('weight_ih', (3 * H, inp)), ('weight_hh', (3 * H, H)), ('bias_ih', (3 * H,)), ('bias_hh', (3 * H,))):
                key = f'{PREFIX}.{nm}_{sfx}'
                P[key] = f32(rng.uniform(-k, k, shp))
                names.append(key)
    return P, names


@pytest.fixture(params=['f32', 'bf16x3'])
def gemm_mode(request):
    """Both precision modes of the parity path (forced on every contraction size), as in tests/test_bigru_gpu.py."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


class launched:
    """The sweeps enqueued inside the block, from the enqueue-order log (a list: the instance log is a set over the whole test, so it
    cannot say what the second of two like calls launched; it is left alone here and keeps recording for tests/conftest.py)."""

    def __enter__(self):
        L.order_log_enable(True)
        L.order_log_read(reset=True)
        return self

    def __exit__(self, *exc):
        log = L.order_log_read(reset=True)
        L.order_log_enable(False)
        self.sweeps = [re.sub(r'^\(|\)$', '', e[2:]) for e in log if e.startswith('K ') and re.search(r'(gru|lstm)2?_(fwd|bwd)_', e)]
        self.inst = set(self.sweeps)


def case_rng(*v):
    return np.random.default_rng(600 + sum(int(a) * 7 ** i for i, a in enumerate(v)))


ident = lambda c: '-'.join(str(v) for v in c)


def make_rnn(B, T, F, H, Lyr, run, p=0.0, pool='mean', impl=6):
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, Lyr, 2, run, p, POOLS[pool], DEV, impl=impl)
    rnn.reserve.fill_(NAN)
    assert (rnn.status_word() is not None) == (impl == 6)              # impl = 6 has an exchange buffer, impl 0 / 2 never
    return rnn


def healthy(rnn):
    rnn.check()
    assert int(rnn.status_word().item()) == 0


def forward_instance(H, split, ragged):
    return 'gru_fwd_cluster_r1<%d, %s, %s, true>' % (H // 32, 'true' if split else 'false', 'true' if ragged else 'false')


def check_instances(inst, H, split, ragged, backward=False):
    """The forward sweeps are the BI cluster instance of this H / precision / raggedness and nothing else -- no gru_fwd_mfma; the
    backward sweeps (when the call had one) are gru_bwd_mfma<.., true> only."""
    fwd = {s for s in inst if '_fwd_' in s}
    assert fwd == {forward_instance(H, split, ragged)}, sorted(inst)
    bwd = inst - fwd
    assert bool(bwd) == backward, sorted(inst)
    for s in bwd:
        assert re.fullmatch(r'gru_bwd_mfma<\d, %s, true>' % ('true' if ragged else 'false'), s), sorted(inst)


def close(what, pairs, tol=ATOL):
    """pairs: (name, device value as float64, expectation).  Every figure is printed before any assertion."""
    errs = [(float(np.abs(a - b).max()) if np.isfinite(a).all() else NAN, n) for n, a, b in pairs]
    print(f'bigru-cluster {what}: ' + ', '.join(f'{n} {e:.2e}' for e, n in errs))
    for e, n in errs:
        assert e < tol, f'{what}: {n}: {e:.3e}'


def close_rel(what, pairs, tol=RTOL):
    errs = [(float(relerr(a, b)) if np.isfinite(a).all() else NAN, n) for n, a, b in pairs]
    print(f'bigru-cluster {what}: ' + ', '.join(f'{n} {e:.2e}' for e, n in errs))
    for (e, n), (_, _, b) in zip(errs, pairs):
        assert np.abs(b).max() > 0, f'{n}: the reference gradient is trivially zero'
        assert e < tol, f'{what}: {n}: {e:.3e}'


def forward(rnn, xd, Wd, B, T, H, Lyr, lengths=None, hx=None, seed=0):
    """One forward with every output NaN-filled; the sweep instances it launched."""
    out = dict(pooled=nans(B, 2 * H), h_n=nans(2 * Lyr, B, H), y=nans(B, T, 2 * H))
    with launched() as k:
        if lengths is not None and hx is not None:
            rnn.forward_state_varlen(xd, Wd, lengths, seed=seed, hx=hx, **out)
        else:
            rnn.forward(xd, Wd, seed=seed, lengths=lengths, hx=hx, **out)
    healthy(rnn) if rnn.status_word() is not None else rnn.check()
    out['inst'], out['sweeps'] = k.inst, k.sweeps
    return out


def forward_pairs(out, rnn, ref, Lyr, layers=True):
    p = [('y', host(out['y']), ref['y']), ('pooled', host(out['pooled']), ref['pooled']), ('h_n', host(out['h_n']), ref['h_n'])]
    if layers:
        p += [(f'layer {l} output', host(rnn.layer_output(l)), ref['ys'][l]) for l in range(Lyr)]
    return p


# ----------------------------------------------------------------------------- forward parity, dense
# (B, T, F, H, layers): one step, no exchange at all | one layer | a ragged second tile, both payload parities | H = 256 |
# H = 512, which the tile sweeps cannot run | three layers: a middle layer reads and writes 2H-wide rows | five layers: the fifth shares
# exchange-header slot 0 with the first and clears it itself
DENSE_CASES = [(3, 1, 8, 64, 2), (5, 2, 8, 64, 1), (17, 3, 12, 128, 2), (19, 5, 16, 256, 2), (5, 4, 8, 512, 2), (4, 6, 8, 64, 3), (3, 3, 8, 64, 5)]


@pytest.mark.parametrize('case', DENSE_CASES, ids=ident)
def test_dense_forward_parity(case, gemm_mode):
    B, T, F, H, Lyr = case
    rng = case_rng(*case)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    Wd = [dev(P[n]) for n in names]
    xd = dev(x)
    ref = bigru(x, P, PREFIX, Lyr, pool='mean')
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL)
    out = forward(rnn, xd, Wd, B, T, H, Lyr)
    close(f'dense {ident(case)} {gemm_mode}', forward_pairs(out, rnn, ref, Lyr))
    check_instances(out['inst'], H, gemm_mode == 'bf16x3', False)
    if H <= 256:
        tile = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL, impl=2)
        o2 = forward(tile, xd, Wd, B, T, H, Lyr)
        assert all('gru_fwd_mfma' in s for s in o2['inst']) and o2['inst']
        close(f'dense {ident(case)} {gemm_mode} against impl = 2',
              [(k, host(out[k]), host(o2[k])) for k in ('y', 'pooled', 'h_n')] +
              [(f'layer {l} output', host(rnn.layer_output(l)), host(tile.layer_output(l))) for l in range(Lyr)], tol=2 * ATOL)
    else:
        with pytest.raises(L.DepError, match='tile-MFMA'):
            L.Rnn(L.CELL_GRU, B, T, F, H, Lyr, 2, False, 0.0, 1, DEV, impl=2)


# ----------------------------------------------------------------------------- ragged
RAGGED_H = [64, 128, 256, 512]


def ragged_case(H, gemm_mode):
    B, T, F, Lyr = 19, 5, 12, 2
    rng = case_rng(B, T, F, H, 1)
    lengths = lengths_mix(B, T, rng)
    assert (lengths == 0).any() and (lengths == T).any()
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    pad = pad_mask(lengths, T)
    x[pad] = 0.0
    return B, T, F, Lyr, lengths, P, names, x, pad


@pytest.mark.parametrize('H', RAGGED_H)
def test_ragged_forward_parity(H, gemm_mode):
    """live = t < len: the reverse direction of a row meets its dead steps first and carries zero through them; y and layer 0's output
    are exactly 0.0 at dead positions, h_n and the pool of an empty row are exactly 0.0."""
    B, T, F, Lyr, lengths, P, names, x, pad = ragged_case(H, gemm_mode)
    Wd = [dev(P[n]) for n in names]
    for pool in ('mean', 'sum'):
        ref = bigru(x, P, PREFIX, Lyr, lengths=lengths, pool=pool)
        rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL, pool=pool)
        out = forward(rnn, dev(x), Wd, B, T, H, Lyr, lengths=idev(lengths))
        close(f'ragged H={H} {gemm_mode} pool={pool}', forward_pairs(out, rnn, ref, Lyr))
        check_instances(out['inst'], H, gemm_mode == 'bf16x3', True)
        assert not bits(out['y'])[pad].any(), 'y is not exactly 0.0 at dead positions'
        assert not bits(rnn.layer_output(0))[pad].any(), 'layer 0 output is not exactly 0.0 at dead positions'
        assert not bits(out['h_n'])[:, lengths == 0].any(), 'h_n of an empty row is not 0'
        assert not bits(out['pooled'])[lengths == 0].any(), 'the pool of an empty row is not 0'


@pytest.mark.parametrize('H', RAGGED_H)
def test_all_lengths_T_gives_the_dense_calls_bits(H, gemm_mode):
    B, T, F, Lyr = 19, 5, 12, 2
    rng = case_rng(B, T, F, H, 2)
    P, names = make_params(rng, F, H, Lyr)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    res = []
    for lengths in (None, idev(np.full(B, T))):
        rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL)
        out = forward(rnn, xd, Wd, B, T, H, Lyr, lengths=lengths)
        check_instances(out['inst'], H, gemm_mode == 'bf16x3', lengths is not None)
        res.append([out['y'], out['pooled'], out['h_n'], rnn.layer_output(0).clone()])
    for nm, a, b in zip(('y', 'pooled', 'h_n', 'layer 0 output'), *res):
        assert torch.isfinite(a).all(), nm
        assert torch.equal(a, b), nm


# ----------------------------------------------------------------------------- state
def state_masks(B, T, H, Lyr, p, seed):
    return [host(L.dropout_mask(B * T * 2 * H, p, seed, 16 + l, DEV)).reshape(B, T, 2 * H) for l in range(Lyr - 1)]      # site = DEP_SITE_RNN0 + l


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('run', ['eval', 'dropout_only'])
@pytest.mark.parametrize('H', [64, 256])
def test_forward_with_a_random_state(H, run, ragged, gemm_mode):
    """hx is taken by every forward: each direction's clusters start from their own slice, ordered like h_n (l * 2 + d).  A ragged row
    of length 0 returns hx bit for bit in both directions."""
    B, T, F, Lyr, p, seed = 19, 4, 12, 2, 0.5, 4321
    rng = case_rng(B, T, H, 3)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    lengths = lengths_mix(B, T, rng) if ragged else None
    if ragged:
        assert (lengths == 0).any() and (lengths == T).any()
        x[pad_mask(lengths, T)] = 0.0
    hx = f32(rng.standard_normal((2 * Lyr, B, H)) * 0.6)
    Wd = [dev(P[n]) for n in names]
    hxd = dev(hx)
    donly = run == 'dropout_only'
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_DROPOUT_ONLY if donly else L.RUN_EVAL, p=p if donly else 0.0)
    out = forward(rnn, dev(x), Wd, B, T, H, Lyr, lengths=None if lengths is None else idev(lengths), hx=hxd, seed=seed)
    masks = state_masks(B, T, H, Lyr, p, seed) if donly else None
    if donly:
        assert 0.3 < (masks[0] == 0).mean() < 0.7
    if ragged:
        ref = svr.stack(x, lengths, P, PREFIX, 'gru', 2, Lyr, hx=hx, pool='mean', masks=masks)
        plain = svr.stack(x, lengths, P, PREFIX, 'gru', 2, Lyr, pool='mean', masks=masks)
    else:
        ref = hx_ref.stack(x, P, PREFIX, 'gru', 2, Lyr, hx=hx, pool='mean', masks=masks)
        plain = hx_ref.stack(x, P, PREFIX, 'gru', 2, Lyr, pool='mean', masks=masks)
    assert np.abs(ref['h_n'] - plain['h_n']).max() > 100 * ATOL and np.abs(ref['y'] - plain['y']).max() > 100 * ATOL      # the state matters
    close(f'state H={H} {run} {"ragged" if ragged else "dense"} {gemm_mode}', forward_pairs(out, rnn, ref, Lyr, layers=not donly))
    check_instances(out['inst'], H, gemm_mode == 'bf16x3', ragged)
    if ragged:
        empty = lengths == 0
        assert np.array_equal(bits(out['h_n'])[:, empty], bits(hxd)[:, empty]), 'len 0: h_n is hx bit for bit, both directions of both layers'
        assert not bits(out['y'])[pad_mask(lengths, T)].any() and not bits(out['pooled'])[empty].any()


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_h_n_may_alias_hx_at_one_step(ragged, gemm_mode):
    """T = 1: no exchange orders a member's h_n store behind the other members' reads of hx, the call stages the layer's 2 x B x H slice."""
    B, T, F, H, Lyr = 19, 1, 12, 128, 2
    rng = case_rng(B, T, H, 5)
    P, names = make_params(rng, F, H, Lyr)
    Wd = [dev(P[n]) for n in names]
    xd = dev(rng.standard_normal((B, T, F)))
    hx = dev(rng.standard_normal((2 * Lyr, B, H)) * 0.6)
    ld = idev(rng.integers(0, T + 1, B)) if ragged else None
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL)

    def run(h_in, h_out):
        rnn.reserve.fill_(NAN)
        pooled = nans(B, 2 * H)
        if ragged:
            rnn.forward_state_varlen(xd, Wd, ld, pooled=pooled, h_n=h_out, hx=h_in)
        else:
            rnn.forward(xd, Wd, pooled=pooled, h_n=h_out, hx=h_in)
        healthy(rnn)
        return rnn.layer_output().clone(), pooled

    h_n = nans(2 * Lyr, B, H)
    y1, p1 = run(hx, h_n)
    h2 = hx.clone()
    y2, p2 = run(h2, h2)
    assert torch.isfinite(h_n).all() and not torch.equal(h_n, hx)
    assert np.array_equal(bits(y1), bits(y2)), 'y'
    assert np.array_equal(bits(p1), bits(p2)), 'pooled'
    assert np.array_equal(bits(h_n), bits(h2)), 'h_n written over hx'


# ----------------------------------------------------------------------------- training: forward on the cluster, backward on the tile sweeps
def run_stack(B, T, F, H, Lyr, form, rng, lengths=None, p=0.0, seed=0, state=False):
    """One DEP_RUN_TRAIN forward + backward on impl = 6.  'full': dy + dpooled + dh_n in (NaN at the dead positions of dy in a ragged
    call: they are ignored), dx out; 'model': dpooled only, no dx.  state: a random hx in, dhx out (dense).  Returns (device results,
    reference, the sweep instances launched)."""
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    pad = None
    if lengths is not None:
        pad = pad_mask(lengths, T)
        x[pad] = 0.0
    pool = 'mean' if form == 'full' else 'sum'
    Wd = [dev(P[n]) for n in names]
    Gd = [torch.full_like(w, NAN) for w in Wd]
    xd = dev(x)
    ld = None if lengths is None else idev(lengths)
    hx = f32(rng.standard_normal((2 * Lyr, B, H)) * 0.6) if state else None
    hxd = None if hx is None else dev(hx)
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_TRAIN, p=p, pool=pool)
    pooled, h_n = nans(B, 2 * H), nans(2 * Lyr, B, H)
    dpool = f32(rng.standard_normal((B, 2 * H)))
    dxd = dhxd = None
    kw = dict(dpooled=dpool)
    bw = dict(dpooled=dev(dpool), dx=None, lengths=ld)
    if form == 'full':
        dyv = f32(rng.standard_normal((B, T, 2 * H)) * 0.3)
        dhn = f32(rng.standard_normal((2 * Lyr, B, H)) * 0.3)
        dy_in = dyv.copy()
        if pad is not None:
            dy_in[pad] = np.nan
        dxd = nans(B, T, F)
        kw.update(dy=dyv, dhn=dhn)
        bw.update(dy=dev(dy_in), dh_n=dev(dhn), dx=dxd)
        if state:
            dhxd = nans(2 * Lyr, B, H)
            bw.update(hx=hxd, dhx=dhxd)
    with launched() as k:
        rnn.forward(xd, Wd, seed=seed, pooled=pooled, h_n=h_n, lengths=ld, hx=hxd)
        rnn.backward(xd, Wd, Gd, **bw)
    healthy(rnn)
    inst = k.inst
    masks = state_masks(B, T, H, Lyr, p, seed) if p > 0 else None
    if state:
        ref = hx_ref.stack(x, P, PREFIX, 'gru', 2, Lyr, hx=hx, pool=pool, masks=masks, **kw)
    else:
        ref = bigru(x, P, PREFIX, Lyr, lengths=lengths, pool=pool, masks=masks, **kw)
    out = dict(rnn=rnn, y=rnn.layer_output(), pooled=pooled, h_n=h_n, dx=dxd, dhx=dhxd, G=Gd, names=names, pad=pad)
    return out, ref, inst


def check_training(what, out, ref, Lyr):
    close(what, forward_pairs(out, out['rnn'], ref, Lyr))
    grads = [(n, host(g), ref['G'][n]) for n, g in zip(out['names'], out['G'])]
    if out['dx'] is not None:
        grads.append(('dx', host(out['dx']), ref['dx']))
    if out['dhx'] is not None:
        grads.append(('dhx', host(out['dhx']), ref['dhx']))
    close_rel(what, grads)


TRAIN_CASES = [(17, 3, 12, 128, 2), (19, 5, 16, 256, 2)]


@pytest.mark.parametrize('form', ['full', 'model'])
@pytest.mark.parametrize('case', TRAIN_CASES, ids=ident)
def test_training_step_dense(case, form, gemm_mode):
    """The reserve of the cluster forward is one the unchanged gru_bwd_mfma<.., true> reads: every gradient against the oracle."""
    B, T, F, H, Lyr = case
    out, ref, inst = run_stack(B, T, F, H, Lyr, form, case_rng(*case, form == 'full'))
    check_training(f'train {ident(case)} {form} {gemm_mode}', out, ref, Lyr)
    check_instances(inst, H, gemm_mode == 'bf16x3', False, backward=True)


@pytest.mark.parametrize('form', ['full', 'model'])
@pytest.mark.parametrize('case', TRAIN_CASES, ids=ident)
def test_training_step_ragged(case, form, gemm_mode):
    B, T, F, H, Lyr = case
    rng = case_rng(*case, form == 'full', 1)
    lengths = lengths_mix(B, T, rng)
    assert (lengths == 0).any() and (lengths == T).any()
    out, ref, inst = run_stack(B, T, F, H, Lyr, form, rng, lengths=lengths)
    check_training(f'train ragged {ident(case)} {form} {gemm_mode}', out, ref, Lyr)
    check_instances(inst, H, gemm_mode == 'bf16x3', True, backward=True)
    pad = out['pad']
    assert not bits(out['y'])[pad].any() and not bits(out['rnn'].layer_output(0))[pad].any()
    if out['dx'] is not None:
        assert not bits(out['dx'])[pad].any(), 'dx is not exactly 0.0 at dead positions'


def test_training_step_with_hx_dh_n_and_dhx(gemm_mode):
    """hx into the cluster forward, hx / dh_n / dhx through the tile backward."""
    B, T, F, H, Lyr = 17, 3, 12, 128, 2
    out, ref, inst = run_stack(B, T, F, H, Lyr, 'full', case_rng(B, T, H, 8), state=True)
    check_training(f'train with state {gemm_mode}', out, ref, Lyr)
    check_instances(inst, H, gemm_mode == 'bf16x3', False, backward=True)
    assert np.abs(ref['dhx']).max() > 0


# ----------------------------------------------------------------------------- dropout
def test_interlayer_dropout_matches_the_oracle_with_the_devices_masks(gemm_mode):
    """The draw is over the element index of (b, t, col) in the (B,T,2H) array at site DEP_SITE_RNN0 + l, as the tile BiGRU's."""
    B, T, F, H, Lyr, p, seed = 5, 9, 10, 128, 2, 0.5, 1234
    out, ref, inst = run_stack(B, T, F, H, Lyr, 'full', case_rng(B, T, H, 9), p=p, seed=seed)
    rnn = out['rnn']
    mask = state_masks(B, T, H, Lyr, p, seed)[0]
    assert set(np.unique(mask)).issubset({0.0, 2.0}) and 0.35 < (mask == 0).mean() < 0.65
    assert torch.equal(rnn.layer_output_dropped(0), rnn.layer_output(0) * dev(mask)), 'dropout(y0) is not y0 * mask'
    check_training(f'dropout {gemm_mode}', out, ref, Lyr)
    check_instances(inst, H, gemm_mode == 'bf16x3', False, backward=True)


def dropout_forward(B, T, F, H, p, seed, run, impl, rng_seed):
    rng = np.random.default_rng(rng_seed)
    P, names = make_params(rng, F, H, 2)
    Wd = [dev(P[n]) for n in names]
    rnn = make_rnn(B, T, F, H, 2, run, p=p, impl=impl)
    out = forward(rnn, dev(rng.standard_normal((B, T, F))), Wd, B, T, H, 2, seed=seed)
    out.update(rnn=rnn, Wd=Wd)
    return out


def test_dropout_only_forward_gives_the_train_forwards_bits(gemm_mode):
    B, T, F, H, p, seed = 19, 5, 12, 64, 0.5, 99
    tr = dropout_forward(B, T, F, H, p, seed, L.RUN_TRAIN, 6, 5)
    do = dropout_forward(B, T, F, H, p, seed, L.RUN_DROPOUT_ONLY, 6, 5)
    for k in ('y', 'pooled', 'h_n'):
        assert torch.isfinite(tr[k]).all(), k
        assert torch.equal(tr[k], do[k]), k
    assert tr['inst'] == do['inst'] == {forward_instance(H, gemm_mode == 'bf16x3', False)}
    Gd = [torch.empty_like(w) for w in do['Wd']]
    with pytest.raises(L.DepError, match='DEP_RUN_TRAIN'):
        do['rnn'].backward(dev(np.zeros((B, T, F))), do['Wd'], Gd, dpooled=do['pooled'])


@pytest.mark.parametrize('H', [64, 256])
def test_the_dropped_positions_are_those_of_impl_2(H, gemm_mode):
    """Same seed, same element index in (B,T,2H): dropout(y0) is zero at the same positions on both plans."""
    B, T, F, p, seed = 19, 5, 12, 0.5, 777
    c6 = dropout_forward(B, T, F, H, p, seed, L.RUN_TRAIN, 6, 11)
    c2 = dropout_forward(B, T, F, H, p, seed, L.RUN_TRAIN, 2, 11)
    z6, z2 = host(c6['rnn'].layer_output_dropped(0)) == 0, host(c2['rnn'].layer_output_dropped(0)) == 0
    assert 0.35 < z6.mean() < 0.65
    assert np.array_equal(z6, z2)
    close(f'dropout H={H} {gemm_mode} against impl = 2', [(k, host(c6[k]), host(c2[k])) for k in ('y', 'pooled', 'h_n')], tol=2 * ATOL)


# ----------------------------------------------------------------------------- two launch chunks
def chunk_utterances(H):
    """Utterances one launch of the bidirectional forward covers.  A 16-utterance tile is two (direction, tile) clusters of H / 32
    workgroups, one workgroup per CU and at most 256 per launch: tiles per direction = min(CUs, 256) // (2 * H / 32), rounded down to
    whole groups of 8 when there are 8 or more (H = 512 on 256 CUs: 8 tiles per direction, 128 utterances)."""
    cus = int(os.environ.get('DEP_NUM_CUS', 0)) or torch.cuda.get_device_properties(0).multi_processor_count
    tiles = min(cus, 256) // (2 * (H // 32))
    if tiles >= 8:
        tiles = tiles // 8 * 8
    return max(tiles, 1) * 16


def test_a_batch_one_past_the_chunk_runs_two_launches(gemm_mode):
    H, T, F, Lyr = 512, 3, 8, 1
    B = chunk_utterances(H) + 1
    rng = case_rng(B, T, H, 10)
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    Wd = [dev(P[n]) for n in names]
    rnn = make_rnn(B, T, F, H, Lyr, L.RUN_EVAL)
    out = forward(rnn, dev(x), Wd, B, T, H, Lyr)
    assert out['sweeps'] == [forward_instance(H, gemm_mode == 'bf16x3', False)] * 2, out['sweeps']      # one layer: one launch per chunk
    ref = bigru(x, P, PREFIX, Lyr, pool='mean')
    close(f'two chunks B={B} {gemm_mode}', forward_pairs(out, rnn, ref, Lyr))
    check_instances(out['inst'], H, gemm_mode == 'bf16x3', False)


def test_h512_has_no_backward():
    B, T, F, H = 3, 2, 8, 512
    rng = case_rng(B, T, H, 12)
    P, names = make_params(rng, F, H, 1)
    Wd = [dev(P[n]) for n in names]
    rnn = make_rnn(B, T, F, H, 1, L.RUN_TRAIN)
    xd = dev(rng.standard_normal((B, T, F)))
    out = forward(rnn, xd, Wd, B, T, H, 1)
    assert torch.isfinite(out['y']).all()
    with pytest.raises(L.DepError, match='forward only'):
        rnn.backward(xd, Wd, [torch.empty_like(w) for w in Wd], dpooled=out['pooled'])
