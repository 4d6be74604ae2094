"""GPU parity of the bidirectional GRU stack, dep_rnn_desc{cell = DEP_CELL_GRU, dirs = 2} == torch.nn.GRU(bidirectional=True,
batch_first=True), dense and ragged, on the tile-MFMA sweeps (gru_*_mfma<JPW, RAG, true>), the only kernels that run it.

The expectation is tests/bigru_ref.py, a composition of the unchanged oracle's unidirectional layer (pinned against stock torch in
tests/test_bigru_cpu.py).  Tolerances are those of tests/test_kernels_gpu.py::test_rnn_stack_fwd_bwd: 1e-4 absolute on y / pooled /
h_n, 1e-4 relerr on dx and every gradient; gradient buffers are pre-filled with NaN.
Run on the MI355X box:  python -m pytest tests/test_bigru_gpu.py -m gpu -q"""
import re

import numpy as np
import pytest

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
    """Both precision modes of the parity path (forced on every contraction size), as in tests/test_varlen_gpu.py."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


def sweep_instances(log):
    return {re.sub(r'^\(|\)$', '', s) for s in log if re.search(r'(gru|lstm)2?_(fwd|bwd)_', s)}


def run_stack(B, T, F, H, Lyr, form, rng, lengths=None, impl=0, pool_kind='mean'):
    """One forward + backward of a BiGRU stack.  'full': dy + dpooled + dh_n in (NaN at the dead positions of dy in a ragged call:
    they are ignored), dx out; 'model': dpooled only, no dx.  Returns (device tensors, reference, the sweep instances launched)."""
    P, names = make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    pad = None
    if lengths is not None:
        pad = pad_mask(lengths, T)
        x[pad] = 0.0
    Wd = [dev(P[n]) for n in names]
    Gd = [torch.full_like(w, float('nan')) for w in Wd]
    xd = dev(x)
    ld = None if lengths is None else idev(lengths)
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, Lyr, 2, True, 0.0, L.POOL_MEAN if pool_kind == 'mean' else L.POOL_SUM, DEV, impl=impl)
    assert rnn.status_word() is None                               # no cluster exchange buffer: never a cluster plan
    rnn.reserve.fill_(float('nan'))
    pooled = torch.full((B, 2 * H), float('nan'), device=DEV)
    h_n = torch.full((2 * Lyr, B, H), float('nan'), device=DEV)
    before = L.instance_log_read()
    rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, lengths=ld)
    dpool = f32(rng.standard_normal((B, 2 * H)))
    dxd = None
    if form == 'full':
        dyv = f32(rng.standard_normal((B, T, 2 * H)) * 0.3)
        dhn = f32(rng.standard_normal((2 * Lyr, B, H)) * 0.3)
        dy_in = dyv.copy()
        if pad is not None:
            dy_in[pad] = np.nan
        dxd = torch.full((B, T, F), float('nan'), device=DEV)
        rnn.backward(xd, Wd, Gd, dy=dev(dy_in), dpooled=dev(dpool), dh_n=dev(dhn), dx=dxd, lengths=ld)
        ref = bigru(x, P, PREFIX, Lyr, lengths=lengths, pool=pool_kind, dy=dyv, dpooled=dpool, dhn=dhn)
    else:
        rnn.backward(xd, Wd, Gd, dpooled=dev(dpool), dx=None, lengths=ld)
        ref = bigru(x, P, PREFIX, Lyr, lengths=lengths, pool=pool_kind, dpooled=dpool)
    rnn.check()
    inst = sweep_instances(L.instance_log_read() - before)
    out = dict(rnn=rnn, y=rnn.layer_output(), pooled=pooled, h_n=h_n, dx=dxd, G=Gd, names=names, pad=pad)
    return out, ref, inst


def check_against(out, ref):
    assert np.abs(host(out['y']) - ref['y']).max() < ATOL, 'y'
    assert np.abs(host(out['pooled']) - ref['pooled']).max() < ATOL, 'pooled'
    assert np.abs(host(out['h_n']) - ref['h_n']).max() < ATOL, 'h_n'
    for l, yl in enumerate(ref['ys']):
        assert np.abs(host(out['rnn'].layer_output(l)) - yl).max() < ATOL, f'layer {l} output'
    if out['dx'] is not None:
        assert relerr(host(out['dx']), ref['dx']) < RTOL, 'dx'
    for n, g in zip(out['names'], out['G']):
        assert relerr(host(g), ref['G'][n]) < RTOL, n


def only_bi_tile_instances(inst, ragged):
    """Every sweep the call launched is a BI instance of the tile-MFMA kernels, RAG as the call; one forward and one backward kernel."""
    rag = 'true' if ragged else 'false'
    assert inst, 'no sweep was recorded'
    for s in inst:
        assert re.fullmatch(r'gru_(fwd|bwd)_mfma<\d, %s, true>' % rag, s), inst
    assert {s[:7] for s in inst} == {'gru_fwd', 'gru_bwd'}, inst


# (B, T, F, H, layers): one step with F no multiple of 4; two steps; jpw 3 in one wave with a ragged last tile; eight waves; jpw 2 at the
# width a unidirectional GRU takes to the cluster kernels; one layer; three layers (a middle layer reads and writes 2H-wide rows)
DENSE_CASES = [(2, 1, 5, 16, 2), (3, 2, 8, 16, 2), (19, 11, 40, 48, 2), (17, 9, 24, 128, 2), (33, 6, 16, 256, 2),
               (5, 7, 12, 16, 1), (5, 7, 12, 16, 3)]


@pytest.mark.parametrize('form', ['full', 'model'])
@pytest.mark.parametrize('B,T,F,H,Lyr', DENSE_CASES)
def test_bigru_stack_fwd_bwd(B, T, F, H, Lyr, form, gemm_mode):
    rng = np.random.default_rng(B * 1000 + T * 100 + F + H + Lyr)
    out, ref, inst = run_stack(B, T, F, H, Lyr, form, rng, pool_kind='mean' if form == 'full' else 'sum')
    check_against(out, ref)
    only_bi_tile_instances(inst, ragged=False)                     # H = 256 included: no cluster, 16-unit-member or fused kernel


def test_bigru_forced_tile_impl_gives_the_auto_plans_bits():
    """impl = 2 and impl = 0 are the same plan for a BiGRU."""
    res = []
    for impl in (0, 2):
        out, _, _ = run_stack(19, 11, 40, 48, 2, 'full', np.random.default_rng(3), impl=impl)
        res.append([out['y'].clone(), out['pooled'], out['h_n'], out['dx']] + out['G'])
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- inter-layer dropout
def dropout_case(B, T, F, H, p, seed, run, rng_seed):
    rng = np.random.default_rng(rng_seed)
    P, names = make_params(rng, F, H, 2)
    x = f32(rng.standard_normal((B, T, F)))
    Wd = [dev(P[n]) for n in names]
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, 2, 2, run, p, L.POOL_MEAN, DEV)
    rnn.reserve.fill_(float('nan'))
    pooled = torch.full((B, 2 * H), float('nan'), device=DEV)
    h_n = torch.full((4, B, H), float('nan'), device=DEV)
    y = torch.full((B, T, 2 * H), float('nan'), device=DEV)
    xd = dev(x)
    rnn.forward(xd, Wd, seed=seed, pooled=pooled, h_n=h_n, y=y)
    return dict(rnn=rnn, P=P, names=names, x=x, xd=xd, Wd=Wd, pooled=pooled, h_n=h_n, y=y, rng=rng)


@pytest.mark.parametrize('H', [16, 128])
def test_bigru_interlayer_dropout_matches_oracle_with_same_masks(H, gemm_mode):
    """The draw is over the element index of (b, t, col) in the (B,T,2H) array at site DEP_SITE_RNN0 + l, as the BiLSTM's."""
    B, T, F, p, seed = 5, 9, 10, 0.5, 1234
    c = dropout_case(B, T, F, H, p, seed, L.RUN_TRAIN, 77 + H)
    rnn, rng = c['rnn'], c['rng']
    mask = host(L.dropout_mask(B * T * 2 * H, p, seed, 16, DEV)).reshape(B, T, 2 * H)      # site = DEP_SITE_RNN0 + 0
    assert set(np.unique(mask)).issubset({0.0, 2.0}) and 0.35 < (mask == 0).mean() < 0.65
    y0 = rnn.layer_output(0); y0d = rnn.layer_output_dropped(0)
    assert torch.equal(y0d, y0 * dev(mask)), 'dropout(y0) is not y0 * mask'
    dyv = f32(rng.standard_normal((B, T, 2 * H))); dpool = f32(rng.standard_normal((B, 2 * H))); dhn = f32(rng.standard_normal((4, B, H)) * 0.3)
    Gd = [torch.full_like(w, float('nan')) for w in c['Wd']]
    dxd = torch.full((B, T, F), float('nan'), device=DEV)
    rnn.backward(c['xd'], c['Wd'], Gd, dy=dev(dyv), dpooled=dev(dpool), dh_n=dev(dhn), dx=dxd)
    rnn.check()
    ref = bigru(c['x'], c['P'], PREFIX, 2, pool='mean', dy=dyv, dpooled=dpool, dhn=dhn, masks=[mask])
    check_against(dict(rnn=rnn, y=c['y'], pooled=c['pooled'], h_n=c['h_n'], dx=dxd, G=Gd, names=c['names']), ref)


def test_bigru_dropout_only_forward_gives_the_train_forwards_bits(gemm_mode):
    B, T, F, H, p, seed = 19, 11, 40, 48, 0.5, 99
    tr = dropout_case(B, T, F, H, p, seed, L.RUN_TRAIN, 5)
    do = dropout_case(B, T, F, H, p, seed, L.RUN_DROPOUT_ONLY, 5)
    tr['rnn'].check(); do['rnn'].check()
    for k in ('y', 'pooled', 'h_n'):
        assert torch.isfinite(tr[k]).all(), k
        assert torch.equal(tr[k], do[k]), k
    Gd = [torch.empty_like(w) for w in do['Wd']]
    with pytest.raises(L.DepError, match='DEP_RUN_TRAIN'):
        do['rnn'].backward(do['xd'], do['Wd'], Gd, dpooled=do['pooled'])


# ----------------------------------------------------------------------------- ragged
RAGGED_CASES = [(19, 11, 40, 48), (33, 6, 16, 256), (48, 5, 8, 16)]


@pytest.mark.parametrize('B,T,F,H', RAGGED_CASES)
def test_bigru_ragged_stack_fwd_bwd(B, T, F, H, gemm_mode):
    """The reverse direction of row b starts at t = len_b - 1; dead positions of every layer's y and of dx are exactly 0.0; dh_n
    enters at the row's last step in sweep order; an empty row contributes nothing and its h_n is 0."""
    rng = np.random.default_rng(B * 1000 + T * 100 + F + H)
    lengths = lengths_mix(B, T, rng)
    assert (lengths == 0).any() and (lengths == T).any()
    out, ref, inst = run_stack(B, T, F, H, 2, 'full', rng, lengths=lengths)
    check_against(out, ref)
    only_bi_tile_instances(inst, ragged=True)
    pad = out['pad']
    assert not bits(out['y'])[pad].any(), 'y is not exactly 0.0 at dead positions'
    assert not bits(out['rnn'].layer_output(0))[pad].any(), 'layer 0 output is not exactly 0.0 at dead positions'
    assert not bits(out['dx'])[pad].any(), 'dx is not exactly 0.0 at dead positions'
    assert not bits(out['h_n'])[:, lengths == 0].any(), 'h_n of an empty row is not 0'
    assert not bits(out['pooled'])[lengths == 0].any(), 'the pool of an empty row is not 0'


@pytest.mark.parametrize('B,T,F,H', RAGGED_CASES)
def test_bigru_all_lengths_T_gives_the_dense_calls_bits(B, T, F, H, gemm_mode):
    res = []
    for lengths in (None, np.full(B, T, np.int32)):
        out, _, inst = run_stack(B, T, F, H, 2, 'full', np.random.default_rng(B + T + H), lengths=lengths)
        only_bi_tile_instances(inst, ragged=lengths is not None)
        res.append([('y', out['y'].clone()), ('pooled', out['pooled']), ('h_n', out['h_n']), ('dx', out['dx'])] + list(zip(out['names'], out['G'])))
    for (nm, a), (_, b) in zip(*res):
        assert torch.isfinite(a).all(), nm
        assert torch.equal(a, b), nm


# ----------------------------------------------------------------------------- refusals
def test_bigru_refusals():
    """No generic and no cluster instances: impl 1 / 3 and every H the tile sweeps cannot run are bad descriptors, with the rule in
    the message."""
    for impl in (1, 3):
        with pytest.raises(L.DepError, match='tile-MFMA'):
            L.Rnn(L.CELL_GRU, 4, 4, 8, 16, 2, 2, True, 0.0, L.POOL_MEAN, DEV, impl=impl)
    with pytest.raises(L.DepError, match='multiple of 16'):
        L.Rnn(L.CELL_GRU, 4, 4, 8, 80, 2, 2, True, 0.0, L.POOL_MEAN, DEV)
    # the entry points themselves: DEP_ERR_ARG and the same message (a descriptor changed behind a good object's back)
    rng = np.random.default_rng(0)
    P, names = make_params(rng, 8, 16, 2)
    Wd = [dev(P[n]) for n in names]
    rnn = L.Rnn(L.CELL_GRU, 4, 4, 8, 16, 2, 2, True, 0.0, L.POOL_MEAN, DEV)
    x = dev(rng.standard_normal((4, 4, 8))); pooled = torch.empty(4, 32, device=DEV)
    rnn.forward(x, Wd, pooled=pooled)
    rnn.desc.impl = 3
    with pytest.raises(L.DepError, match=r'\(-1\).*multiple of 16'):
        rnn.forward(x, Wd, pooled=pooled)
    with pytest.raises(L.DepError, match=r'\(-1\).*multiple of 16'):
        rnn.backward(x, Wd, [torch.empty_like(w) for w in Wd], dpooled=pooled)
    rnn.desc.impl = 0
    rnn.forward(x, Wd, pooled=pooled)
    rnn.check()
