"""GPU parity of impl = 7, the per-layer cluster sweeps of a bidirectional GRU, forward and backward: the forward is impl = 6's, the
backward one launch per layer and batch chunk of gru_bwd_cluster_r1<NTW, SPLIT, KB, false, false, AG, RAG, true>.

Expectations: tests/bigru_ref.py for the plain call, tests/hx_ref.py for a dense call with state, tests/state_varlen_ref.py for a
ragged call with state.  Tolerances are the project's own for every recurrent path: 1e-4 absolute on y / pooled / h_n, 1e-4 relerr
on dx, dhx and every weight and bias gradient.  Where the same call also runs on impl = 6 (H <= 256) the forward outputs and the
dropout masks are bit-equal and the gradients within 2e-4 (relerr) of each other.  Every case fills outputs and gradient buffers
with NaN, ends with rnn.check() and status word 0, and asserts through the enqueue-order log that the backward sweeps are exactly the
expected instance, once per layer and chunk, and that no gru_bwd_mfma ran.

Which case reaches which of the 16 table rows (NTW = H / 64; exact = mode f32, split = mode bf16x3):
  <1|2, false|true, 4, .., false, false, true>   H 64 / 128, dense:   test_dense_grid, test_burst_phases[dense] (H 64), test_header_slots (H 64)
  <1|2, false|true, 4, .., false, true,  true>   H 64 / 128, ragged:  test_ragged, test_burst_phases[ragged] (H 64)
  <4, false, 4, .., false, false|true, true>     H 256 exact:         test_dense_grid / test_ragged, test_two_launch_chunks (dense)
  <4, true,  4, .., true,  false|true, true>     H 256 split (AG):    test_dense_grid / test_ragged, test_two_launch_chunks (dense)
  <8, false|true, 0, .., false, false|true, true> H 512:              test_dense_grid / test_ragged, test_two_launch_chunks, test_h512_trains
The state, aliasing and determinism cases run the same rows again.
Run on the MI355X box:  python -m pytest tests/test_bigru_cluster_bwd_gpu.py -m gpu -q"""
import numpy as np
import pytest

import hx_ref
import state_varlen_ref as svr
import test_bigru_cluster_gpu as base
from bigru_ref import bigru
from varlen_ref import lengths_mix

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

ATOL, RTOL, NAN, PREFIX = base.ATOL, base.RTOL, base.NAN, base.PREFIX
dev, idev, host, bits, f32, nans, pad_mask, ident = base.dev, base.idev, base.host, base.bits, base.f32, base.nans, base.pad_mask, base.ident
gemm_mode = base.gemm_mode
HS = [64, 128, 256, 512]


def case_rng(*v):
    return np.random.default_rng(7000 + sum(int(a) * 7 ** i for i, a in enumerate(v)))


def backward_instance(H, split, ragged):
    ag = H == 256 and split
    return 'gru_bwd_cluster_r1<%d, %s, %d, false, false, %s, %s, true>' % (H // 64, 'true' if split else 'false', 0 if H == 512 else 4,
                                                                           'true' if ag else 'false', 'true' if ragged else 'false')


def chunks(H, B):
    per = base.chunk_utterances(H)
    return (B + per - 1) // per


def make_rnn(B, T, F, H, Lyr, p, pool, impl):
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, Lyr, 2, L.RUN_TRAIN, p, base.POOLS[pool], DEV, impl=impl)
    rnn.reserve.fill_(NAN)
    assert rnn.status_word() is not None
    return rnn


def problem(B, T, F, H, Lyr, rng, lengths=None, state=False, pool='mean'):
    """Parameters and inputs of one training step: dy, dpooled and dh_n all non-zero; a ragged call gets NaN in dy behind each length."""
    P, names = base.make_params(rng, F, H, Lyr)
    x = f32(rng.standard_normal((B, T, F)))
    pad = None
    if lengths is not None:
        pad = pad_mask(lengths, T)
        x[pad] = 0.0
    q = dict(B=B, T=T, F=F, H=H, Lyr=Lyr, P=P, names=names, x=x, pad=pad, lengths=lengths, pool=pool,
             dy=f32(rng.standard_normal((B, T, 2 * H)) * 0.3), dpool=f32(rng.standard_normal((B, 2 * H))),
             dhn=f32(rng.standard_normal((2 * Lyr, B, H)) * 0.3), hx=f32(rng.standard_normal((2 * Lyr, B, H)) * 0.6) if state else None)
    return q


def step(q, impl, p=0.0, seed=0, alias=False):
    """One DEP_RUN_TRAIN forward + backward.  alias: dhx is dh_n's tensor.  Returns the device results and the sweeps of each call."""
    B, T, F, H, Lyr = q['B'], q['T'], q['F'], q['H'], q['Lyr']
    Wd = [dev(q['P'][n]) for n in q['names']]
    Gd = [torch.full_like(w, NAN) for w in Wd]
    xd = dev(q['x'])
    ld = None if q['lengths'] is None else idev(q['lengths'])
    hxd = None if q['hx'] is None else dev(q['hx'])
    dy_in = q['dy'].copy()
    if q['pad'] is not None:
        dy_in[q['pad']] = np.nan
    rnn = make_rnn(B, T, F, H, Lyr, p, q['pool'], impl)
    pooled, h_n, dxd = nans(B, 2 * H), nans(2 * Lyr, B, H), nans(B, T, F)
    dhnd = dev(q['dhn'])
    dhxd = None if hxd is None else (dhnd if alias else nans(2 * Lyr, B, H))
    with base.launched() as kf:
        if ld is not None and hxd is not None:
            rnn.forward_state_varlen(xd, Wd, ld, seed=seed, pooled=pooled, h_n=h_n, hx=hxd)
        else:
            rnn.forward(xd, Wd, seed=seed, pooled=pooled, h_n=h_n, lengths=ld, hx=hxd)
    with base.launched() as kb:
        bw = dict(dy=dev(dy_in), dpooled=dev(q['dpool']), dh_n=dhnd, dx=dxd)
        if hxd is not None and ld is not None:
            rnn.backward_state_varlen(xd, Wd, Gd, ld, hx=hxd, dhx=dhxd, **bw)
        elif hxd is not None:
            rnn.backward(xd, Wd, Gd, hx=hxd, dhx=dhxd, **bw)
        else:
            rnn.backward(xd, Wd, Gd, lengths=ld, **bw)
    base.healthy(rnn)
    return dict(rnn=rnn, y=rnn.layer_output(), pooled=pooled, h_n=h_n, dx=dxd, dhx=dhxd, G=Gd, names=q['names'], fwd=kf.sweeps, bwd=kb.sweeps)


def oracle(q, p=0.0, seed=0):
    B, T, H, Lyr = q['B'], q['T'], q['H'], q['Lyr']
    masks = base.state_masks(B, T, H, Lyr, p, seed) if p > 0 else None
    kw = dict(pool=q['pool'], dy=q['dy'], dpooled=q['dpool'], dhn=q['dhn'], masks=masks)
    if q['hx'] is not None and q['lengths'] is not None:
        ref = svr.stack(q['x'], q['lengths'], q['P'], PREFIX, 'gru', 2, Lyr, hx=q['hx'], **kw)
    elif q['hx'] is not None:
        ref = hx_ref.stack(q['x'], q['P'], PREFIX, 'gru', 2, Lyr, hx=q['hx'], **kw)
    else:
        ref = bigru(q['x'], q['P'], PREFIX, Lyr, lengths=q['lengths'], **kw)
    return ref, masks


def check_sweeps(out, q, split):
    H, ragged = q['H'], q['lengths'] is not None
    n = q['Lyr'] * chunks(H, q['B'])
    assert out['fwd'] == [base.forward_instance(H, split, ragged)] * n, out['fwd']
    assert out['bwd'] == [backward_instance(H, split, ragged)] * n, out['bwd']      # exactly these: no gru_bwd_mfma, nothing else
    assert not any('gru_bwd_mfma' in s for s in out['fwd'] + out['bwd'])


def check_masks(out, masks, Lyr):
    """The masks fed to the oracle are the ones in the reserve: dropout(y_l) is y_l * mask_l bit for bit."""
    for l in range(Lyr - 1):
        assert set(np.unique(masks[l])).issubset({0.0, 2.0}) and 0.3 < (masks[l] == 0).mean() < 0.7
        assert torch.equal(out['rnn'].layer_output_dropped(l), out['rnn'].layer_output(l) * dev(masks[l])), f'dropout(y{l}) is not y{l} * mask'


def gradient_pairs(out, ref):
    g = [(n, host(t), ref['G'][n]) for n, t in zip(out['names'], out['G'])] + [('dx', host(out['dx']), ref['dx'])]
    if out['dhx'] is not None:
        g.append(('dhx', host(out['dhx']), ref['dhx']))
    return g


def check_against_oracle(what, out, ref, q):
    base.close(what, base.forward_pairs(out, out['rnn'], ref, q['Lyr']))
    pairs = gradient_pairs(out, ref)
    # one step from a zero state: h_prev is 0, so dW_hh is 0 in the oracle -- no scale for a relative error; the device value is held to exactly 0
    zero = [pr for pr in pairs if not np.asarray(pr[2]).any()]
    for n, a, _ in zero:
        assert q['T'] == 1 and q['hx'] is None and 'weight_hh' in n, f'{n}: the reference gradient is trivially zero'
        assert np.isfinite(a).all() and not a.any(), f'{what}: {n} is not exactly 0 at T = 1 without a state'
    base.close_rel(what, [pr for pr in pairs if np.asarray(pr[2]).any()])
    if q['pad'] is not None:
        assert not bits(out['dx'])[q['pad']].any(), 'dx is not exactly 0.0 behind a length'
        assert not bits(out['y'])[q['pad']].any()


def check_against_impl6(what, out, q, p=0.0, seed=0, alias=False):
    """The same call on impl = 6 (the tile-MFMA backward behind the same forward): forward outputs and dropout masks bit for bit,
    gradients within 2e-4 of each other."""
    o6 = step(q, 6, p=p, seed=seed, alias=alias)
    assert all('gru_bwd_mfma' in s for s in o6['bwd']) and o6['bwd']
    assert o6['fwd'] == out['fwd']
    for k in ('y', 'pooled', 'h_n'):
        assert np.array_equal(bits(out[k]), bits(o6[k])), f'{what}: {k} differs from impl = 6'
    for l in range(q['Lyr']):
        assert np.array_equal(bits(out['rnn'].layer_output(l)), bits(o6['rnn'].layer_output(l))), f'{what}: layer {l} output differs from impl = 6'
        if p > 0 and l < q['Lyr'] - 1:
            assert np.array_equal(bits(out['rnn'].layer_output_dropped(l)), bits(o6['rnn'].layer_output_dropped(l))), f'{what}: mask {l}'
    pairs = [(n, host(a), host(b)) for n, a, b in zip(out['names'], out['G'], o6['G'])] + [('dx', host(out['dx']), host(o6['dx']))]
    if out['dhx'] is not None:
        pairs.append(('dhx', host(out['dhx']), host(o6['dhx'])))
    for n, a, b in pairs:
        if not b.any():      # (dW_hh of one step from a zero state: exactly 0 on both plans)
            assert q['T'] == 1 and q['hx'] is None and 'weight_hh' in n and not a.any(), f'{what}: {n}'
    base.close_rel(what + ' against impl = 6', [pr for pr in pairs if pr[2].any()], tol=2 * RTOL)


def run_case(what, q, mode, p=0.0, seed=0, alias=False):
    out = step(q, 7, p=p, seed=seed, alias=alias)
    ref, masks = oracle(q, p=p, seed=seed)
    if p > 0:
        check_masks(out, masks, q['Lyr'])
    check_sweeps(out, q, mode == 'bf16x3')
    check_against_oracle(f'{what} {mode}', out, ref, q)
    if q['H'] <= 256:
        check_against_impl6(f'{what} {mode}', out, q, p=p, seed=seed, alias=alias)
    return out, ref


# ----------------------------------------------------------------------------- dense grid
# (B, T, F, layers, p, pool): T = 1 has no exchange step | T = 2, 3 lie inside the burst prologue (T < KB) | T = 9: two bursts and a
# tail, T odd, three batch tiles
GRID = [(3, 1, 8, 1, 0.0, 'mean'), (5, 2, 8, 2, 0.5, 'sum'), (19, 3, 12, 2, 0.5, 'mean'), (37, 9, 8, 2, 0.5, 'sum')]


@pytest.mark.parametrize('shape', GRID, ids=ident)
@pytest.mark.parametrize('H', HS)
def test_dense_grid(H, shape, gemm_mode):
    B, T, F, Lyr, p, pool = shape
    q = problem(B, T, F, H, Lyr, case_rng(B, T, F, H, Lyr), pool=pool)
    run_case(f'dense H={H} {ident(shape)}', q, gemm_mode, p=p, seed=1234 + B)


# ----------------------------------------------------------------------------- ragged
def ragged_lengths(B, T, rng):
    """lengths_mix (T, 1, 0 in rows 0..2, a full row 15) with T-1 in row 3, the second tile all zeros and, where there is a third
    tile, every row of it shorter than T.  (B = 19 has two tiles: the zero tile is its short one.)"""
    n = lengths_mix(B, T, rng)
    n[3] = T - 1
    n[16:32] = 0
    if B > 32:
        n[32:] = rng.integers(1, T, B - 32)
        n[32] = T - 1
    assert {0, 1, T - 1, T} <= set(n.tolist()) and not n[16:32].any() and (n[32:] < T).all()
    return n


@pytest.mark.parametrize('shape', [(19, 5, 'mean'), (37, 9, 'sum')], ids=ident)
@pytest.mark.parametrize('H', HS)
def test_ragged(H, shape, gemm_mode):
    """live = t < len in both directions; direction 1's dead steps come at the end of its backward sweep.  dx behind each length is
    exactly 0 (checked in check_against_oracle)."""
    B, T, pool = shape
    rng = case_rng(B, T, H, 1)
    q = problem(B, T, 12, H, 2, rng, lengths=ragged_lengths(B, T, rng), pool=pool)
    run_case(f'ragged H={H} {ident(shape)}', q, gemm_mode, p=0.5, seed=77 + B)


# ----------------------------------------------------------------------------- burst phases, launch chunks, header slots
@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_burst_phases(ragged, gemm_mode):
    """25 batch tiles in one launch: tiles bt >= 8, 16, 24 take the dirty-step phases 1, 2, 3, and block -> (member, direction, tile)
    is the pair mapping at nbtp = 32."""
    B, T, F, H = 389, 6, 8, 64
    rng = case_rng(B, T, H, 2, ragged)
    lengths = lengths_mix(B, T, rng) if ragged else None
    assert chunks(H, B) == 1
    q = problem(B, T, F, H, 1, rng, lengths=lengths)
    run_case(f'burst phases {"ragged" if ragged else "dense"}', q, gemm_mode)


@pytest.mark.parametrize('H,B', [(512, 130), (256, 260)])
def test_two_launch_chunks(H, B, gemm_mode):
    """Two directions halve the tiles of one co-resident launch under the 256-workgroup cap: these batches take two."""
    q = problem(B, 2, 8, H, 1, case_rng(B, H, 3))
    assert chunks(H, B) >= 2
    run_case(f'two chunks H={H} B={B}', q, gemm_mode)


def test_header_slots(gemm_mode):
    """One layer more than there are exchange-header slots: the deepest layers share slot 0 and clear it themselves."""
    Lyr = 5                                       # DEP_HDR_SLOTS + 1 (csrc/dep_common.h)
    q = problem(5, 3, 8, 64, Lyr, case_rng(5, 3, 64, 4))
    run_case('header slots', q, gemm_mode)


# ----------------------------------------------------------------------------- state
@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('T', [4, 1])
@pytest.mark.parametrize('H', [64, 256, 512])
def test_state(H, T, ragged, gemm_mode):
    """hx in, dhx out.  Ragged: lengths_mix has rows of length 0 (dhx = dh_n) and rows of length T, whose direction-1 recurrent term is
    the product behind the sweep; the others end their reverse sweep in dead steps and get it in-kernel."""
    B, F, Lyr = 19, 12, 2
    rng = case_rng(B, T, H, 5, ragged)
    lengths = lengths_mix(B, T, rng) if ragged else None
    q = problem(B, T, F, H, Lyr, rng, lengths=lengths, state=True)
    out, ref = run_case(f'state H={H} T={T} {"ragged" if ragged else "dense"}', q, gemm_mode, p=0.5, seed=4321)
    assert np.abs(ref['dhx']).max() > 0
    if ragged:
        assert (lengths == 0).any() and (lengths == T).any()
        empty = lengths == 0
        assert np.array_equal(bits(out['dhx'])[:, empty], bits(dev(q['dhn']))[:, empty]), 'len 0: dhx is dh_n bit for bit'


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_dhx_may_alias_dh_n(ragged, gemm_mode):
    B, T, F, H, Lyr = 19, 4, 12, 256, 2
    rng = case_rng(B, T, H, 6, ragged)
    lengths = lengths_mix(B, T, rng) if ragged else None
    q = problem(B, T, F, H, Lyr, rng, lengths=lengths, state=True)
    apart = step(q, 7)
    over = step(q, 7, alias=True)
    ref, _ = oracle(q)
    check_sweeps(over, q, gemm_mode == 'bf16x3')
    check_against_oracle(f'dhx over dh_n {gemm_mode}', over, ref, q)
    assert np.array_equal(bits(apart['dhx']), bits(over['dhx'])), 'dhx written over dh_n differs'
    for n, a, b in zip(q['names'], apart['G'], over['G']):
        assert np.array_equal(bits(a), bits(b)), n


# ----------------------------------------------------------------------------- determinism, H = 512
@pytest.mark.parametrize('H', [128, 256, 512])      # burst reduce-scatter | (split mode) all-gather | round-1 schedule
def test_a_second_run_gives_the_same_bits(H, gemm_mode):
    B, T = 37, 9
    rng = case_rng(B, T, H, 7)
    q = problem(B, T, 8, H, 2, rng, lengths=ragged_lengths(B, T, rng), state=True)
    a, b = step(q, 7, p=0.5, seed=5), step(q, 7, p=0.5, seed=5)
    assert a['bwd'] == b['bwd'] == [backward_instance(H, gemm_mode == 'bf16x3', True)] * 2
    for n, x, y in [(n, g, h) for n, g, h in zip(q['names'], a['G'], b['G'])] + [('dx', a['dx'], b['dx']), ('dhx', a['dhx'], b['dhx'])]:
        assert torch.isfinite(x).all(), n
        assert np.array_equal(bits(x), bits(y)), n


def test_h512_trains(gemm_mode):
    """No device comparator at H = 512 (the tile sweeps stop at 256): the oracle alone."""
    B, T, F, H, Lyr = 5, 3, 8, 512, 2
    q = problem(B, T, F, H, Lyr, case_rng(B, T, F, H, Lyr, 8))
    out, ref = run_case('H = 512 trains', q, gemm_mode)
    with pytest.raises(L.DepError, match='forward only'):
        r6 = make_rnn(B, T, F, H, Lyr, 0.0, 'mean', 6)
        r6.backward(dev(q['x']), [dev(q['P'][n]) for n in q['names']], out['G'], dpooled=out['pooled'])
