"""GPU parity of the recurrent stacks beyond two layers and beyond the two model shapes: depth 1 / 3 / 5 / 8 on every kernel family,
the unidirectional LSTM (forward AND backward, generic / tile-MFMA / cluster), dh_n in every layer, two dropout sites, each gradient
input alone, ragged calls at the new depths, and the exchange-header slots past DEP_HDR_SLOTS (layers 4 .. 7 of a cluster stack).

The expectation is tests/stack_ref.py, a composition of the unchanged oracle's layer functions (pinned against stock torch.nn.GRU /
torch.nn.LSTM float64 autograd in tests/test_stack_ref_cpu.py).  Bars are the project's own (include/dep_rnn.h,
tests/test_varlen_gpu.py): 1e-4 absolute on EVERY layer's output, y, pooled and h_n of every layer and direction; 1e-4 relerr on dx and
every gradient tensor.  The reserve, pooled, h_n, dx and the gradient tensors are pre-filled with NaN; in a ragged call dy is NaN at
padded positions; dep_rnn_status is read after the step.  Around every case the launch-instance log says which sweeps ran: a cluster
case must not pass on tile kernels, and no fused two-layer launch may appear where L != 2.
Every check prints its worst figures ('stack-depth <section> ...'; pytest -s shows them).
Run on the MI355X box:  python -m pytest tests/test_stack_depth_gpu.py -m gpu -q"""
import re

import numpy as np
import pytest

from stack_ref import stack
from varlen_ref import lengths_mix

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

ATOL = 1e-4
RTOL = 1e-4
PREFIX = 'rnn'


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


def make_params(rng, cell, F, H, Lyr, dirs):
    """Weights in the header's order: layer l, direction d -> weight_ih (G H, in), weight_hh (G H, H), bias_ih, bias_hh; in = F | dirs H."""
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
    """Both precision modes of the parity path (forced on every contraction size), as in tests/test_varlen_gpu.py."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


def sweep_instances(log):
    return {re.sub(r'^\(|\)$', '', re.sub(r' @ .*$', '', s)) for s in log if re.search(r'(gru|lstm)2?_(fwd|bwd)_', s)}


FAMILY = {   # what a case of (cell, impl) may launch as its sweeps; impl 3 at L = 2, H = 256 adds the fused two-layer launches
    ('gru', 1): r'gru_(fwd|bwd)_generic<.*>', ('gru', 2): r'gru_(fwd|bwd)_mfma<.*>', ('gru', 3): r'gru_(fwd_cluster_r1|fwd_cluster16|bwd_cluster_r1)<.*>',
    ('lstm', 1): r'lstm_(fwd|bwd)_generic<.*>', ('lstm', 2): r'lstm_(fwd|bwd)_mfma<.*>', ('lstm', 3): r'lstm_(fwd|bwd)_cluster<.*>',
}


# the ragged instances: RAG = true is the last template argument, behind all the others written out
RAGGED_INSTANCE = (r'gru_fwd_cluster_r1<(\w+, ){2}true>|gru_bwd_cluster_r1<(\w+, ){6}true>|lstm_(fwd|bwd)_cluster<(\w+, ){2}true>|'
                   r'(gru|lstm)_(fwd|bwd)_mfma<\d, true>')


def check_family(inst, cell, impl, Lyr, H, first_run=True):
    """Every sweep the call launched is of the family the case is named for, forward and backward both (the log keeps an instance once
    per test: a second run of the same descriptor inside one test records nothing new and is not asked for both)."""
    pat = FAMILY[(cell, impl)]
    fused_ok = cell == 'gru' and impl == 3 and Lyr == 2 and H == 256
    for s in inst:
        if fused_ok and re.fullmatch(r'gru2_(fwd|bwd)_fused<.*>', s):
            continue
        assert 'gru2_' not in s or fused_ok, f'a fused two-layer launch at L = {Lyr}, H = {H}: {sorted(inst)}'
        assert re.fullmatch(pat, s), f'{cell} impl {impl}: {s} is not of the family of this case ({sorted(inst)})'
    if first_run:
        kinds = {re.search(r'_(fwd|bwd)_', s).group(1) for s in inst}
        assert kinds == {'fwd', 'bwd'}, f'no forward or no backward sweep was recorded: {sorted(inst)}'


def run_stack(cell, dirs, B, T, F, H, Lyr, impl, rng, grads=('dy', 'dpooled', 'dhn'), want_dx=True, lengths=None, p=0.0, seed=0,
              pool_kind='mean'):
    """One forward + backward of a stack.  grads: which of dy / dpooled / dhn go in (dpooled: GRU only; dhn is non-zero in EVERY layer
    and direction; NaN at the dead positions of dy in a ragged call: they are ignored).  Returns (device tensors, reference, sweeps)."""
    gru = cell == 'gru'
    grads = tuple(g for g in grads if gru or g != 'dpooled')
    W = H * dirs
    P, names = make_params(rng, cell, F, H, Lyr, dirs)
    x = f32(rng.standard_normal((B, T, F)))
    pad = None
    if lengths is not None:
        pad = pad_mask(lengths, T)
        x[pad] = 0.0                                                   # the padding is finite (zeros)
    Wd = [dev(P[n]) for n in names]
    Gd = [torch.full_like(w, float('nan')) for w in Wd]
    xd = dev(x)
    ld = None if lengths is None else idev(lengths)
    pool = (L.POOL_MEAN if pool_kind == 'mean' else L.POOL_SUM) if gru else L.POOL_NONE
    rnn = L.Rnn(L.CELL_GRU if gru else L.CELL_LSTM, B, T, F, H, Lyr, dirs, True, p, pool, DEV, impl=impl)
    assert (rnn.status_word() is not None) == (impl == 3)
    rnn.reserve.fill_(float('nan'))
    pooled = torch.full((B, W), float('nan'), device=DEV) if gru else None
    h_n = torch.full((Lyr * dirs, B, H), float('nan'), device=DEV)
    before = L.instance_log_read()
    rnn.forward(xd, Wd, seed=seed, pooled=pooled, h_n=h_n, lengths=ld)
    masks = None
    if p > 0:
        masks = [host(L.dropout_mask(B * T * W, p, seed, 16 + l, DEV)).reshape(B, T, W) for l in range(Lyr - 1)]      # site = DEP_SITE_RNN0 + l
    dyv = f32(rng.standard_normal((B, T, W)) * 0.3)
    dpool = f32(rng.standard_normal((B, W)))
    dhn = f32(rng.standard_normal((Lyr * dirs, B, H)) * 0.3)
    dy_in = dyv.copy()
    if pad is not None:
        dy_in[pad] = np.nan
    dxd = torch.full((B, T, F), float('nan'), device=DEV) if want_dx else None
    rnn.backward(xd, Wd, Gd, dy=dev(dy_in) if 'dy' in grads else None, dpooled=dev(dpool) if 'dpooled' in grads else None,
                 dh_n=dev(dhn) if 'dhn' in grads else None, dx=dxd, lengths=ld)
    rnn.check()
    inst = sweep_instances(L.instance_log_read() - before)
    ref = stack(x, P, PREFIX, cell, dirs, Lyr, lengths=lengths, pool=pool_kind if gru else 'none', dy=dyv if 'dy' in grads else None,
                dpooled=dpool if 'dpooled' in grads else None, dhn=dhn if 'dhn' in grads else None, masks=masks)
    out = dict(rnn=rnn, y=rnn.layer_output(), pooled=pooled, h_n=h_n, dx=dxd, G=Gd, names=names, pad=pad, masks=masks, lengths=lengths)
    return out, ref, inst


def check_against(out, ref, section, what=''):
    """The first tensor off its bar fails the test, lower layers first; the worst figures are printed before any assertion."""
    rnn = out['rnn']
    Lyr, dirs, H = rnn.desc.L, rnn.desc.dirs, rnn.desc.H
    outs = [(f'layer {l} output', host(rnn.layer_output(l)), yl) for l, yl in enumerate(ref['ys'])]
    outs.append(('y', host(out['y']), ref['y']))
    hn = host(out['h_n'])
    outs += [(f'h_n[layer {i // dirs}, direction {i % dirs}]', hn[i], ref['h_n'][i]) for i in range(Lyr * dirs)]
    if out['pooled'] is not None:
        outs.append(('pooled', host(out['pooled']), ref['pooled']))
    gr = []
    for l in range(Lyr - 1, -1, -1):                                   # the order the backward forms them: the first layer that is off
        for n, g in zip(out['names'], out['G']):
            if re.search(r'_l%d(_reverse)?$' % l, n):
                gr.append((n, host(g), ref['G'][n]))
    if out['dx'] is not None:
        gr.append(('dx', host(out['dx']), ref['dx']))
    assert len(gr) == len(out['G']) + (out['dx'] is not None)
    ea = [(float(np.abs(a - b).max()) if np.isfinite(a).all() else float('nan'), n) for n, a, b in outs]
    er = [(float(relerr(a, b)) if np.isfinite(a).all() else float('nan'), n) for n, a, b in gr]
    worst = lambda e: max(e, key=lambda v: float('inf') if v[0] != v[0] else v[0])
    print(f'stack-depth {section} {what}: worst abs {worst(ea)[0]:.3e} ({worst(ea)[1]}), worst rel {worst(er)[0]:.3e} ({worst(er)[1]})')
    for e, n in ea:
        assert e < ATOL, f'{n}: {e:.3e}'
    for (e, n), (_, _, b) in zip(er, gr):
        # (the reference gradient is not trivially zero -- but for dW_hh of a one-step sweep, h_prev = 0: the device's must be 0 too)
        assert np.abs(b).max() > 0 or ('weight_hh' in n and rnn.desc.T == 1), n
        assert e < RTOL, f'{n}: {e:.3e}'


def check_dead_positions(out):
    """Ragged calls: exact 0.0 bits at dead positions of y, every layer's output and dx; an empty row's h_n and pool are 0."""
    pad, lengths, rnn = out['pad'], out['lengths'], out['rnn']
    assert not bits(out['y'])[pad].any(), 'y is not exactly 0.0 at dead positions'
    for l in range(rnn.desc.L):
        assert not bits(rnn.layer_output(l))[pad].any(), f'layer {l} output is not exactly 0.0 at dead positions'
    if out['dx'] is not None:
        assert not bits(out['dx'])[pad].any(), 'dx is not exactly 0.0 at dead positions'
    assert not bits(out['h_n'])[:, lengths == 0].any(), 'h_n of an empty row is not 0'
    if out['pooled'] is not None:
        assert not bits(out['pooled'])[lengths == 0].any(), 'the pool of an empty row is not 0'


def case_rng(*v):
    return np.random.default_rng(sum(int(a) * 7 ** i for i, a in enumerate(v)))


ident = lambda c: '-'.join(str(v) for v in c)

# ----------------------------------------------------------------------------- a. depth 1 and 3 on every kernel family
# (cell, dirs, B, T, F, H, L, impl).  Generic; tile-MFMA (jpw 3 and 2, a ragged second tile); cluster GRU at every member count
# (H = 64 .. 512; even T = the PK gate-gradient image, odd T = fp32 rows; B = 20: a ragged second tile; H = 256 is the per-layer
# cluster kernels as the planned path, dep_fused2_ok needs L = 2; H = 512 at L = 3 only); cluster LSTM with both and with ONE direction
# (half the members: a geometry no other oracle test reaches).
DEPTH_CASES = [(c, d, 4, 6, 5, 8, Ly, 1) for c, d in (('gru', 1), ('lstm', 2), ('lstm', 1)) for Ly in (1, 3)]
DEPTH_CASES += [c + (Ly, 2) for c in (('gru', 1, 19, 7, 12, 48), ('lstm', 2, 19, 5, 16, 32), ('lstm', 1, 19, 5, 16, 32)) for Ly in (1, 3)]
DEPTH_CASES += [('gru', 1, 20, T, 12, H, Ly, 3) for H in (64, 128, 256, 512) for Ly in (1, 3) for T in (6, 7) if not (H == 512 and Ly == 1)]
DEPTH_CASES += [('lstm', d, 19, T, 40, 128, Ly, 3) for d in (2, 1) for Ly in (1, 3) for T in (6, 7)]
# 'model' form (GRU: dpooled only, no dx; LSTM: dy + dh_n, no dx) on a cut of the cluster cases
MODEL_CASES = [('gru', 1, 20, 7, 12, 64, 1, 3), ('gru', 1, 20, 6, 12, 128, 3, 3), ('gru', 1, 20, 6, 12, 256, 3, 3),
               ('lstm', 1, 19, 7, 40, 128, 1, 3), ('lstm', 1, 19, 6, 40, 128, 3, 3), ('lstm', 2, 19, 7, 40, 128, 3, 3)]
FORM_CASES = [c + ('full',) for c in DEPTH_CASES] + [c + ('model',) for c in MODEL_CASES]


@pytest.mark.parametrize('case', FORM_CASES, ids=ident)
def test_depth_1_and_3_on_every_kernel_family(case, gemm_mode):
    cell, dirs, B, T, F, H, Lyr, impl, form = case
    full = form == 'full'
    grads = ('dy', 'dpooled', 'dhn') if full else (('dpooled',) if cell == 'gru' else ('dy', 'dhn'))
    out, ref, inst = run_stack(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, B, T, F, H, Lyr, impl), grads=grads, want_dx=full,
                               pool_kind='mean' if full else 'sum')
    check_against(out, ref, 'a', ident(case))
    check_family(inst, cell, impl, Lyr, H)


# ----------------------------------------------------------------------------- b. the plain nn.LSTM(bidirectional=False) user
# L = 2 on all three impls; the cluster sweeps at T = 1 and at T = burst + 1
UNI_LSTM_CASES = [('lstm', 1, 6, 20, 24, 16, 2, 1), ('lstm', 1, 6, 20, 24, 16, 2, 2), ('lstm', 1, 19, 11, 40, 128, 2, 3),
                  ('lstm', 1, 2, 1, 8, 128, 2, 3), ('lstm', 1, 40, 5, 8, 128, 2, 3)]


@pytest.mark.parametrize('case', UNI_LSTM_CASES, ids=ident)
def test_unidirectional_lstm_two_layers(case, gemm_mode):
    cell, dirs, B, T, F, H, Lyr, impl = case
    out, ref, inst = run_stack(cell, dirs, B, T, F, H, Lyr, impl, case_rng(B, T, F, H, impl))
    check_against(out, ref, 'b', ident(case))
    check_family(inst, cell, impl, Lyr, H)


# ----------------------------------------------------------------------------- c. past the exchange-header slots
# DEP_HDR_SLOTS = 4: layers 4 .. 7 of a cluster stack share header slot 0 with layer 0 and clear it themselves; a batch of more than
# one chunk clears its slot in front of every chunk but the first.
SLOT_CASES = [('gru', 1, 20, 5, 8, 128, 5, 3), ('gru', 1, 20, 4, 8, 256, 5, 3), ('lstm', 2, 20, 5, 8, 128, 5, 3), ('lstm', 1, 20, 5, 8, 128, 5, 3),
              ('gru', 1, 5, 3, 8, 128, 8, 3), ('gru', 1, 530, 3, 8, 256, 3, 3)]


@pytest.mark.parametrize('case', SLOT_CASES, ids=ident)
def test_stacks_past_the_header_slots(case, gemm_mode):
    """Regression: dep_rnn_backward walks the layers downwards, so layer 0 came to header slot 0 AFTER layers 4 .. L-1 had used it and
    still took it for clean.  With the stale flag / hello words every wait of its sweep passed at once; (gru, H = 256, L = 5) in
    bf16x3 mode then gave layer 0's weight gradients 2.7e-2 off (every other tensor within 1e-6).  Layer 0 of such a stack now clears
    the slot itself."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    out, ref, inst = run_stack(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, B, T, H, Lyr))
    check_against(out, ref, 'c', ident(case))
    check_family(inst, cell, impl, Lyr, H)


# ----------------------------------------------------------------------------- d. two dropout sites
DROP_CASES = [('gru', 1, 16, 2), ('gru', 1, 128, 3), ('gru', 1, 256, 3), ('lstm', 2, 128, 3), ('lstm', 1, 128, 3), ('lstm', 1, 8, 1)]


@pytest.mark.parametrize('cell,dirs,H,impl', DROP_CASES)
def test_two_dropout_sites_match_oracle_with_same_masks(cell, dirs, H, impl, gemm_mode):
    """L = 3, p = 0.5: sites DEP_SITE_RNN0 + 0 and + 1, drawn in the forward and re-drawn in the backward; the oracle is fed the masks
    dep_dropout_mask draws for those sites."""
    B, T, F, Lyr, p, seed = (37 if H == 256 else 5), 9, 10, 3, 0.5, 1234
    out, ref, inst = run_stack(cell, dirs, B, T, F, H, Lyr, impl, case_rng(dirs, H, impl, 77), p=p, seed=seed)
    rnn = out['rnn']
    assert len(out['masks']) == 2 and not np.array_equal(out['masks'][0], out['masks'][1])
    for l, mask in enumerate(out['masks']):
        assert set(np.unique(mask)).issubset({0.0, 2.0}) and 0.35 < (mask == 0).mean() < 0.65, l
        assert np.abs(host(rnn.layer_output_dropped(l)) - host(rnn.layer_output(l)) * mask).max() < 1e-6, f'dropout(y{l}) is not y{l} * mask'
    assert rnn.layer_output_dropped(2) is None
    check_against(out, ref, 'd', f'{cell}-{dirs}-H{H}-impl{impl}')
    check_family(inst, cell, impl, Lyr, H)


# ----------------------------------------------------------------------------- e. each gradient input alone, dense, two-layer GRU
# H = 256: the fused two-layer launches (f.dhn0 / f.dhn1); H = 128: the per-layer cluster sweeps; H = 16: tile-MFMA
ALONE_CASES = [('gru', 1, 33, 4, 16, 256, 2, 3), ('gru', 1, 20, 3, 8, 256, 2, 3), ('gru', 1, 20, 7, 12, 128, 2, 3), ('gru', 1, 6, 20, 24, 16, 2, 2)]


@pytest.mark.parametrize('grads', [('dhn',), ('dy',), ('dy', 'dhn', 'dpooled')], ids='+'.join)
@pytest.mark.parametrize('case', ALONE_CASES, ids=ident)
def test_each_gradient_input_alone(case, grads, gemm_mode):
    """dh_n alone (non-zero in BOTH layers) must give the oracle's gradients -- not NaN or zeros from an input treated as absent --
    and so must dy alone; all three together are the sum."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    out, ref, inst = run_stack(cell, dirs, B, T, F, H, Lyr, impl, case_rng(B, T, F, H, len(grads)), grads=grads)
    check_against(out, ref, 'e', ident(case) + ' ' + '+'.join(grads))
    check_family(inst, cell, impl, Lyr, H)


# ----------------------------------------------------------------------------- f. ragged at the new depths
RAGGED_CASES = [('gru', 1, 20, 9, 12, 128, 3, 3), ('gru', 1, 20, 9, 12, 256, 1, 3), ('lstm', 1, 19, 11, 40, 128, 2, 3), ('lstm', 1, 6, 9, 8, 16, 3, 2),
                ('lstm', 2, 19, 6, 8, 128, 3, 3)]


@pytest.mark.parametrize('case', RAGGED_CASES, ids=ident)
def test_ragged_stacks_at_the_new_depths(case, gemm_mode):
    """Lengths 0, 1, T and a mix; dh_n of every layer enters at the row's last live step in sweep order."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    rng = case_rng(dirs, B, T, F, H, Lyr)
    lengths = lengths_mix(B, T, rng)
    assert (lengths == 0).any() and (lengths == 1).any() and (lengths == T).any() and ((lengths > 1) & (lengths < T)).any()
    out, ref, inst = run_stack(cell, dirs, B, T, F, H, Lyr, impl, rng, lengths=lengths)
    check_against(out, ref, 'f', ident(case))
    check_dead_positions(out)
    check_family(inst, cell, impl, Lyr, H)
    for s in inst:                                                     # ... and every sweep is a ragged instance (RAG is the last argument)
        assert re.fullmatch(RAGGED_INSTANCE, s), inst


@pytest.mark.parametrize('case', [('gru', 1, 20, 9, 12, 128, 3, 3), ('lstm', 1, 19, 11, 40, 128, 2, 3)], ids=ident)
def test_all_lengths_T_gives_the_dense_calls_bits(case, gemm_mode):
    """Same kernel family, instances that differ by the length predicate alone: bit-identical (tests/test_varlen_gpu.py at L = 2)."""
    cell, dirs, B, T, F, H, Lyr, impl = case
    res, sweeps = [], []
    for lengths in (None, np.full(B, T, np.int32)):
        out, _, inst = run_stack(cell, dirs, B, T, F, H, Lyr, impl, case_rng(B, T, H), lengths=lengths)
        check_family(inst, cell, impl, Lyr, H)
        sweeps.append(inst)
        res.append([('y', out['y'].clone()), ('pooled', out['pooled']), ('h_n', out['h_n']), ('dx', out['dx'])] + list(zip(out['names'], out['G'])) +
                   [(f'layer {l} output', out['rnn'].layer_output(l).clone()) for l in range(Lyr)])
    assert not (sweeps[0] & sweeps[1]), sweeps                         # the ragged call launched its own instances
    for (nm, a), (_, b) in zip(*res):
        if a is None:
            continue
        assert torch.isfinite(a).all(), nm
        assert torch.equal(a, b), nm
