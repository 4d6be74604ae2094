"""GPU parity of the ragged-batch entry points (dep_rnn_*_varlen, dep_attn_*_varlen, the models' `lengths=`).

Definition (include/dep_rnn.h): row b of every result equals the dense path on that utterance alone at T' = lengths[b]; positions
t >= lengths[b] of every output sequence, and of dx, are exactly 0.0; weight gradients are the sum over rows.  The expectation is
tests/varlen_ref.py, a row loop around the unchanged oracle (pinned against torch's packed sequences in tests/test_varlen_cpu.py).
Tolerances are those of tests/test_kernels_gpu.py: 1e-4 absolute on outputs, 1e-4 relerr on gradients and dx.
Run on the MI355X box:  python -m pytest tests/test_varlen_gpu.py -m gpu -q"""
import re

import numpy as np
import pytest

from oracle import ref_numpy as R
from varlen_ref import attention_ragged, audio_ragged_step, bilstm_ragged, gru_ragged, lengths_mix, text_ragged_step

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    from icassp2022_depression_amd import audio_bilstm_perm, audio_gru_whole, nn, text_bilstm_whole
    DEV = torch.device('cuda:0')

ATOL = 1e-4
RTOL = 1e-4


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
    """(B, T) bool: True at padded positions."""
    return np.arange(T)[None, :] >= np.asarray(lengths)[:, None]


def make_rnn_params(rng, cell, F, H, Lyr, dirs):
    G = 3 if cell == 'gru' else 4
    P = {}; names = []
    prefix = 'lstm_net_audio' if cell == 'gru' else 'lstm_net'
    k = 1.0 / np.sqrt(H)
    for l in range(Lyr):
        for d in range(dirs):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else H * dirs
            for nm, shp in (('weight_ih', (G * H, inp)), ('weight_hh', (G * H, H)), ('bias_ih', (G * H,)), ('bias_hh', (G * H,))):
                key = f'{prefix}.{nm}_{sfx}'
                P[key] = f32(rng.uniform(-k, k, shp))
                names.append(key)
    return P, names, prefix


def ragged_input(rng, B, T, F, lengths):
    x = f32(rng.standard_normal((B, T, F)))
    x[pad_mask(lengths, T)] = 0.0                      # the padding is finite (zeros), as pad_ragged makes it
    return x


@pytest.fixture(params=['f32', 'bf16x3'])
def gemm_mode(request):
    """Both precision modes a ragged call supports (forced on every contraction size)."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


# Shapes drawn from tests/test_kernels_gpu.py RNN_CASES, so that every required kernel family runs: the generic (impl 1) and
# one-workgroup MFMA (impl 2) sweeps of both cells; gru_*_cluster_r1 at H = 64 / 128 / 256 / 512 (burst, all-gather, PK and fp32-row
# forms: even and odd T at H = 256), lstm_*_cluster; a ragged last tile, more than one batch chunk (B > 512), T = 1, T = 2, the
# benchmark's T = 300 at B = 16, and the cfg2 (GRU 256) / cfg3 (BiLSTM 128) hidden sizes.
STACK_CASES = [
    ('gru', 4, 6, 5, 8, 1), ('gru', 6, 20, 24, 16, 2), ('gru', 37, 9, 64, 256, 2), ('gru', 5, 7, 12, 48, 2), ('gru', 2, 1, 5, 16, 2),
    ('lstm', 6, 20, 24, 16, 1), ('lstm', 19, 11, 40, 128, 2), ('lstm', 3, 5, 16, 32, 2), ('lstm', 1, 1, 3, 8, 1),
    ('gru', 8, 50, 39, 128, 3), ('gru', 37, 9, 64, 256, 3), ('gru', 130, 12, 32, 256, 3), ('gru', 16, 300, 256, 256, 3),
    ('gru', 530, 4, 16, 256, 3), ('gru', 1, 1, 8, 256, 3), ('gru', 3, 2, 8, 128, 3), ('gru', 300, 13, 8, 128, 3),
    ('gru', 20, 9, 24, 64, 3), ('gru', 40, 6, 32, 512, 3),
    ('lstm', 19, 11, 40, 128, 3), ('lstm', 530, 3, 8, 128, 3), ('lstm', 2, 1, 8, 128, 3), ('lstm', 40, 5, 8, 128, 3),
    ('lstm', 400, 7, 16, 128, 3),
]
STACK_FORM_CASES = [c + ('full',) for c in STACK_CASES] + [c + ('model',) for c in STACK_CASES if c[5] == 3]


def check_stack(cell, B, T, F, H, impl, form, lengths, rng):
    """One ragged forward + backward of a 2-layer stack against the row-loop oracle.  'full': every gradient input (NaN at the padded
    positions of dy: they are ignored) and dx; 'model': what the training step passes (GRU: dpooled; BiLSTM: dy + dh_n; no dx)."""
    Lyr = 2
    dirs = 1 if cell == 'gru' else 2
    P, names, prefix = make_rnn_params(rng, cell, F, H, Lyr, dirs)
    x = ragged_input(rng, B, T, F, lengths)
    pad = pad_mask(lengths, T)
    Wd = [dev(P[n]) for n in names]
    Gd = [torch.full_like(w, float('nan')) for w in Wd]
    xd, ld = dev(x), idev(lengths)
    mean = form == 'full' or H != 128                  # the model form at H = 128 takes the sum pool (the regression model's)
    pool = (L.POOL_MEAN if mean else L.POOL_SUM) if cell == 'gru' else L.POOL_NONE
    rnn = L.Rnn(L.CELL_GRU if cell == 'gru' else L.CELL_LSTM, B, T, F, H, Lyr, dirs, True, 0.0, pool, DEV, impl=impl)
    rnn.reserve.fill_(float('nan'))
    pooled = torch.full((B, H), float('nan'), device=DEV) if cell == 'gru' else None
    h_n = torch.full((Lyr * dirs, B, H), float('nan'), device=DEV)
    rnn.forward(xd, Wd, pooled=pooled, h_n=h_n, lengths=ld)
    y = rnn.layer_output()
    dxd = torch.full((B, T, F), float('nan'), device=DEV) if form == 'full' else None
    if cell == 'gru':
        dpool = f32(rng.standard_normal((B, H)))
        if form == 'full':
            dyv = f32(rng.standard_normal((B, T, H)) * 0.3)
            dhn = np.zeros((Lyr, B, H)); dhn[-1] = f32(rng.standard_normal((B, H)) * 0.3)
            dy_in = dyv.copy(); dy_in[pad] = np.nan
            rnn.backward(xd, Wd, Gd, dy=dev(dy_in), dpooled=dev(dpool), dh_n=dev(dhn), dx=dxd, lengths=ld)
            ref = gru_ragged(x, lengths, P, prefix, Lyr, 'mean' if mean else 'sum', dy=dyv, dpooled=dpool, dhn_top=dhn[-1])
        else:
            rnn.backward(xd, Wd, Gd, dpooled=dev(dpool), dx=None, lengths=ld)
            ref = gru_ragged(x, lengths, P, prefix, Lyr, 'mean' if mean else 'sum', dpooled=dpool)
        assert np.abs(host(pooled) - ref['pooled']).max() < ATOL, 'pooled'
    else:
        dyv = f32(rng.standard_normal((B, T, 2 * H)) * 0.3)
        dhn = f32(rng.standard_normal((Lyr * 2, B, H)) * 0.3)
        dy_in = dyv.copy()
        if form == 'full':
            dy_in[pad] = np.nan
        rnn.backward(xd, Wd, Gd, dy=dev(dy_in), dh_n=dev(dhn), dx=dxd, lengths=ld)
        ref = bilstm_ragged(x, lengths, P, prefix, Lyr, dy=dyv, dhn=dhn)
    rnn.check()                                        # dep_rnn_status is DEP_OK after a ragged step
    assert np.abs(host(y) - ref['y']).max() < ATOL, 'y'
    assert not bits(y)[pad].any(), 'y is not exactly 0.0 at padded positions'
    assert not bits(rnn.layer_output(0))[pad].any(), 'layer 0 output is not exactly 0.0 at padded positions'
    assert np.abs(host(h_n) - ref['h_n']).max() < ATOL, 'h_n'
    if dxd is not None:
        assert relerr(host(dxd), ref['dx']) < RTOL, 'dx'
        assert not bits(dxd)[pad].any(), 'dx is not exactly 0.0 at padded positions'
    for n, g in zip(names, Gd):
        assert relerr(host(g), ref['G'][n]) < RTOL, n


@pytest.mark.parametrize('cell,B,T,F,H,impl,form', STACK_FORM_CASES)
def test_ragged_stack_fwd_bwd(cell, B, T, F, H, impl, form, gemm_mode):
    rng = np.random.default_rng(B * 1000 + T * 100 + F + H + impl)
    check_stack(cell, B, T, F, H, impl, form, lengths_mix(B, T, rng), rng)


def test_the_required_length_mix_runs_in_one_batch():
    """One batch with a full row, 1, 0, a length on either side of a tile boundary and a whole tile of short rows, through each
    cluster family (the vectors of the parametrised cases above with B >= 48 have the same rows)."""
    for cell, B, T, F, H in (('gru', 50, 8, 16, 256), ('gru', 50, 7, 16, 128), ('lstm', 50, 8, 16, 128)):
        rng = np.random.default_rng(B + T + H)
        n = lengths_mix(B, T, rng)
        assert n[0] == T and n[1] == 1 and n[2] == 0 and n[15] == T and n[16] == 1 and (n[16:32] <= 2).all()
        check_stack(cell, B, T, F, H, 3, 'full', n, rng)


def test_lengths_outside_0_T_are_clamped_on_the_device():
    rng = np.random.default_rng(11)
    cell, B, T, F, H = 'gru', 6, 5, 8, 16
    P, names, prefix = make_rnn_params(rng, cell, F, H, 2, 1)
    n_in = np.array([-3, 0, 5, 9, 2, 100], dtype=np.int32); n = np.clip(n_in, 0, T)
    x = ragged_input(rng, B, T, F, n)
    for impl in (1, 2):
        rnn = L.Rnn(L.CELL_GRU, B, T, F, H, 2, 1, False, 0.0, L.POOL_MEAN, DEV, impl=impl)
        pooled = torch.full((B, H), float('nan'), device=DEV)
        rnn.forward(dev(x), [dev(P[k]) for k in names], pooled=pooled, lengths=idev(n_in))
        ref = gru_ragged(x, n, P, prefix, 2, 'mean')
        assert np.abs(host(pooled) - ref['pooled']).max() < ATOL
        assert np.isfinite(host(pooled)).all()


# ----------------------------------------------------------------------------- inter-layer dropout
@pytest.mark.parametrize('mode', ['train', 'dropout_only'])
@pytest.mark.parametrize('cell,impl,H,T', [('gru', 2, 16, 9), ('gru', 1, 16, 9), ('lstm', 2, 16, 9), ('lstm', 1, 8, 9), ('gru', 3, 128, 9),
                                           ('lstm', 3, 128, 9), ('lstm', 3, 128, 8), ('gru', 3, 256, 9), ('gru', 3, 256, 8), ('gru', 3, 64, 6)])
def test_ragged_interlayer_dropout_matches_oracle_with_same_masks(cell, impl, H, T, mode, gemm_mode):
    """The Philox element index of (b, t, col) is the dense call's: the oracle is fed the masks dep_dropout_mask draws for the dense
    layout.  DEP_RUN_DROPOUT_ONLY draws the same masks and keeps no backward reserve (forward only)."""
    rng = np.random.default_rng(77 + impl + H + T)
    B, F, Lyr, p, seed = (37 if H >= 128 else 21), 10, 2, 0.5, 1234
    dirs = 1 if cell == 'gru' else 2
    lengths = lengths_mix(B, T, rng)
    pad = pad_mask(lengths, T)
    P, names, prefix = make_rnn_params(rng, cell, F, H, Lyr, dirs)
    x = ragged_input(rng, B, T, F, lengths)
    Wd = [dev(P[n]) for n in names]; Gd = [torch.full_like(w, float('nan')) for w in Wd]
    xd, ld = dev(x), idev(lengths)
    pool = L.POOL_MEAN if cell == 'gru' else L.POOL_NONE
    run = L.RUN_TRAIN if mode == 'train' else L.RUN_DROPOUT_ONLY
    rnn = L.Rnn(L.CELL_GRU if cell == 'gru' else L.CELL_LSTM, B, T, F, H, Lyr, dirs, run, p, pool, DEV, impl=impl)
    rnn.reserve.fill_(float('nan'))
    pooled = torch.full((B, H), float('nan'), device=DEV) if cell == 'gru' else None
    h_n = torch.full((Lyr * dirs, B, H), float('nan'), device=DEV)
    yout = torch.full((B, T, H * dirs), float('nan'), device=DEV)
    rnn.forward(xd, Wd, seed=seed, pooled=pooled, h_n=h_n, y=yout, lengths=ld)
    mask = host(L.dropout_mask(B * T * H * dirs, p, seed, 16, DEV)).reshape(B, T, H * dirs)      # site = DEP_SITE_RNN0 + 0
    y0d = rnn.layer_output_dropped(0)
    assert not bits(y0d)[pad].any(), 'dropout(y0) is not exactly 0.0 at padded positions'
    if mode == 'train':
        y0 = host(rnn.layer_output(0))
        assert np.abs(host(y0d) - y0 * mask).max() < 1e-6
    dyv = f32(rng.standard_normal((B, T, H * dirs)))
    if cell == 'gru':
        dpool = f32(rng.standard_normal((B, H)))
        ref = gru_ragged(x, lengths, P, prefix, Lyr, 'mean', dy=dyv, dpooled=dpool, masks=[mask])
        assert np.abs(host(pooled) - ref['pooled']).max() < ATOL
        if mode == 'train':
            rnn.backward(xd, Wd, Gd, dy=dev(dyv), dpooled=dev(dpool), lengths=ld)
    else:
        dhn = f32(rng.standard_normal((Lyr * 2, B, H)) * 0.3)
        ref = bilstm_ragged(x, lengths, P, prefix, Lyr, dy=dyv, dhn=dhn, masks=[mask])
        if mode == 'train':
            rnn.backward(xd, Wd, Gd, dy=dev(dyv), dh_n=dev(dhn), lengths=ld)
    rnn.check()
    assert np.abs(host(yout) - ref['y']).max() < ATOL
    assert not bits(yout)[pad].any()
    assert np.abs(host(h_n) - ref['h_n']).max() < ATOL
    if mode == 'train':
        for n, g in zip(names, Gd):
            assert relerr(host(g), ref['G'][n]) < RTOL, n


# ----------------------------------------------------------------------------- every length equal to T
def run_stack(cell, B, T, F, H, impl, p, lengths, P, names, x, dyv, dpool, dhn):
    dirs = 1 if cell == 'gru' else 2
    Wd = [dev(P[n]) for n in names]; Gd = [torch.full_like(w, float('nan')) for w in Wd]
    pool = L.POOL_MEAN if cell == 'gru' else L.POOL_NONE
    rnn = L.Rnn(L.CELL_GRU if cell == 'gru' else L.CELL_LSTM, B, T, F, H, 2, dirs, True, p, pool, DEV, impl=impl)
    pooled = torch.full((B, H), float('nan'), device=DEV) if cell == 'gru' else None
    h_n = torch.full((2 * dirs, B, H), float('nan'), device=DEV)
    dxd = torch.full((B, T, F), float('nan'), device=DEV)
    ld = None if lengths is None else idev(lengths)
    xd = dev(x)
    before = L.instance_log_read()
    rnn.forward(xd, Wd, seed=99, pooled=pooled, h_n=h_n, lengths=ld)
    if cell == 'gru':
        rnn.backward(xd, Wd, Gd, dy=dev(dyv), dpooled=dev(dpool), dx=dxd, lengths=ld)
    else:
        rnn.backward(xd, Wd, Gd, dy=dev(dyv), dh_n=dev(dhn), dx=dxd, lengths=ld)
    rnn.check()
    sweeps = {s for s in L.instance_log_read() - before if re.search(r'(gru|lstm)2?_(fwd|bwd)_', s)}
    outs = [rnn.layer_output().clone(), h_n, dxd] + Gd + ([pooled] if pooled is not None else [])
    return outs, sweeps


@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('cell,B,T,F,H,impl', [('gru', 6, 20, 24, 16, 1), ('gru', 37, 9, 64, 256, 2), ('lstm', 6, 20, 24, 16, 1), ('lstm', 19, 11, 40, 128, 2),
                                               ('lstm', 19, 11, 40, 128, 3), ('lstm', 40, 8, 16, 128, 3), ('gru', 8, 50, 39, 128, 3),
                                               ('gru', 37, 9, 64, 256, 3), ('gru', 33, 4, 16, 256, 3), ('gru', 20, 9, 24, 64, 3), ('gru', 40, 6, 32, 512, 3)])
def test_all_lengths_T_equals_the_dense_call(cell, B, T, F, H, impl, p, gemm_mode):
    """Within 1e-4 everywhere; bit-identical where the dense and the ragged call ran the same kernel family (the BiLSTM cluster sweeps,
    impl 1 / 2): the ragged instances differ from the dense ones by the predicate alone, and the dropout masks are the dense call's.

    Figures of the last device run of this test (one MI355X; it predates the last change to where the backward kernels select, which
    has NOT run on a device yet): every case within 1e-4; bit-identical in all tensors for impl 2 (both cells), for every cluster
    family in exact-fp32 mode, and y / h_n / pooled everywhere but the generic LSTM.  NOT bit-identical then: the generic GRU's four
    bias gradients; every tensor of the generic LSTM; in bf16x3 mode dx and the weight gradients of gru_bwd_cluster_r1 (H = 64 / 128 /
    512) and lstm_bwd_cluster, largest difference 5.5e-6 (weight_ih_l0, H = 512; 1e-7 .. 2e-6 elsewhere).  Cause in each case: the
    backend fused a product into a later sum or into split_pair's residual in the dense instance and could not across the ragged
    instance's select.  The selects now sit behind those sums (workgroup-uniform branches in the generic kernels, split words zeroed
    after rounding in the cluster kernels); whether that closes every case is what the next device run of this test shows."""
    rng = np.random.default_rng(B + T + H + impl)
    dirs = 1 if cell == 'gru' else 2
    P, names, prefix = make_rnn_params(rng, cell, F, H, 2, dirs)
    x = f32(rng.standard_normal((B, T, F)))
    dyv = f32(rng.standard_normal((B, T, H * dirs)) * 0.3); dpool = f32(rng.standard_normal((B, H))); dhn = f32(rng.standard_normal((2 * dirs, B, H)) * 0.3)
    dense, sw_d = run_stack(cell, B, T, F, H, impl, p, None, P, names, x, dyv, dpool, dhn)
    ragged, sw_r = run_stack(cell, B, T, F, H, impl, p, np.full(B, T, np.int32), P, names, x, dyv, dpool, dhn)
    assert sw_r and not (sw_r & sw_d), (sw_r, sw_d)                    # the ragged call launched its own instances ...
    family = lambda names_: {re.sub(r'<.*', '', re.sub(r'^\(', '', s)) for s in names_}
    same_family = family(sw_r) == family(sw_d)
    assert same_family or (impl == 3 and cell == 'gru'), (sw_r, sw_d)      # impl 1 / 2 and the BiLSTM cluster sweeps: one family each
    what = ['y', 'h_n', 'dx'] + names + ['pooled']
    differ = []
    for nm, a, b in zip(what, dense, ragged):
        ha, hb = host(a), host(b)
        if nm in ('y', 'h_n', 'pooled'):
            assert np.abs(ha - hb).max() < ATOL, nm                  # outputs: 1e-4 absolute
        else:
            assert relerr(hb, ha) < RTOL, nm                         # dx and the weight gradients: 1e-4 relerr, as in check_stack
        if not torch.equal(a, b):
            differ.append((nm, float(np.abs(ha - hb).max())))
    print(f'all lengths T vs dense, {cell} impl {impl} H {H} p {p}: same family {same_family}, not bit-identical: {differ}')
    if same_family:
        assert not differ, 'same kernel family: the results must be bit-identical'


# ----------------------------------------------------------------------------- which kernels a ragged call launches
def test_ragged_cfg2_and_cfg3_shaped_calls_launch_the_ragged_cluster_instances(gemm_mode):
    rng = np.random.default_rng(4)
    for cell, B, T, F, H in (('gru', 48, 8, 256, 256), ('lstm', 48, 8, 1024, 128)):       # cfg2 / cfg3 widths, auto plan (impl 0)
        dirs = 1 if cell == 'gru' else 2
        P, names, prefix = make_rnn_params(rng, cell, F, H, 2, dirs)
        lengths = lengths_mix(B, T, rng)
        x = ragged_input(rng, B, T, F, lengths)
        Wd = [dev(P[n]) for n in names]; Gd = [torch.empty_like(w) for w in Wd]
        pool = L.POOL_MEAN if cell == 'gru' else L.POOL_NONE
        rnn = L.Rnn(L.CELL_GRU if cell == 'gru' else L.CELL_LSTM, B, T, F, H, 2, dirs, True, 0.5, pool, DEV, impl=0)
        before = L.instance_log_read()
        pooled = torch.empty(B, H, device=DEV) if cell == 'gru' else None
        rnn.forward(dev(x), Wd, seed=3, pooled=pooled, lengths=idev(lengths))
        if cell == 'gru':
            rnn.backward(dev(x), Wd, Gd, dpooled=dev(rng.standard_normal((B, H))), lengths=idev(lengths))
        else:
            rnn.backward(dev(x), Wd, Gd, dy=dev(rng.standard_normal((B, T, 2 * H))), dh_n=dev(rng.standard_normal((4, B, H))), lengths=idev(lengths))
        rnn.check()
        log = L.instance_log_read() - before
        text = '\n'.join(sorted(log))
        for banned in ('gru2_fwd_fused', 'gru2_bwd_fused', 'gru_fwd_cluster16', 'gru2_fwd_df'):
            assert banned not in text, text
        if cell == 'gru':
            assert re.search(r'gru_fwd_cluster_r1<8, (true|false), true>', text), text
            assert re.search(r'gru_bwd_cluster_r1<4, (\w+, ){5}true>', text), text
            assert not re.search(r'gru_fwd_cluster_r1<8, (true|false)>', text), text          # ... and no dense instance
            assert not re.search(r'gru_bwd_cluster_r1<4, (\w+, ){1,4}\w+>', text), text
        else:
            assert re.search(r'lstm_fwd_cluster<(\w+, ){2}true>', text), text                # <SPLIT, SV16, RAG>: the dense instances are written
            assert re.search(r'lstm_bwd_cluster<(\w+, ){2}true>', text), text                # with one or two arguments, RAG defaulted
            assert not re.search(r'lstm_(fwd|bwd)_cluster<(\w+, ){0,1}\w+>', text), text
            assert not re.search(r'lstm_(fwd|bwd)_cluster<(\w+, ){2}false>', text), text


# ----------------------------------------------------------------------------- attention
@pytest.mark.parametrize('B,T,H', [(3, 6, 8), (7, 50, 128), (2, 300, 16), (5, 300, 128), (3, 330, 128), (4, 33, 64), (5, 60, 256), (6, 90, 256),
                                   (2, 170, 256), (2, 1, 128), (3, 17, 128)])
def test_ragged_attention(B, T, H):
    rng = np.random.default_rng(B + T + H)
    lengths = lengths_mix(B, T, rng)
    pad = pad_mask(lengths, T)
    out = f32(rng.standard_normal((B, T, 2 * H)))
    out_in = out.copy(); out_in[pad] = np.nan          # never read behind an utterance's last step
    hn = f32(rng.standard_normal((4, B, H)))
    Wa = f32(rng.standard_normal((H, H)) / np.sqrt(H)); ba = f32(rng.standard_normal(H))
    dctx = f32(rng.standard_normal((B, H)))
    ld = idev(lengths)
    ctx, saved = L.attn_fwd(dev(out_in), dev(hn), dev(Wa), dev(ba), lengths=ld)
    ref = attention_ragged(out, lengths, hn, Wa, ba, dctx)
    assert np.abs(host(ctx) - ref['ctx']).max() < ATOL
    assert np.abs(host(saved[0]) - ref['alpha']).max() < 1e-5
    assert not bits(saved[0])[pad].any(), 'alpha is not exactly 0 behind the utterance'
    empty = lengths == 0
    if empty.any():
        assert not bits(ctx)[empty].any(), 'an empty row must give ctx = 0'
    dWa = torch.full((H, H), float('nan'), device=DEV); dba = torch.full((H,), float('nan'), device=DEV)
    dout, dhn = L.attn_bwd(dev(dctx), dev(out_in), dev(Wa), saved, 4, dWa, dba, lengths=ld)
    for t in (dout, dhn, dWa, dba):
        assert np.isfinite(host(t)).all()
    assert not bits(dout)[pad].any(), 'dout is not exactly 0 behind the utterance'
    assert relerr(host(dout), ref['dout']) < RTOL
    assert relerr(host(dhn), ref['dhn']) < RTOL
    assert relerr(host(dWa), ref['dWa']) < RTOL
    assert relerr(host(dba), ref['dba']) < RTOL


# ----------------------------------------------------------------------------- models
MODEL_CASES = [('audio', 'clf', 24, 16), ('audio', 'reg', 24, 16), ('text', 'clf', 24, 16),
               ('audio', 'clf', 32, 256), ('audio', 'reg', 16, 128), ('text', 'clf', 24, 128)]      # the last three: the cluster sweeps


def build_model(kind, variant, F, H):
    mod = {('audio', 'clf'): audio_gru_whole, ('audio', 'reg'): audio_bilstm_perm, ('text', 'clf'): text_bilstm_whole}[(kind, variant)]
    cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0, rnn_layers=2)
    model = (mod.AudioBiLSTM if kind == 'audio' else mod.TextBiLSTM)(cfg, seed=0)
    P = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    return mod, model, cfg, P


@pytest.mark.parametrize('kind,variant,F,H', MODEL_CASES)
def test_model_ragged_batch_equals_each_utterance_alone(kind, variant, F, H):
    """Eval mode: row b of the ragged batch == the same model on x[b:b+1, :len_b] through the DENSE path at its own length."""
    mod, model, cfg, P = build_model(kind, variant, F, H)
    rng = np.random.default_rng(F + H)
    B, T = 21, 7
    lengths = np.maximum(lengths_mix(B, T, rng), 1)                  # (a model output of an empty utterance is not defined by the dense path)
    x = ragged_input(rng, B, T, F, lengths).astype(np.float32)
    model.eval()
    out = model(x, lengths=lengths).numpy()
    assert out.shape[0] == B and np.isfinite(out).all()
    for b in range(B):
        alone = model(x[b:b + 1, :lengths[b]]).numpy()
        assert np.abs(out[b] - alone[0]).max() < ATOL, (b, int(lengths[b]))
    model.check_health()


@pytest.mark.parametrize('kind,variant,F,H', MODEL_CASES)
def test_model_ragged_train_step_matches_row_loop_oracle(kind, variant, F, H):
    """One full train step (forward, loss, backward, AdamW / Adam) on a ragged batch; every live parameter's gradient and updated
    value against the row-loop oracle."""
    mod, model, cfg, P = build_model(kind, variant, F, H)
    rng = np.random.default_rng(F + H + 1)
    B, T = 21, 7
    lengths = np.maximum(lengths_mix(B, T, rng), 1)
    x = ragged_input(rng, B, T, F, lengths)
    lr = 1e-3
    if variant == 'clf':
        y = rng.integers(0, 2, B).astype(np.int64)
        opt = nn.AdamW(mod.get_param_group(model), lr=lr); crit = nn.CrossEntropyLoss()
    else:
        y = f32(rng.uniform(0, 3, (B, 1))).astype(np.float32)
        opt = nn.Adam(model.parameters(), lr=lr); crit = nn.L1Loss()
    model.train()
    opt.zero_grad()
    out = model(x.astype(np.float32), lengths=lengths)
    loss = crit(out, y)
    loss.backward()
    step = audio_ragged_step if kind == 'audio' else text_ragged_step
    o_ref, l_ref, G = step(P, x, lengths, y if variant == 'clf' else y.astype(np.float64), {'rnn_layers': 2}, variant)
    assert np.abs(out.numpy() - o_ref).max() < ATOL
    assert abs(loss.item() - l_ref) < ATOL * max(1.0, abs(l_ref))
    live = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(live) <= set(G)
    Gdev = {k: g.cpu().numpy().astype(np.float64) for k, g in live.items()}
    for k in live:
        assert relerr(Gdev[k], G[k]) < RTOL, k
    opt.step()
    model.check_health()
    # the optimizer, as tests/test_step_coverage_gpu.py checks it: fed the DEVICE gradients (compared with the oracle's above) -- an
    # lr-sized first Adam step is sign-like, so element-wise it amplifies any gradient difference near zero
    sd = model.state_dict()
    for k in live:
        wd = 0.0 if (variant == 'reg' or 'ln' in k) else 1e-5
        want, _, _ = R.adam_step(P[k], Gdev[k], np.zeros_like(P[k]), np.zeros_like(P[k]), 1, lr, wd=wd,
                                 decoupled=variant == 'clf')
        assert np.abs(sd[k].cpu().numpy() - want).max() < 2e-7, k
        assert np.abs(want - P[k]).max() > 0.5 * lr, k             # the step really moved the parameter


@pytest.mark.parametrize('kind,variant,F,H', [('audio', 'clf', 24, 16), ('audio', 'reg', 16, 128), ('text', 'clf', 24, 128)])
def test_model_with_an_empty_utterance_stays_finite(kind, variant, F, H):
    """The dense path cannot run T = 0, so nothing defines the model output of an empty utterance beyond "pooled = 0 / ctx = 0 go into
    the head"; what is promised is that it divides by nothing: outputs and every gradient finite, the other rows unchanged."""
    mod, model, cfg, P = build_model(kind, variant, F, H)
    rng = np.random.default_rng(F + H + 2)
    B, T = 21, 7
    lengths = lengths_mix(B, T, rng)
    assert (lengths == 0).any()
    x = ragged_input(rng, B, T, F, lengths).astype(np.float32)
    model.eval()
    out = model(x, lengths=lengths).numpy()
    assert np.isfinite(out).all()
    ref = model(x, lengths=np.maximum(lengths, 1)).numpy()           # (rows with len >= 1 do not depend on their neighbours)
    assert np.abs(out - ref)[lengths > 0].max() < 1e-6
    model.train()
    y = rng.integers(0, 2, B).astype(np.int64) if variant == 'clf' else f32(rng.uniform(0, 3, (B, 1))).astype(np.float32)
    loss = (nn.CrossEntropyLoss() if variant == 'clf' else nn.L1Loss())(model(x, lengths=lengths), y)
    loss.backward()
    model.check_health()
    assert np.isfinite(loss.item())
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert np.isfinite(p.grad.cpu().numpy()).all(), k


def test_overlapped_ragged_backward_single_rank_equals_the_plain_ragged_backward():
    """dep_rnn_backward_overlapped_varlen through the models (Rnn.backward with grad_sync AND lengths), as
    tests/test_dp_gpu.py::test_native_rccl_comm_overlapped_backward_single_rank does for the dense call: with a one-rank native
    communicator (a one-rank SUM is the identity) the gradient bucket must be exactly the plain ragged backward's."""
    from icassp2022_depression_amd import parallel
    grads = {}
    try:
        for native in (False, True):
            if native:
                assert parallel.init_native_comm(force_single=True) is not None
            for name, mod, cls, F, H in (('audio', audio_gru_whole, 'AudioBiLSTM', 24, 128), ('text', text_bilstm_whole, 'TextBiLSTM', 40, 128)):
                cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0)
                model = getattr(mod, cls)(cfg, seed=3)
                rng = np.random.default_rng(5)
                lengths = np.maximum(lengths_mix(19, 11, rng), 1)
                x = ragged_input(rng, 19, 11, F, lengths).astype(np.float32)
                y = np.random.default_rng(6).integers(0, 2, 19)
                model.train()
                loss = nn.CrossEntropyLoss()(model(x, lengths=lengths), y)
                assert (parallel.make_grad_sync(model, model.sync_plan()[0]) is not None) == native      # native: backward takes the overlapped entry point
                loss.backward()
                torch.cuda.synchronize()
                model.check_health()
                grads[(name, native)] = model.live_grad_bucket().clone()
    finally:
        parallel.destroy_native_comm()
    for name in ('audio', 'text'):
        assert torch.isfinite(grads[(name, True)]).all()
        assert torch.equal(grads[(name, False)], grads[(name, True)]), name


# ----------------------------------------------------------------------------- refusals
def test_ragged_refusals():
    rng = np.random.default_rng(2)
    B, T, F, H = 5, 4, 8, 16
    P, names, prefix = make_rnn_params(rng, 'gru', F, H, 2, 1)
    Wd = [dev(P[n]) for n in names]
    x = dev(rng.standard_normal((B, T, F)))
    rnn = L.Rnn(L.CELL_GRU, B, T, F, H, 2, 1, True, 0.0, L.POOL_MEAN, DEV, impl=2)
    pooled = torch.empty(B, H, device=DEV)
    good = idev(np.full(B, T))
    for bad in (good.to(torch.int64), good.float(), good[:-1].contiguous(), torch.cat([good, good]), good.cpu(), [T] * B):
        with pytest.raises(L.DepError, match='lengths'):
            rnn.forward(x, Wd, pooled=pooled, lengths=bad)
        with pytest.raises(L.DepError, match='lengths'):
            L.attn_fwd(torch.empty(B, T, 2 * H, device=DEV), torch.empty(4, B, H, device=DEV), torch.empty(H, H, device=DEV),
                       torch.empty(H, device=DEV), lengths=bad)
    # the single-product GEMM modes have no ragged instances: DEP_ERR_ARG with a message, forward and backward
    rnn.forward(x, Wd, pooled=pooled, lengths=good)
    try:
        for mode in (2, 3):
            L.set_gemm_mode(mode)
            with pytest.raises(L.DepError, match=r'\(-1\).*ragged'):
                rnn.forward(x, Wd, pooled=pooled, lengths=good)
            with pytest.raises(L.DepError, match=r'\(-1\).*ragged'):
                rnn.backward(x, Wd, [torch.empty_like(w) for w in Wd], dpooled=pooled, lengths=good)
    finally:
        L.set_gemm_mode(1, 1 << 28)
    # the C entry points refuse a null lengths pointer (the dense call is dep_rnn_forward)
    lib = L.load()
    rc = lib.dep_rnn_forward_varlen(L.C.byref(rnn.desc), x.data_ptr(), None, rnn._warr, None, pooled.data_ptr(), None,
                                    rnn.reserve.data_ptr(), rnn.reserve.numel() * 4, rnn.workspace.data_ptr(), rnn.workspace.numel() * 4,
                                    L.stream())
    assert rc == -1 and lib.dep_last_error()
    rnn.forward(x, Wd, pooled=pooled, lengths=good)
    rnn.check()


def test_feature_feeder_keeps_lengths_on_the_device():
    from icassp2022_depression_amd import _common as C
    rng = np.random.default_rng(8)
    seqs = [rng.standard_normal((n, 6)) for n in (4, 1, 3, 4, 2, 0, 4)]
    x, lengths = C.pad_ragged(seqs)
    idxs = [5, 0, 3, 6, 1]
    feed = C.FeatureFeeder(x, idxs, DEV, role='ragged_test', lengths=lengths)
    xb, lb = feed.rows(1, 4), feed.lengths_rows(1, 4)
    assert lb.dtype == torch.int32 and lb.is_cuda and lb.cpu().tolist() == [4, 4, 4]
    assert np.array_equal(xb.cpu().numpy(), x[[0, 3, 6]])
    assert feed.lengths_rows(0, 5).cpu().tolist() == [0, 4, 4, 4, 1]
    assert C.FeatureFeeder(x, idxs, DEV, role='ragged_test').lengths_rows(0, 2) is None
