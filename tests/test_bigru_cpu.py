"""The bidirectional GRU, the parts that need no GPU: the yardstick of the GPU tests (tests/bigru_ref.py, a composition of the
unchanged oracle's unidirectional layer) against stock torch.nn.GRU(bidirectional=True), the size queries of the built library for
dep_rnn_desc{cell = DEP_CELL_GRU, dirs = 2}, and the unchanged layout of every other descriptor."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from bigru_ref import bigru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = C.c_size_t(-1).value


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib
    return _lib, _lib.load()


def _params(rng, F, H, L):
    P = {}
    for l in range(L):
        for d in range(2):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else 2 * H
            for nm, shp in (('weight_ih', (3 * H, inp)), ('weight_hh', (3 * H, H)), ('bias_ih', (3 * H,)), ('bias_hh', (3 * H,))):
                P[f'rnn.{nm}_{sfx}'] = rng.uniform(-0.4, 0.4, shp)
    return P


@pytest.mark.parametrize('form', ['dense', 'packed'])
def test_composed_oracle_equals_torch_bidirectional_gru(form):
    """fp64: y, h_n, a (length-masked) mean pool over (B,2H), dx and all 16 weight gradients, dense and through
    pack_padded_sequence(enforce_sorted=False).  Bars of tests/test_varlen_cpu.py: 1e-13 on outputs, 1e-12 relative on gradients."""
    torch = pytest.importorskip('torch')
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    rng = np.random.default_rng(5)
    B, T, F, H, L = 7, 9, 5, 6, 2
    lengths = np.array([9, 1, 4, 9, 2, 7, 3], dtype=np.int32) if form == 'packed' else np.full(B, T, np.int32)
    P = _params(rng, F, H, L)
    x = rng.standard_normal((B, T, F))
    for b in range(B):
        x[b, lengths[b]:] = 0.0
    mod = torch.nn.GRU(F, H, num_layers=L, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for k, v in P.items():
            getattr(mod, k.split('.', 1)[1]).copy_(torch.from_numpy(v))
    xt = torch.from_numpy(x).requires_grad_(True)
    if form == 'packed':
        out, hid = mod(pack_padded_sequence(xt, torch.from_numpy(lengths.astype(np.int64)), batch_first=True, enforce_sorted=False))
        yt, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    else:
        yt, hid = mod(xt)
    w = rng.standard_normal((B, 2 * H)); dy = rng.standard_normal((B, T, 2 * H)); dhn = rng.standard_normal((2 * L, B, H))
    for b in range(B):
        dy[b, lengths[b]:] = 0.0
    pool_t = yt.sum(1) / torch.from_numpy(lengths.astype(np.float64))[:, None]
    ((pool_t * torch.from_numpy(w)).sum() + (yt * torch.from_numpy(dy)).sum() + (hid * torch.from_numpy(dhn)).sum()).backward()
    r = bigru(x, P, 'rnn', L, lengths=lengths if form == 'packed' else None, pool='mean', dy=dy, dpooled=w, dhn=dhn)
    assert r['pooled'].shape == (B, 2 * H)
    assert np.abs(r['pooled'] - pool_t.detach().numpy()).max() < 1e-13
    assert np.abs(r['y'] - yt.detach().numpy()).max() < 1e-13
    assert np.abs(r['h_n'] - hid.detach().numpy()).max() < 1e-13
    assert np.abs(r['dx'] - xt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(xt.grad.numpy()).max())
    assert len(r['G']) == 16
    for k, g in r['G'].items():
        ref = getattr(mod, k.split('.', 1)[1]).grad.numpy()
        assert np.abs(g - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), k


def test_ragged_builder_with_full_lengths_is_the_dense_builder():
    rng = np.random.default_rng(1)
    B, T, F, H, L = 3, 4, 5, 4, 2
    P = _params(rng, F, H, L)
    x = rng.standard_normal((B, T, F)); dy = rng.standard_normal((B, T, 2 * H))
    a = bigru(x, P, 'rnn', L, pool='sum', dy=dy)
    b = bigru(x, P, 'rnn', L, lengths=np.full(B, T), pool='sum', dy=dy)
    for k in ('y', 'pooled', 'h_n', 'dx'):
        assert np.abs(a[k] - b[k]).max() < 1e-13, k
    for k in a['G']:
        assert np.abs(a['G'][k] - b['G'][k]).max() < 1e-12, k


def test_bigru_size_queries_run_on_cpu(lib):
    """dirs = 2 is accepted exactly where the tile-MFMA sweeps run: impl 0 or 2 and an H they tile."""
    _lib, so = lib
    B, T, F, L = 19, 11, 40, 2
    for H in (16, 48, 128, 256):
        for impl in (0, 2):
            for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
                d = _lib.RnnDesc(_lib.CELL_GRU, B, T, F, H, L, 2, run, 0.5, 0, _lib.POOL_MEAN, impl)
                rb, wb = so.dep_rnn_reserve_bytes(C.byref(d)), so.dep_rnn_workspace_bytes(C.byref(d))
                assert rb > 0 and wb > 0, (H, impl, run)
                assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) == NONE, (H, impl, run)      # never the cluster kernels
                if run == _lib.RUN_TRAIN:
                    offs = [so.dep_rnn_reserve_y_offset(C.byref(d), l) for l in range(L)]
                    assert all(o != NONE and o + B * T * 2 * H * 4 <= rb for o in offs), offs
                    assert len(set(offs)) == L
                    assert rb >= L * 5 * B * T * 2 * H * 4                                    # y + four saved gates per layer, 2H wide
                    assert so.dep_rnn_reserve_ydrop_offset(C.byref(d), 0) != NONE
        for impl in (1, 3):
            d = _lib.RnnDesc(_lib.CELL_GRU, B, T, F, H, L, 2, _lib.RUN_TRAIN, 0.0, 0, _lib.POOL_MEAN, impl)
            assert so.dep_rnn_reserve_bytes(C.byref(d)) == 0 and so.dep_rnn_workspace_bytes(C.byref(d)) == 0, (H, impl)
            assert so.dep_rnn_reserve_y_offset(C.byref(d), 0) == NONE
    for H in (4, 80, 20, 512):            # no multiple of 16 / not tileable (5 tiles) / over the LDS bound
        for impl in (0, 1, 2, 3):
            d = _lib.RnnDesc(_lib.CELL_GRU, B, T, F, H, L, 2, _lib.RUN_TRAIN, 0.0, 0, _lib.POOL_MEAN, impl)
            assert so.dep_rnn_reserve_bytes(C.byref(d)) == 0 and so.dep_rnn_workspace_bytes(C.byref(d)) == 0, (H, impl)
    d = _lib.RnnDesc(_lib.CELL_GRU, B, T, F, 80, L, 2, _lib.RUN_TRAIN, 0.0, 0, _lib.POOL_MEAN, 0)
    assert so.dep_rnn_reserve_bytes(C.byref(d)) == 0
    assert b'multiple of 16' in so.dep_last_error()
    with pytest.raises(_lib.DepError, match='multiple of 16'):
        _lib.Rnn(_lib.CELL_GRU, B, T, F, 80, L, 2, True, 0.0, _lib.POOL_MEAN, 'cpu')


def test_layout_of_every_other_descriptor_is_the_parents(lib):
    """tests/golden/rnn_layout_parent.json: reserve / workspace sizes and the y / dropout(y) / exchange-buffer offsets recorded from the
    library before it accepted dirs = 2 for a GRU (cfg2, cfg3, a tile shape, generic shapes, the three run modes)."""
    _lib, so = lib
    cases = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'rnn_layout_parent.json')))['cases']
    assert len(cases) >= 12
    fix = lambda v: -1 if v == NONE else int(v)
    for c in cases:
        cell, B, T, F, H, L, dirs, run, p, pool, impl = c['desc']
        assert not (cell == _lib.CELL_GRU and dirs == 2)
        d = _lib.RnnDesc(cell, B, T, F, H, L, dirs, run, p, 0, pool, impl)
        assert so.dep_rnn_reserve_bytes(C.byref(d)) == c['reserve_bytes'], c['desc']
        assert so.dep_rnn_workspace_bytes(C.byref(d)) == c['workspace_bytes'], c['desc']
        assert [fix(so.dep_rnn_reserve_y_offset(C.byref(d), l)) for l in range(L)] == c['y_offset'], c['desc']
        assert [fix(so.dep_rnn_reserve_ydrop_offset(C.byref(d), l)) for l in range(L)] == c['ydrop_offset'], c['desc']
        assert fix(so.dep_rnn_workspace_xbuf_offset(C.byref(d))) == c['xbuf_offset'], c['desc']
