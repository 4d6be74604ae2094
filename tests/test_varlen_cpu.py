"""Ragged batches, the parts that need no GPU: the new C-ABI symbols, the loader helper, and the yardstick of the GPU tests
(tests/varlen_ref.py: a row loop around the unchanged oracle) against stock torch's packed nn.GRU / nn.LSTM."""
import os
import re
import subprocess

import numpy as np
import pytest

from varlen_ref import bilstm_ragged, gru_ragged, lengths_mix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARLEN = ('dep_rnn_forward_varlen', 'dep_rnn_backward_varlen', 'dep_rnn_backward_overlapped_varlen',
          'dep_attn_fwd_varlen', 'dep_attn_bwd_varlen')


def test_varlen_symbols_in_header_library_and_binding():
    from icassp2022_depression_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    for name in VARLEN:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), f'{name} is not declared in include/dep_rnn.h'
        assert name in _lib.EXPORTS, f'{name} is not in _lib.EXPORTS'
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in VARLEN:
        assert name in exported, f'{name} is not exported by {_lib.LIB_PATH}'
    _lib.load()                             # every declared symbol resolves with its signature


def test_pad_ragged_round_trip(tmp_path):
    from icassp2022_depression_amd import _common as C
    rng = np.random.default_rng(0)
    lens = [5, 1, 0, 3, 5]
    seqs = [rng.standard_normal((n, 4)) for n in lens]
    x, lengths = C.pad_ragged(seqs)
    assert x.shape == (5, 5, 4) and x.dtype == np.float32
    assert lengths.dtype == np.int32 and lengths.tolist() == lens
    for i, s in enumerate(seqs):
        assert np.array_equal(x[i, :lens[i]], s.astype(np.float32))
        assert not x[i, lens[i]:].any()                      # the padding is zeros (the ragged entry points need it finite)
    # the object array a ragged Python list becomes in np.savez: loading needs allow_pickle=True
    obj = np.empty(len(seqs), dtype=object)
    for i, s in enumerate(seqs):
        obj[i] = s
    path = tmp_path / 'ragged.npz'
    np.savez(path, feats=obj)
    with pytest.raises(ValueError):
        np.load(path)['feats']
    x2, l2 = C.pad_ragged(np.load(path, allow_pickle=True)['feats'])
    assert np.array_equal(x2, x) and np.array_equal(l2, lengths)
    with pytest.raises(ValueError):
        C.pad_ragged([np.zeros((3, 4)), np.zeros((2, 5))])
    with pytest.raises(ValueError):
        C.pad_ragged([np.zeros(4)])


def test_lengths_mix_has_the_required_rows():
    n = lengths_mix(50, 9)
    assert n[0] == 9 and n[1] == 1 and n[2] == 0                      # full, one step, empty
    assert n[15] == 9 and n[16] == 1                                  # either side of a 16-row tile boundary
    assert (n[16:32] <= 2).all()                                      # a whole tile of short rows
    assert n.dtype == np.int32 and (n >= 0).all() and (n <= 9).all()


def _params(rng, cell, F, H, L, dirs):
    G = 3 if cell == 'gru' else 4
    prefix = 'rnn'
    P = {}
    for l in range(L):
        for d in range(dirs):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else H * dirs
            for nm, shp in (('weight_ih', (G * H, inp)), ('weight_hh', (G * H, H)), ('bias_ih', (G * H,)), ('bias_hh', (G * H,))):
                P[f'{prefix}.{nm}_{sfx}'] = rng.uniform(-0.4, 0.4, shp)
    return P, prefix


@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_row_loop_oracle_equals_torch_packed_sequences(cell):
    """The yardstick itself: pack_padded_sequence(enforce_sorted=False) -> nn.GRU / bidirectional nn.LSTM ->
    pad_packed_sequence(total_length=T) in fp64, against the row loop: y, h_n, a length-masked mean pool, every weight gradient."""
    torch = pytest.importorskip('torch')
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    rng = np.random.default_rng(5)
    B, T, F, H, L = 7, 9, 5, 6, 2
    dirs = 1 if cell == 'gru' else 2
    lengths = np.array([9, 1, 4, 9, 2, 7, 3], dtype=np.int32)
    P, prefix = _params(rng, cell, F, H, L, dirs)
    x = rng.standard_normal((B, T, F))
    for b in range(B):
        x[b, lengths[b]:] = 0.0
    mod = (torch.nn.GRU if cell == 'gru' else torch.nn.LSTM)(F, H, num_layers=L, batch_first=True, bidirectional=dirs == 2).double()
    with torch.no_grad():
        for k, v in P.items():
            getattr(mod, k.split('.', 1)[1]).copy_(torch.from_numpy(v))
    xt = torch.from_numpy(x).requires_grad_(True)
    packed = pack_padded_sequence(xt, torch.from_numpy(lengths.astype(np.int64)), batch_first=True, enforce_sorted=False)
    out, hid = mod(packed)
    yt, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    h_n = hid if cell == 'gru' else hid[0]
    w = rng.standard_normal((B, H * dirs))
    pool_t = yt.sum(1) / torch.from_numpy(lengths.astype(np.float64))[:, None]         # length-masked mean (yt is 0 behind each row's end)
    (pool_t * torch.from_numpy(w)).sum().backward()
    if cell == 'gru':
        r = gru_ragged(x, lengths, P, prefix, L, pool='mean', dpooled=w)
        assert np.abs(r['pooled'] - pool_t.detach().numpy()).max() < 1e-13
    else:
        dy = np.zeros((B, T, 2 * H))
        for b in range(B):
            dy[b, :lengths[b]] = w[b] / lengths[b]
        r = bilstm_ragged(x, lengths, P, prefix, L, dy=dy, dhn=np.zeros((2 * L, B, H)))
    assert np.abs(r['y'] - yt.detach().numpy()).max() < 1e-13
    assert np.abs(r['h_n'] - h_n.detach().numpy()).max() < 1e-13
    assert np.abs(r['dx'] - xt.grad.numpy()).max() < 1e-12
    for k, g in r['G'].items():
        ref = getattr(mod, k.split('.', 1)[1]).grad.numpy()
        assert np.abs(g - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), k
