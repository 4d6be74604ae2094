"""The dropout-only run mode (DEP_RUN_DROPOUT_ONLY, include/dep_rnn.h) on the GPU: the frozen encoders of the late-fusion
scripts (fusion_net.pretrained_feature, Classification/fuse_net_whole.py:336-366) run with dropout drawn exactly as in training
but keep no backward reserve.

1. bit-identity with a DEP_RUN_TRAIN forward of the same seed (pooled, the top sequence, h_n) over the fused / cluster /
   tile-MFMA / generic forwards, depths 1-3, both cells, pool none / mean / sum, split and exact precision -- with the reserve
   and workspace poisoned (0xffffffff, a NaN in every word) before every call, so a read of an array the mode no longer writes
   shows up;
2. the cfg4 features against the oracle with the device-drawn masks;
3. dep_rnn_backward refuses a dropout-only descriptor and a reserve a dropout-only forward wrote;
4. the instances a dropout-only forward launches are a subset of the training forward's (no new template instance);
5. under the forced soft fallback of the fused GRU forward, dropout-only equals the training forward bit for bit;
6. FusionNet.pretrained_feature (clf and reg) binds the mode: same features as through DEP_RUN_TRAIN encoders, smaller reserves.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import ref_numpy as R

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L, nn
    DEV = torch.device('cuda:0')

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = np.array([0, 1, 15, 16, 17, 130, 255, 256, 257, 300, 383, 384, 495, 496, 510, 511])


def weights(cell, F, H, Ly, dirs, seed):
    G = 3 if cell == L.CELL_GRU else 4
    g = torch.Generator(device='cpu'); g.manual_seed(seed)
    k = 1.0 / np.sqrt(H)
    ws = []
    for l in range(Ly):
        inp = F if l == 0 else H * dirs
        for _ in range(dirs):
            for shape in ((G * H, inp), (G * H, H), (G * H,), (G * H,)):
                ws.append(((torch.rand(shape, generator=g) * 2 - 1) * k).to(DEV))
    return ws


def run(mode, cell, B, T, F, H, Ly, dirs, p, pool, impl, x, ws, seed, want_y=True, rnn=None):
    """One forward in `mode` on poisoned buffers -> (pooled, y, h_n, rnn)."""
    if rnn is None:
        rnn = L.Rnn(cell, B, T, F, H, Ly, dirs, mode, p, pool, DEV, impl=impl)
    rnn.reserve.view(torch.int32).fill_(-1)
    rnn.workspace.view(torch.int32).fill_(-1)
    pooled = torch.full((B, H), float('nan'), device=DEV) if (cell == L.CELL_GRU and pool != L.POOL_NONE) else None
    y = torch.full((B, T, H * dirs), float('nan'), device=DEV) if want_y else None
    h_n = torch.full((Ly * dirs, B, H), float('nan'), device=DEV)
    rnn.forward(x, ws, seed=seed, pooled=pooled, h_n=h_n, y=y)
    rnn.check()
    torch.cuda.synchronize()
    return pooled, y, h_n, rnn


def assert_same(a, b, what):
    assert a is not None and b is not None, what
    assert not torch.isnan(a).any(), what + ': NaN (an array the run mode no longer writes was read?)'
    assert torch.equal(a, b), what + ': max |diff| %g' % (a - b).abs().max().item()


def check_bit_identity(cell, B, T, F, H, Ly, dirs, p, pool, impl=0, seed=0x5eed):
    x = torch.randn(B, T, F, generator=torch.Generator(device='cpu').manual_seed(seed)).to(DEV)
    ws = weights(cell, F, H, Ly, dirs, seed + 1)
    p1, y1, h1, r1 = run(L.RUN_TRAIN, cell, B, T, F, H, Ly, dirs, p, pool, impl, x, ws, seed)
    p2, y2, h2, r2 = run(L.RUN_DROPOUT_ONLY, cell, B, T, F, H, Ly, dirs, p, pool, impl, x, ws, seed)
    assert r2.reserve.numel() < r1.reserve.numel()
    assert_same(y2, y1, 'y'); assert_same(h2, h1, 'h_n')
    if p1 is not None:
        assert_same(p2, p1, 'pooled')
        # without a caller y the pooled GRU's top sequence is written nowhere: pooled / h_n stay the same
        p3, _, h3, _ = run(L.RUN_DROPOUT_ONLY, cell, B, T, F, H, Ly, dirs, p, pool, impl, x, ws, seed, want_y=False, rnn=r2)
        assert_same(p3, p1, 'pooled (no y)'); assert_same(h3, h1, 'h_n (no y)')
    else:
        assert_same(r2.layer_output(), r1.layer_output(), 'zero-copy top sequence')
    return r1, r2


# ---- 1. bit-identity -----------------------------------------------------------------------------------------------------------
def test_cfg4_encoders_bit_identical_to_training_forward():
    check_bit_identity(L.CELL_GRU, 512, 300, 256, 256, 2, 1, 0.3, L.POOL_SUM)
    check_bit_identity(L.CELL_LSTM, 512, 300, 1024, 128, 2, 2, 0.3, L.POOL_NONE)


# pool: 0 none, 1 mean, 2 sum (DEP_POOL_*)
GRU_CASES = [(H, Ly, pool, 0) for H in (128, 256) for Ly in (1, 2, 3) for pool in (0, 1, 2)]
GRU_CASES += [(256, 2, 1, impl) for impl in (1, 2, 3)] + [(128, 3, 0, impl) for impl in (1, 2, 3)]


@pytest.mark.parametrize('H,Ly,pool,impl', GRU_CASES)
def test_gru_bit_identical_to_training_forward(H, Ly, pool, impl):
    check_bit_identity(L.CELL_GRU, 40, 12, 24, H, Ly, 1, 0.3, pool, impl)


LSTM_CASES = [(dirs, Ly, 0) for dirs in (1, 2) for Ly in (1, 2, 3)] + [(1, 2, 1), (1, 2, 2), (2, 2, 1), (2, 2, 2), (2, 2, 3)]


@pytest.mark.parametrize('dirs,Ly,impl', LSTM_CASES)
def test_lstm_bit_identical_to_training_forward(dirs, Ly, impl):
    check_bit_identity(L.CELL_LSTM, 40, 12, 24, 128, Ly, dirs, 0.3, L.POOL_NONE, impl)


def test_no_dropout_keeps_the_plain_lower_outputs_and_stays_identical():
    check_bit_identity(L.CELL_GRU, 40, 12, 24, 256, 2, 1, 0.0, L.POOL_MEAN)
    check_bit_identity(L.CELL_LSTM, 40, 12, 24, 128, 3, 2, 0.0, L.POOL_NONE)


def test_exact_mode_bit_identical_to_training_forward():
    old = L.get_gemm_mode()
    L.set_gemm_mode(0)
    try:
        check_bit_identity(L.CELL_GRU, 40, 12, 24, 256, 2, 1, 0.3, L.POOL_MEAN)
        check_bit_identity(L.CELL_GRU, 40, 12, 24, 128, 3, 1, 0.3, L.POOL_NONE)
        check_bit_identity(L.CELL_LSTM, 40, 12, 24, 128, 2, 2, 0.3, L.POOL_NONE)
    finally:
        L.set_gemm_mode(old)


# ---- 2. cfg4 against the oracle ---------------------------------------------------------------------------------------------------
def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def _mask(n, p, seed, site, shape, rows):
    m = L.dropout_mask(n, p, seed, site, DEV).view(*shape)
    out = _host(m[torch.from_numpy(rows).to(DEV)])
    del m
    return out


def test_cfg4_features_against_sampled_oracle():
    from icassp2022_depression_amd import fuse_net_whole as mod
    B, T, Ha, Ht = 512, 300, 256, 128
    cfg = dict(mod.config); cfg.update(audio_embed_size=256, audio_hidden_dims=Ha, text_embed_size=1024, text_hidden_dims=Ht)
    model = mod.fusion_net(1024, Ht, cfg['rnn_layers'], cfg['dropout'], cfg['num_classes'], Ha, 256, seed=0)
    g = torch.Generator(device='cpu'); g.manual_seed(77)
    xa = torch.randn(B, T, 256, generator=g).to(DEV); xt = torch.randn(B, T, 1024, generator=g).to(DEV)
    model.train()
    P0 = R.to_f64({k: _host(v) for k, v in model.state_dict().items() if torch.is_tensor(v) and v.is_cuda})
    seed = nn.next_dropout_seed(); nn._seed_counter[0] -= 1
    tf, af = model.pretrained_feature((xa, xt))
    assert model._rnn_t.last.desc.training == L.RUN_DROPOUT_ONLY and model._rnn_a.last.desc.training == L.RUN_DROPOUT_ONLY
    p, S = model.dropout, SAMPLE
    masks = {'rnn_text': [_mask(B * T * 2 * Ht, p, seed, 16, (B, T, 2 * Ht), S)],
             'rnn_audio': [_mask(B * T * Ha, p, seed + 1, 16, (B, T, Ha), S)],
             't0': _mask(B * Ht, p, seed, L.SITE_FC0, (B, Ht), S), 't1': _mask(B * Ht, p, seed, L.SITE_FC1, (B, Ht), S),
             'a0': _mask(B * Ha, p, seed, L.SITE_FC2, (B, Ha), S), 'a1': _mask(B * Ha, p, seed, L.SITE_FC3, (B, Ha), S)}
    Sd = torch.from_numpy(S).to(DEV)
    tfr, afr = R.fusion_features(P0, _host(xa[Sd]), _host(xt[Sd]), {'rnn_layers': 2}, 'clf', masks=masks)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)
    assert rel(_host(tf)[S], tfr) <= 1e-4
    assert rel(_host(af)[S], afr) <= 1e-4


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def test_backward_refuses_dropout_only():
    B, T, F, H = 40, 12, 24, 256
    x = torch.randn(B, T, F, device=DEV)
    ws = weights(L.CELL_GRU, F, H, 2, 1, 3)
    dws = [torch.empty_like(w) for w in ws]
    dpooled = torch.ones(B, H, device=DEV)
    _, _, _, r2 = run(L.RUN_DROPOUT_ONLY, L.CELL_GRU, B, T, F, H, 2, 1, 0.3, L.POOL_MEAN, 0, x, ws, 9)
    with pytest.raises(L.DepError) as e:
        r2.backward(x, ws, dws, dpooled=dpooled)
    assert 'DROPOUT_ONLY' in str(e.value) or 'DROPOUT_ONLY' in L.load().dep_last_error().decode()
    # a training descriptor handed a reserve whose last forward was dropout-only (buffers large enough for training)
    r1 = L.Rnn(L.CELL_GRU, B, T, F, H, 2, 1, L.RUN_TRAIN, 0.3, L.POOL_MEAN, DEV)
    r2.reserve, r2.workspace = r1.reserve, r1.workspace
    run(L.RUN_DROPOUT_ONLY, L.CELL_GRU, B, T, F, H, 2, 1, 0.3, L.POOL_MEAN, 0, x, ws, 9, rnn=r2)
    with pytest.raises(L.DepError) as e:
        r1.backward(x, ws, dws, dpooled=dpooled)
    assert 'DROPOUT_ONLY' in str(e.value) or 'DROPOUT_ONLY' in L.load().dep_last_error().decode()
    # a training forward on the same reserve makes it a backward's reserve again
    run(L.RUN_TRAIN, L.CELL_GRU, B, T, F, H, 2, 1, 0.3, L.POOL_MEAN, 0, x, ws, 9, rnn=r1)
    r1.backward(x, ws, dws, dpooled=dpooled)
    torch.cuda.synchronize()
    assert all(torch.isfinite(d).all() for d in dws)


# ---- 4. launch instances ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_dropout_only_launches_a_subset_of_the_training_instances(cell):
    args = ((L.CELL_GRU, 512, 300, 256, 256, 2, 1, 0.3, L.POOL_SUM) if cell == 'gru' else
            (L.CELL_LSTM, 512, 300, 1024, 128, 2, 2, 0.3, L.POOL_NONE))
    c, B, T, F, H, Ly, dirs, p, pool = args
    x = torch.randn(B, T, F, device=DEV)
    ws = weights(c, F, H, Ly, dirs, 5)
    r1 = L.Rnn(c, B, T, F, H, Ly, dirs, L.RUN_TRAIN, p, pool, DEV)
    r2 = L.Rnn(c, B, T, F, H, Ly, dirs, L.RUN_DROPOUT_ONLY, p, pool, DEV)
    sets = []
    for mode, rnn in ((L.RUN_TRAIN, r1), (L.RUN_DROPOUT_ONLY, r2)):
        torch.cuda.synchronize()
        L.instance_log_enable(True)
        run(mode, *args, 0, x, ws, 11, want_y=(cell == 'lstm'), rnn=rnn)
        sets.append(L.instance_log_read(reset=True))
        L.instance_log_enable(False)
    train, donly = sets
    assert donly <= train, sorted(donly - train)
    key = 'gru2_fwd_fused<true' if cell == 'gru' else 'lstm_fwd_cluster'
    assert any(key in s for s in donly), sorted(donly)


# ---- 5. soft fallback -------------------------------------------------------------------------------------------------------------
FALLBACK_CHILD = r'''
import sys, json, ctypes, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_dropout_only_gpu as t
from icassp2022_depression_amd import _lib as L
B, T, F, H = 40, 12, 24, 256
x = torch.randn(B, T, F, generator=torch.Generator(device='cpu').manual_seed(21)).to(t.DEV)
ws = t.weights(L.CELL_GRU, F, H, 2, 1, 22)
res, arrs = {}, {}
for mode in (L.RUN_TRAIN, L.RUN_DROPOUT_ONLY):
    L.load().dep_rnn_set_exclusive(1)          # (Rnn.check() switched the attempt off after the first fallback)
    pooled, y, h_n, rnn = t.run(mode, L.CELL_GRU, B, T, F, H, 2, 1, 0.3, L.POOL_MEAN, 0, x, ws, 23)
    res['status%d' % mode] = int(L.load().dep_rnn_status(ctypes.byref(rnn.desc), L._ptr(rnn.workspace), L.stream()))
    res['soft%d' % mode] = int(rnn.fallback_word().item())
    for k, v in (('pooled', pooled), ('y', y), ('h_n', h_n)):
        arrs['%s%d' % (k, mode)] = v.cpu().numpy()
np.savez(sys.argv[2], **arrs)
print(json.dumps(res))
'''


def test_forced_soft_fallback_is_bit_identical(tmp_path):
    # DEP_FORCE_SOFT_FALLBACK=1 (read once per process: a child): every fused launch gives up and the per-layer kernels redo the
    # forward.  Dropout-only must then equal the training forward's fallback bit for bit (same kernels, same masks) with a clean
    # status.  The per-layer kernels are not the fused kernel's arithmetic (layer 1's projection is a GEMM there): against the
    # fused run the fallback agrees within the path's tolerance, as in mode 1 (include/dep_rnn.h, dep_rnn_set_exclusive).
    out = str(tmp_path / 'fb.npz')
    env = dict(os.environ, DEP_FORCE_SOFT_FALLBACK='1')
    r = subprocess.run([sys.executable, '-c', FALLBACK_CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    assert res['status1'] == 0 and res['status2'] == 0 and res['soft1'] != 0 and res['soft2'] != 0, res     # both fell back, cleanly
    B, T, F, H = 40, 12, 24, 256
    x = torch.randn(B, T, F, generator=torch.Generator(device='cpu').manual_seed(21)).to(DEV)
    ws = weights(L.CELL_GRU, F, H, 2, 1, 22)
    pooled, y, h_n, rnn = run(L.RUN_DROPOUT_ONLY, L.CELL_GRU, B, T, F, H, 2, 1, 0.3, L.POOL_MEAN, 0, x, ws, 23)
    assert int(rnn.fallback_word().item()) == 0                                 # in this process the fused forward ran
    fb = np.load(out)
    for name, t in (('pooled', pooled), ('y', y), ('h_n', h_n)):
        a2, a1 = fb[name + '2'], fb[name + '1']
        assert not np.isnan(a2).any() and np.array_equal(a2.view(np.uint32), a1.view(np.uint32)), name
        fused = t.cpu().numpy()
        assert np.abs(a2 - fused).max() <= 1e-4 * max(1.0, np.abs(fused).max()), name


# ---- 6. model level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['clf', 'reg'])
def test_fusion_pretrained_feature_binds_dropout_only(variant):
    if variant == 'clf':
        from icassp2022_depression_amd import fuse_net_whole as mod
    else:
        from icassp2022_depression_amd import fuse_net as mod
    B, T = 48, 20
    model = mod.fusion_net(1024, 128, 2, 0.3, mod.config['num_classes'], 256, 256, seed=0)
    g = torch.Generator(device='cpu'); g.manual_seed(31)
    xa = torch.randn(B, T, 256, generator=g).to(DEV); xt = torch.randn(B, T, 1024, generator=g).to(DEV)
    model.train()
    s0 = nn._seed_counter[0]
    tf2, af2 = model.pretrained_feature((xa, xt))
    rt, ra = model._rnn_t.last, model._rnn_a.last
    assert rt.desc.training == L.RUN_DROPOUT_ONLY and ra.desc.training == L.RUN_DROPOUT_ONLY
    tf2, af2 = tf2.clone(), af2.clone()
    # the same call through training-mode encoders (what the library ran before the mode existed)
    for cache in (model._rnn_t, model._rnn_a):
        cache.get = (lambda g_: lambda B_, T_, m: g_(B_, T_, L.RUN_TRAIN if m == L.RUN_DROPOUT_ONLY else m))(cache.get)
    nn._seed_counter[0] = s0
    tf1, af1 = model.pretrained_feature((xa, xt))
    assert model._rnn_t.last.desc.training == L.RUN_TRAIN
    assert_same(tf2, tf1, 'text feature'); assert_same(af2, af1, 'audio feature')
    assert rt.reserve.numel() < model._rnn_t.last.reserve.numel() and ra.reserve.numel() < model._rnn_a.last.reserve.numel()
    # eval: no dropout, unchanged
    model.eval()
    tfe, afe = model.pretrained_feature((xa, xt))
    assert model._rnn_t.last.desc.training == L.RUN_EVAL and model._rnn_a.last.desc.training == L.RUN_EVAL
    tfe2, afe2 = model.pretrained_feature((xa, xt))
    assert_same(tfe, tfe2, 'eval text feature'); assert_same(afe, afe2, 'eval audio feature')
    assert not torch.equal(tfe, tf2)
