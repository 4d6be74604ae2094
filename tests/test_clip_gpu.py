"""Global-norm gradient clipping on the device: dep_grad_sqnorm, dep_adam_step_clipped, dep_grad_clip_scale and the optimizer /
clip_grad_norm_ surface over them, against the numpy fp64 yardstick of clip_ref.py (pinned against torch in test_clip_cpu.py).

Bounds.  The sum of squares accumulates exact fp64 products: its error is at most n * 2^-53 relative (1.8e-10 at n = 1.6 M), checked
at 1e-9; the host's own sum of the 256 partials adds 256 * 2^-53.  Determinism is checked on the BITS of the partial sums.  The
clipped update is held to tests/test_step_coverage_gpu.py's bar for the plain one (2e-7 absolute at lr <= 1e-4, parameters below 1
in magnitude: three roundings of a value whose ulp is at most 6e-8), fed the gradients the device holds.  Against torch's own fp32
update on the CPU (non-finite cases) both sides round such a value a few times: the same 2e-7.
"""
import os
import sys

import numpy as np
import pytest

from clip_ref import clip_coef, clipped_adam_step, sqnorm
from conftest import ROOT, load_golden

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L, nn
    DEV = torch.device('cuda:0')
    SLOTS = L.grad_norm_slots()
    CHUNK = int(L.load().dep_grad_norm_chunk())
else:
    SLOTS, CHUNK = 256, 1024            # only to build the parameter lists below; every test here needs the GPU

NEW_KERNELS = ('grad_sqnorm_kernel', 'adam_clipped_kernel', 'grad_clip_scale_kernel')
BUCKET = 1610242                        # the text classifier's gradient bucket


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def partials_of(ranges):
    part = torch.full((SLOTS,), -1.0, dtype=torch.float64, device=DEV)       # every slot must be overwritten
    L.grad_sqnorm(ranges, part)
    return host(part)


def _values(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(rng.uniform(-6, 2, n))).astype(np.float32)      # magnitudes over several decades


# ------------------------------------------------------------------------------------------------ sum of squares
@pytest.mark.parametrize('n', [1, 3, CHUNK - 1, CHUNK, CHUNK + 1, SLOTS * CHUNK + 1, BUCKET])
def test_sqnorm_one_range(n):
    g = _values(n, n)
    part = partials_of([dev(g)])
    ref = sqnorm([g])
    assert np.all(part >= 0.0)
    assert abs(part.sum() - ref) <= 1e-9 * ref
    nchunks = -(-n // CHUNK)
    assert np.all(part[min(nchunks, SLOTS):] == 0.0)                         # slots without a chunk hold 0
    if n == SLOTS * CHUNK + 1:                                               # slot 0 took a second chunk: the one element behind the first round
        first = sqnorm([g[:CHUNK]])
        assert abs(part[0] - (first + float(g[-1]) ** 2)) <= 1e-12 * part[0] and part[0] > first


SPLIT = [5, 1, 1023, 4096, 7, 2, 1025, 300000, 3, 64, 999, 4, 1, 2048, 77777, 13]      # 16 ranges, two of them a single element


def test_sqnorm_sixteen_ranges_equal_their_concatenation_bit_for_bit():
    assert len(SPLIT) == 16
    g = _values(sum(SPLIT), 7)
    cuts = np.cumsum([0] + SPLIT)
    pieces = [dev(g[a:b].copy()) for a, b in zip(cuts[:-1], cuts[1:])]      # each range in an allocation of its own (16-byte aligned)
    split = partials_of(pieces)
    whole = partials_of([dev(g)])
    ref = sqnorm([g])
    assert abs(split.sum() - ref) <= 1e-9 * ref
    assert split.tobytes() == whole.tobytes()
    assert partials_of(pieces).tobytes() == split.tobytes()                  # two runs: the same bits
    two = partials_of([dev(g[:12345].copy()), dev(g[12345:].copy())])        # another cut, off the 16-byte grid
    assert two.tobytes() == whole.tobytes()


def test_sqnorm_two_runs_are_bit_equal_at_the_bucket_size():
    g = dev(_values(BUCKET, 11))
    assert partials_of([g]).tobytes() == partials_of([g]).tobytes()


# ------------------------------------------------------------------------------------------------ clipped update
def _state(n, seed, fresh=False):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    g = (0.05 * rng.standard_normal(n)).astype(np.float32)
    m = np.zeros(n, np.float32) if fresh else (0.01 * rng.standard_normal(n)).astype(np.float32)
    v = np.zeros(n, np.float32) if fresh else (1e-4 * rng.random(n)).astype(np.float32)
    return p, g, m, v


def _clipped(st, part, max_norm, step, wd, decoupled, lr=1e-4, skip=False, clip_out=None, stats=None):
    p, g, m, v = (dev(a) for a in st)
    L.adam_step_clipped(p, g, m, v, lr, 0.9, 0.999, 1e-8, wd, decoupled, step, part, max_norm, skip, clip_out, stats)
    return p, g, m, v


def _plain(st, step, wd, decoupled, lr=1e-4, g=None):
    p, g0, m, v = (dev(a) for a in st)
    L.adam_step(p, g0 if g is None else g, m, v, lr, 0.9, 0.999, 1e-8, wd, decoupled, step)
    return p, m, v


SIZES = (5000, 1, 2049)                 # more than one workgroup with a ragged tail; one element; one element past a workgroup's 2048


@pytest.mark.parametrize('decoupled,wd', [(True, 1e-5), (False, 0.0), (False, 1e-3)])
@pytest.mark.parametrize('max_norm', [0.01, 0.5, 1e9])
def test_clipped_update_against_numpy(decoupled, wd, max_norm):
    sts = [_state(n, 20 + i, fresh=(i == 1)) for i, n in enumerate(SIZES)]
    step = 3
    gs = [dev(s[1]) for s in sts]
    part = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
    L.grad_sqnorm(gs, part)
    S = sqnorm([s[1] for s in sts])
    coef = clip_coef(S, max_norm)
    assert (coef < 1.0) == (max_norm < 1.0)                                  # norm ~ 4.2: the first two clip, 1e9 does not
    clip_out = torch.zeros(4, device=DEV)
    for i, st in enumerate(sts):
        p, g, m, v = _clipped(st, part, max_norm, step, wd, decoupled, clip_out=clip_out if i == 0 else None)
        assert np.array_equal(host(g), st[1])                                # g is not written back
        pn, mn, vn = clipped_adam_step(st[0], st[1], st[2].astype(np.float64), st[3].astype(np.float64), step, 1e-4, coef, wd=wd,
                                       decoupled=decoupled)
        print('n=%d max_norm=%g: |dp| %.3g |dm| %.3g |dv| %.3g' % (st[0].size, max_norm, np.abs(host(p) - pn).max(),
                                                                     np.abs(host(m) - mn).max(), np.abs(host(v) - vn).max()))
        assert np.abs(host(p) - pn).max() < 2e-7
        # the moments: the kernel forms 1 - beta in fp32, which is off by up to 2^-24 / (1 - beta) relative (6e-7 for beta1, 6e-5 for beta2)
        assert np.abs(host(m) - mn).max() <= 2e-6 * np.abs(mn).max()
        assert np.abs(host(v) - vn).max() <= 1e-4 * np.abs(vn).max()
        assert np.abs(pn - st[0]).max() > 1e-6                               # the step moved something
    co = host(clip_out).astype(np.float64)
    q = min(1.0, max_norm / (np.sqrt(S) + 1e-6))
    assert abs(co[0] - q) <= 1e-6 * q and abs(co[1] - np.sqrt(S)) <= 1e-6 * np.sqrt(S) and co[2] == 1.0 and co[3] == 0.0


# every size of SIZES (the plain kernel takes one element per thread, the clipped one eight: a ragged tail, one element, one element past a
# clipped workgroup's 2048) in each of the three forms of the expression; the cases at 5000 keep the ids they always had
@pytest.mark.parametrize('n,decoupled,wd,max_norm', [
    pytest.param(n, decoupled, wd, max_norm, id=f'{max_norm}-{decoupled}-{wd}' + ('' if n == SIZES[0] else f'-{n}'))
    for n in SIZES for max_norm in (float('inf'), 0.0, 1e9) for decoupled, wd in [(True, 1e-5), (False, 0.0), (False, 1e-3)]])
def test_coefficient_one_gives_the_plain_update_bit_for_bit(n, decoupled, wd, max_norm):
    st = _state(n, 31)
    part = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
    L.grad_sqnorm([dev(st[1])], part)
    clip_out = torch.zeros(4, device=DEV)
    p, _, m, v = _clipped(st, part, max_norm, 2, wd, decoupled, clip_out=clip_out)
    p0, m0, v0 = _plain(st, 2, wd, decoupled)
    assert host(clip_out)[0] == 1.0
    assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)


@pytest.mark.parametrize('decoupled,wd', [(True, 1e-5), (False, 1e-3)])
def test_scale_in_place_then_plain_update_equals_the_fused_update(decoupled, wd):
    sts = [_state(n, 40 + i) for i, n in enumerate(SIZES)]
    gs = [dev(s[1]) for s in sts]
    part = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
    L.grad_sqnorm(gs, part)
    max_norm = 0.3
    coef = clip_coef(sqnorm([s[1] for s in sts]), max_norm)
    assert coef < 1.0
    fused = [_clipped(st, part, max_norm, 4, wd, decoupled) for st in sts]
    clip_out = torch.zeros(4, device=DEV)
    L.grad_clip_scale(gs, part, max_norm, clip_out)
    c = host(clip_out)[0]                                                    # the device's own fp32 coefficient
    assert c.dtype == np.float32 and abs(float(c) - float(coef)) <= 1e-6 * coef
    for st, g, f in zip(sts, gs, fused):
        assert np.array_equal(host(g), st[1] * c)                            # one fp32 product per element
        p, m, v = _plain(st, 4, wd, decoupled, g=g)
        assert torch.equal(p, f[0]) and torch.equal(m, f[2]) and torch.equal(v, f[3])
    # measure only: the gradients are left as they are
    before = [host(g).copy() for g in gs]
    L.grad_sqnorm(gs, part)
    L.grad_clip_scale(gs, part, float('inf'), clip_out)
    assert all(np.array_equal(host(g), b) for g, b in zip(gs, before)) and host(clip_out)[0] == 1.0


# ------------------------------------------------------------------------------------------------ non-finite gradients
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_nonfinite_gradient_is_skipped_or_follows_torch(bad):
    sts = [_state(3000, 50), _state(700, 51)]
    sts[1][1][123] = bad
    gs = [dev(s[1]) for s in sts]
    part = torch.empty(SLOTS, dtype=torch.float64, device=DEV)
    L.grad_sqnorm(gs, part)
    # skip_nonfinite: nothing moves, the record says why
    clip_out = torch.zeros(4, device=DEV); stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    for i, st in enumerate(sts):
        p, _, m, v = _clipped(st, part, 1.0, 1, 1e-5, True, skip=True, clip_out=clip_out if i == 0 else None, stats=stats if i == 0 else None)
        assert host(p).tobytes() == st[0].tobytes() and host(m).tobytes() == st[2].tobytes() and host(v).tobytes() == st[3].tobytes()
    assert host(clip_out)[2] == 0.0
    assert host(stats).tolist() == [1.0, 0.0, 1.0, 0.0]
    # without it the arithmetic follows, as torch's does (error_if_nonfinite=False)
    ps = [torch.nn.Parameter(torch.from_numpy(s[0].copy())) for s in sts]
    opt = torch.optim.AdamW(ps, lr=1e-4, weight_decay=1e-5)
    for q, s in zip(ps, sts):
        q.grad = torch.from_numpy(s[1].copy())
        opt.state[q] = {'step': torch.tensor(4.0), 'exp_avg': torch.from_numpy(s[2].copy()), 'exp_avg_sq': torch.from_numpy(s[3].copy())}
    torch.nn.utils.clip_grad_norm_(ps, 1.0)
    opt.step()
    nans = 0
    for q, st in zip(ps, sts):
        p, _, m, v = _clipped(st, part, 1.0, 5, 1e-5, True)
        want, got = q.detach().numpy(), host(p)
        assert np.array_equal(np.isnan(want), np.isnan(got))
        ok = ~np.isnan(want)
        assert np.abs(want[ok] - got[ok]).max(initial=0.0) < 2e-7
        nans += int(np.isnan(got).sum())
    assert nans == (3700 if np.isnan(bad) else 1)                            # NaN: the coefficient is NaN; inf: coefficient 0, inf * 0 at one element


# ------------------------------------------------------------------------------------------------ models
def _pads(model):
    """Indices of _flat_grad that belong to no tensor: the alignment pads inside the live bucket."""
    used = np.zeros(model._flat_grad.numel(), bool)
    for p in model.parameters():
        if p.live:
            used[p.offset:p.offset + p.numel] = True
    return np.flatnonzero(~used)


def _model(name):
    from icassp2022_depression_amd import audio_gru_whole, text_bilstm_whole
    mod, cls, fix = {'audio': (audio_gru_whole, 'AudioBiLSTM', 'audio_clf_tiny'), 'text': (text_bilstm_whole, 'TextBiLSTM', 'text_clf_tiny')}[name]
    g = load_golden(fix)
    B, T, F, H = [int(v) for v in g['shape']]
    cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0)
    model = getattr(mod, cls)(cfg, seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()}, strict=True)
    return mod, model, g


@pytest.mark.parametrize('name', ['audio', 'text'])
def test_model_steps_with_clipping_against_numpy(name):
    mod, model, g = _model(name)
    lr, max_norm = 1e-4, 1e-3
    opt = nn.AdamW(mod.get_param_group(model), lr=lr, max_grad_norm=max_norm)
    wd = {p.name: grp['weight_decay'] for grp in opt.param_groups for p in grp['params']}
    crit = nn.CrossEntropyLoss()
    model.train()
    params = dict(model.named_parameters())
    M, V = {}, {}
    assert len(_pads(model)) > 0                                             # these shapes have pads (ln: 5 elements, the head's bias: 2)
    for step in (1, 2, 3):
        opt.zero_grad()
        loss = crit(model(g['x']), g['y'])
        loss.backward()
        live = [n for n, p in params.items() if p.grad is not None]
        assert len(live) >= 12
        P0 = {n: host(params[n].data).astype(np.float64) for n in live}
        G = {n: host(params[n].grad).copy() for n in live}
        assert not host(model._flat_grad)[_pads(model)].any()
        opt.step()
        S = sqnorm(list(G.values()))
        coef = clip_coef(S, max_norm)
        stats = opt.grad_stats()
        assert stats['steps'] == step and stats['last_finite']
        assert abs(stats['last_coef'] - coef) <= 1e-6 * coef and abs(stats['last_norm'] - np.sqrt(S)) <= 1e-6 * np.sqrt(S)
        if step == 1:
            assert coef < 1.0 and stats['last_coef'] < 1.0 and stats['clipped'] == 1       # the first step clips
        for n in live:
            if step == 1:
                M[n] = np.zeros_like(P0[n]); V[n] = np.zeros_like(P0[n])
            pn, M[n], V[n] = clipped_adam_step(P0[n], G[n], M[n], V[n], step, lr, coef, wd=wd[n], decoupled=True)
            assert np.abs(host(params[n].data) - pn).max() < 2e-7, (step, n)
            assert np.abs(pn - P0[n]).max() > 0.1 * lr, (step, n)            # the step really moved the parameter
        assert not host(model._flat_grad)[_pads(model)].any()               # the pads the norm runs over are exactly zero
    stats = opt.grad_stats()
    assert stats['steps'] == 3 and stats['clipped'] >= 1 and stats['skipped'] == 0 and stats['max_norm'] > 0.0
    model.check_health()


def test_fusion_head_step_with_clipping_keeps_its_pads_zero():
    """FusionNet trains fc_final.0.weight only.  Ht + Ha = 18 leaves a two-element pad behind it in the gradient bucket; the step runs on
    given features (the frozen encoders are not part of it)."""
    from icassp2022_depression_amd import fuse_net
    Ht, Ha, B = 8, 10, 6
    model = fuse_net.fusion_net(12, Ht, 2, 0.0, 1, Ha, 7, seed=4)
    pads = _pads(model)
    assert model._flat_grad.numel() == 20 and pads.tolist() == [18, 19]
    opt = nn.Adam(model.parameters(), lr=1e-4, max_grad_norm=1e-3)
    crit = fuse_net.MyLoss()
    rng = np.random.default_rng(8)
    tf, af = dev(rng.standard_normal((B, Ht)).astype(np.float32)), dev(rng.standard_normal((B, Ha)).astype(np.float32))
    y = rng.uniform(0, 20, (B, 1)).astype(np.float32)
    model.train()
    W = dict(model.named_parameters())['fc_final.0.weight']
    for step in (1, 2):
        opt.zero_grad()
        crit(tf, af, y, model).backward()
        P0, G = host(W.data).astype(np.float64), host(W.grad).copy()
        opt.step()
        coef = clip_coef(sqnorm([G]), 1e-3)
        assert coef < 1.0
        if step == 1:
            pn, m, v = clipped_adam_step(P0, G, np.zeros_like(P0), np.zeros_like(P0), 1, 1e-4, coef)
            assert np.abs(host(W.data) - pn).max() < 2e-7
        assert not host(model._flat_grad)[pads].any()
    assert opt.grad_stats()['steps'] == 2 and opt.grad_stats()['clipped'] == 2


def test_clip_grad_norm_function_on_a_model():
    mod, model, g = _model('audio')
    model.train()
    nn.CrossEntropyLoss()(model(g['x']), g['y']).backward()
    params = [p for p in model.parameters() if p.grad is not None]
    G = [host(p.grad).copy() for p in params]
    S = sqnorm(G)
    max_norm = 0.25 * np.sqrt(S)
    r = nn.clip_grad_norm_(model.parameters(), max_norm)
    coef = clip_coef(S, max_norm)
    c = np.float32(r.coef())                                                 # the device's own fp32 coefficient
    assert coef < 1.0 and abs(r.item() - np.sqrt(S)) <= 1e-6 * np.sqrt(S) and abs(float(c) - float(coef)) <= 1e-6 * coef
    for p, g0 in zip(params, G):
        assert np.array_equal(host(p.grad), g0 * c), p.name
    assert not host(model._flat_grad)[_pads(model)].any()
    after = sqnorm([host(p.grad) for p in params])
    assert abs(np.sqrt(after) - max_norm) <= 1e-5 * max_norm


# ------------------------------------------------------------------------------------------------ launch sequence
def _kernels_of_a_step(opt_kw):
    mod, model, g = _model('audio')
    opt = nn.AdamW(mod.get_param_group(model), lr=1e-4, **opt_kw)
    crit = nn.CrossEntropyLoss()
    model.train()

    def step():
        opt.zero_grad(); crit(model(g['x']), g['y']).backward(); opt.step()
    step(); torch.cuda.synchronize()
    L.order_log_enable(True)
    try:
        step(); torch.cuda.synchronize()
        log = L.order_log_read(reset=True)
    finally:
        L.order_log_enable(False)
    return [e[2:] for e in log if e.startswith('K ')]


def test_default_optimizer_launches_none_of_the_new_kernels_and_clipping_adds_one_launch():
    plain = _kernels_of_a_step({})
    assert not [k for k in plain if any(n in k for n in NEW_KERNELS)], plain
    n_adam = sum('adam_kernel' in k for k in plain)
    assert n_adam == 2                                                       # the two weight-decay groups
    on = _kernels_of_a_step({'max_grad_norm': 1.0})
    assert sum('grad_sqnorm_kernel' in k for k in on) == 1 and sum('adam_clipped_kernel' in k for k in on) == n_adam
    assert not any('adam_kernel' in k or 'grad_clip_scale_kernel' in k for k in on)
    assert len(on) == len(plain) + 1                                         # one extra launch per step
    i = on.index(next(k for k in on if 'grad_sqnorm_kernel' in k))
    assert all('adam_clipped_kernel' in k for k in on[i + 1:]) and len(on[i + 1:]) == n_adam    # the norm first, then the updates, last in the step
    strip = lambda ks: [k for k in ks if 'adam' not in k and 'grad_sqnorm' not in k]
    assert strip(on) == strip(plain)


# ------------------------------------------------------------------------------------------------ data parallel
def _run_rank(rank, world, port, q, backend):
    # backend 'nccl': one rank per GPU over the C-ABI's RCCL communicator; 'gloo': the ranks share cuda:0 (as tests/test_dp_gpu.py runs them)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank) if backend == 'nccl' else '0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    sys.path.insert(0, ROOT)
    import contextlib
    import io
    from icassp2022_depression_amd import audio_gru_whole as m, nn, parallel
    if backend == 'nccl':
        torch.cuda.set_device(rank)
    parallel.init_from_env(backend)
    g = load_golden('audio_clf_train_eval')
    N, T, F, H = [int(v) for v in g['shape']]
    m.config.update(embedding_size=F, hidden_dims=H, dropout=0.0, batch_size=5, learning_rate=float(g['lr']))
    m.audio_features = g['feats']; m.audio_targets = g['targs']
    m.model = m.AudioBiLSTM(m.config, seed=0)
    m.model.load_state_dict({k: torch.from_numpy(v) for k, v in g['sd'].items()})
    m.optimizer = nn.AdamW(m.get_param_group(m.model), lr=m.config['learning_rate'], max_grad_norm=1e-3)
    m.criterion = nn.CrossEntropyLoss()
    with contextlib.redirect_stdout(io.StringIO()):
        m.train(1, list(range(17)))
    q.put((rank, {k: v.cpu().numpy() for k, v in m.model.state_dict().items()}, m.optimizer.grad_stats()))
    parallel.barrier()
    parallel.destroy_native_comm()
    import torch.distributed as dist
    dist.destroy_process_group()


@pytest.mark.parametrize('backend', ['gloo', 'nccl'])
def test_two_ranks_with_clipping_end_with_bit_equal_parameters(backend):
    """Every rank holds the same reduced gradients and forms the clip coefficient from them with the same bits: no collective is added,
    and the replicas stay identical.  'nccl' is one rank per GPU; 'gloo' runs the two ranks on one GPU."""
    if backend == 'nccl' and torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs (a multi-GPU driver box)')
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 25000 + os.getpid() % 1000 + (backend == 'nccl')
    procs = [ctx.Process(target=_run_rank, args=(r, 2, port, q, backend)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r, (sd, st)) for r, sd, st in (q.get(timeout=240) for _ in range(2)))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (sd0, st0), (sd1, st1) = res[0], res[1]
    assert st0 == st1 and st0['steps'] == 4 and st0['clipped'] >= 1
    for k in sd0:
        assert sd0[k].tobytes() == sd1[k].tobytes(), k
