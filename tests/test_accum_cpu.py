"""Gradient accumulation over micro-batches, the parts that need no GPU.

1. dep_grad_accumulate refuses bad arguments (DEP_ERR_ARG) before any HIP call, as the clipping entry points do (tests/test_clip_cpu.py).
2. The grouping helper of the training loop: row totals, a ragged last group, K larger than the number of mini-batches.
3. The optimizer's host logic against a recording stand-in of the binding: K = 3 over 7 micro-steps plus flush() -- the `first` flags,
   which calls carry `partials`, when the step number advances, what the updates read.
4. The data-parallel deferral flag and the declared row count.
"""
import pytest

torch = pytest.importorskip('torch')

from optim_rec import ERR_ARG, _Owner, _arrs, _params, lib, name_buffers, record_binding  # noqa: E402,F401 -- lib is a fixture


# ------------------------------------------------------------------------------------------------ argument refusals
def test_grad_accumulate_refuses_bad_arguments(lib):
    ok = 0x1000                                                       # never dereferenced on the host: the checks come first
    acc, cnts = _arrs([ok], [8])
    g, _ = _arrs([0x2000], [8])
    call = lib.dep_grad_accumulate
    assert call(None, g, cnts, 1, 1.0, 0, None, None) == ERR_ARG
    assert call(acc, None, cnts, 1, 1.0, 0, None, None) == ERR_ARG
    assert call(acc, g, None, 1, 1.0, 0, None, None) == ERR_ARG
    assert b'bad argument' in lib.dep_last_error()
    assert call(acc, g, cnts, 0, 1.0, 0, None, None) == ERR_ARG
    assert call(acc, g, cnts, -1, 1.0, 0, None, None) == ERR_ARG
    a17, c17 = _arrs([ok] * 17, [4] * 17)
    g17, _ = _arrs([0x2000] * 17, [4] * 17)
    assert call(a17, g17, c17, 17, 1.0, 0, None, None) == ERR_ARG
    assert call(acc, g, cnts, 1, float('nan'), 0, None, None) == ERR_ARG
    assert call(acc, g, cnts, 1, float('nan'), 1, ok, None) == ERR_ARG
    for bad in (0, -3):
        a2, c2 = _arrs([ok, ok], [4, bad])
        g2, _ = _arrs([0x2000, 0x2000], [4, 4])
        assert call(a2, g2, c2, 2, 1.0, 0, None, None) == ERR_ARG
    _, c2 = _arrs([ok, ok], [4, 4])
    for a_ptrs, g_ptrs in (([ok, None], [0x2000, 0x2000]), ([ok, ok], [0x2000, None]),            # a NULL range on either side
                           ([ok, ok + 4], [0x2000, 0x2000]), ([ok, ok], [0x2000, 0x2008])):       # a pointer off the 16-byte grid
        a2, _ = _arrs(a_ptrs, [4, 4]); g2, _ = _arrs(g_ptrs, [4, 4])
        assert call(a2, g2, c2, 2, 1.0, 0, None, None) == ERR_ARG, (a_ptrs, g_ptrs)


# ------------------------------------------------------------------------------------------------ grouping helper
def test_accumulation_groups():
    from icassp2022_depression_amd._common import accumulation_groups
    assert accumulation_groups([4, 4, 4, 3], 2) == [(0, 2, 8), (2, 4, 7)]
    assert accumulation_groups([5, 5, 5, 5, 2], 2) == [(0, 2, 10), (2, 4, 10), (4, 5, 2)]          # a ragged last group of one
    assert accumulation_groups([5, 5, 2], 3) == [(0, 3, 12)]
    assert accumulation_groups([5, 2], 8) == [(0, 2, 7)]                                            # K larger than the batch count
    assert accumulation_groups([6, 1], 1) == [(0, 1, 6), (1, 2, 1)]
    assert accumulation_groups([], 4) == []
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            accumulation_groups([1, 2], bad)


def test_train_epoch_declares_each_group_before_its_criteria_and_flushes(monkeypatch):
    from icassp2022_depression_amd import _common, nn, parallel
    log = []
    monkeypatch.setattr(parallel, 'set_global_count', lambda n: log.append(('count', n)))
    monkeypatch.setattr(parallel, 'set_accumulated_count', lambda n: log.append(('rows', n)))

    class Model:
        device = torch.device('cpu')

    class Opt:
        accumulate_steps = 2

        def zero_grad(self):
            pass

        def step(self):
            log.append(('opt_step',))

        def flush(self):
            log.append(('flush',))

    def step(a, b, then):
        log.append(('step', a, b))
        return nn.Loss(torch.tensor([float(b - a)]), lambda: None), None

    total = _common.train_epoch(Model(), Opt(), 15, 4, step)
    assert log == [('count', 4), ('rows', 8), ('step', 0, 4), ('opt_step',), ('count', 4), ('step', 4, 8), ('opt_step',),
                   ('count', 4), ('rows', 7), ('step', 8, 12), ('opt_step',), ('count', 3), ('step', 12, 15), ('opt_step',),
                   ('flush',), ('rows', None), ('count', None)]
    assert total == 15.0


# ------------------------------------------------------------------------------------------------ host logic, recording binding
@pytest.fixture()
def rec(monkeypatch):
    return record_binding(monkeypatch, adam_logs_p=True)


def _groups(nn, names):
    a, b = _Owner(32, 20), _Owner(16, 12)
    name_buffers(names, a=a, b=b)
    pa = _params(nn, a, [5, 8, 3, 6], dead=(3,))           # offsets 0, 8, 16, 20; the last one is dead (grad None)
    pb = _params(nn, b, [10])
    return [{'params': [pa[0], pa[1]], 'weight_decay': 0.0}, {'params': [pa[2], pa[3], pb[0]], 'weight_decay': 1e-5, 'lr': 5e-4}], (a, b), pa, pb


G_SPANS = [('aG', 0, 16), ('aG', 16, 20), ('bG', 0, 12)]


def _acc_spans(opt, owners, names):
    """Names the accumulators once the optimizer has made them, and returns the spans the launches must cover."""
    a, b = owners
    names[opt._accum[id(a)].untyped_storage().data_ptr()] = 'aA'
    names[opt._accum[id(b)].untyped_storage().data_ptr()] = 'bA'
    return [('aA', 0, 16), ('aA', 16, 20), ('bA', 0, 12)]


@pytest.mark.parametrize('kw', [dict(), dict(max_grad_norm=0.5), dict(skip_nonfinite=True)])
def test_call_sequence_of_three_step_groups_over_seven_micro_steps_and_a_flush(rec, kw):
    nn, log, names = rec
    groups, owners, pa, pb = _groups(nn, names)
    opt = nn.AdamW(groups, lr=1e-3, accumulate_steps=3, **kw)
    clip = bool(kw)
    upd = 'clipped' if clip else 'adam'
    assert opt.pending == 0 and opt.accumulated_grad(pa[0]) is None
    opt.flush()
    assert log == [] and opt._step == 0                                   # nothing pending: nothing launched
    steps_seen, pend_seen = [], []
    for i in range(7):
        opt.step()
        steps_seen.append(opt._step); pend_seen.append(opt.pending)
    assert steps_seen == [0, 0, 1, 1, 1, 2, 2] and pend_seen == [1, 2, 0, 1, 2, 0, 1]
    a_spans = _acc_spans(opt, owners, names)
    accs = [e for e in log if e[0] == 'accum']
    assert len(accs) == 7
    assert [e[4] for e in accs] == [True, False, False, True, False, False, True]                  # `first` per group
    assert [e[5] is not None for e in accs] == [False, False, clip, False, False, clip, False]     # partials: boundary + clipping, one rank
    assert all(e[3] == 1.0 and e[2] == G_SPANS for e in accs)
    assert all(e[1] == a_spans for e in accs)
    # order: a a a U U U | a a a U U U | a     (one update launch per range, straight after the boundary accumulate; no sqnorm)
    assert [e[0] for e in log] == ['accum'] * 3 + [upd] * 3 + ['accum'] * 3 + [upd] * 3 + ['accum']
    ups = [e for e in log if e[0] == upd]
    for k, e in enumerate(ups):
        i = k % 3
        assert e[1] == (G_SPANS[i][0][0] + 'P',) + G_SPANS[i][1:] and e[2] == a_spans[i]             # the update reads the ACCUMULATOR
        lr, b1, b2, eps, wd, dec, st = e[3:10]
        assert (lr, wd) == ((1e-3, 0.0) if i == 0 else (5e-4, 1e-5)) and dec is True and st == k // 3 + 1    # bias correction counts updates
        if clip:
            part, mx, skip, clip_out, stats = e[10:]
            assert part is accs[2][5] and mx == kw.get('max_grad_norm', 0.0) and skip == kw.get('skip_nonfinite', False)
            assert (clip_out is not None) == (i == 0) and (stats is not None) == (i == 0)
    # flush: the partial group of one micro-step updates; no accumulate launch carried its norm, so dep_grad_sqnorm runs on the accumulator
    del log[:]
    opt.flush()
    assert opt._step == 3 and opt.pending == 0
    assert [e[0] for e in log] == (['sqnorm'] if clip else []) + [upd] * 3
    if clip:
        assert log[0][1] == a_spans
    assert [e[2] for e in log if e[0] == upd] == a_spans and all(e[9] == 3 for e in log if e[0] == upd)
    del log[:]
    opt.flush()
    assert log == [] and opt._step == 3                                   # a second flush launches nothing
    # introspection: views into the accumulator, none for the dead parameter
    v = opt.accumulated_grad(pa[1])
    assert v.shape == (8,) and v.untyped_storage().data_ptr() == opt._accum[id(owners[0])].untyped_storage().data_ptr() and v.storage_offset() == 8
    assert opt.accumulated_grad(pa[3]) is None
    # the accumulators are laid out like _flat_grad
    assert opt._accum[id(owners[0])].shape == owners[0]._flat_grad.shape


def test_accumulate_steps_one_is_the_plain_optimizer(rec):
    nn, log, names = rec
    groups, owners, pa, pb = _groups(nn, names)
    opt = nn.AdamW(groups, lr=1e-3, accumulate_steps=1)
    opt.step(); opt.step()
    assert [e[0] for e in log] == ['adam'] * 6 and [e[2] for e in log[:3]] == G_SPANS and opt._step == 2
    assert opt.pending == 0 and not hasattr(owners[0], '_defer_grad_sync')
    del log[:]
    opt = nn.AdamW(groups, lr=1e-3, accumulate_steps=1, max_grad_norm=1.0)
    opt.step()
    assert [e[0] for e in log] == ['sqnorm', 'clipped', 'clipped', 'clipped'] and log[0][1] == G_SPANS


@pytest.mark.parametrize('bad', [0, -2, 1.5, 2.0, '2', None, True])
def test_bad_accumulate_steps_is_a_value_error(rec, bad):
    nn, log, names = rec
    groups, *_ = _groups(nn, names)
    with pytest.raises(ValueError):
        nn.Adam(groups, accumulate_steps=bad)


def test_more_ranges_than_one_launch_takes_is_an_error(rec):
    nn, log, names = rec
    o = _Owner(17 * 8, 17 * 8)
    ps = _params(nn, o, [4] * 34, dead=tuple(range(1, 34, 2)))          # 17 live tensors, none adjacent to another
    with pytest.raises(nn.L.DepError):
        nn.Adam(ps, accumulate_steps=2).step()


# ------------------------------------------------------------------------------------------------ data parallel, row count
def test_an_accumulating_optimizer_defers_the_gradient_exchange(rec, monkeypatch):
    nn, log, names = rec
    from icassp2022_depression_amd import parallel

    class Stream:
        cuda_stream = 0x77

    groups, owners, pa, pb = _groups(nn, names)
    calls = []
    monkeypatch.setattr(parallel, 'all_reduce_grads', lambda model: calls.append(model))
    monkeypatch.setitem(parallel._native, 'comm', 0x55)
    monkeypatch.setitem(parallel._native, 'stream', Stream())
    a = owners[0]
    in_call = {1: (0, 16)}
    assert not parallel.defers_grad_sync(a)
    assert parallel.make_grad_sync(a, in_call) is not None                # a native communicator and in-call ranges: overlapped
    nn.AdamW(groups, accumulate_steps=2)
    assert parallel.defers_grad_sync(a) and parallel.defers_grad_sync(owners[1])
    assert parallel.make_grad_sync(a, in_call) is None
    parallel.finish_grad_sync(a, in_call, [(16, 4)])                      # both return at once: no stream, no event, no collective
    parallel.reduce_zero_contribution(a, in_call, [(16, 4)])
    monkeypatch.setitem(parallel._native, 'comm', None)
    parallel.finish_grad_sync(a, in_call, [(16, 4)])
    parallel.reduce_zero_contribution(a, in_call, [(16, 4)])
    assert calls == []
    plain = _Owner(8, 8)
    parallel.finish_grad_sync(plain, {}, [(0, 8)])                        # a model without the flag still takes the torch path
    assert calls == [plain]


def test_declared_row_count_overrides_and_clears():
    from icassp2022_depression_amd import parallel
    try:
        assert parallel.loss_count(5) == 5 and parallel.loss_count(5, 3) == 15        # unset: the local number of terms
        parallel.set_global_count(64)
        assert parallel.global_count(5) == 5 and parallel.loss_count(5) == 5          # one rank: set_global_count is ignored, as before
        parallel.set_accumulated_count(12)
        assert parallel.loss_count(5) == 12 and parallel.loss_count(5, 3) == 36       # the regression losses keep their factor C
        assert parallel.global_count(5) == 5                                          # global_count itself does not change
        parallel.set_accumulated_count(None)
        assert parallel.loss_count(5) == 5 and parallel.loss_count(2, 4) == 8
    finally:
        parallel.set_accumulated_count(None); parallel.set_global_count(None)
