"""GPU parity of impl = 9, the exchange-free per-layer LSTM sweeps, forward and backward (csrc/rnn_local_lstm.hip): a DEP_RUN_TRAIN
forward runs lstm_fwd_save_local<SPLIT, RAG>, every backward entry point lstm_bwd_local<SPLIT, RAG>, one launch per layer each, with
the whole recurrent state going in (hx, cx), out (h_n, c_n) and back (dh_n, dc_n -> dhx, dcx).

The expectation is tests/hx_ref.py (dense) and tests/state_varlen_ref.py (lengths), both float64, on the dropout masks read back from
the device's dropout(y).  Bars are those of tests/test_state_cluster_bwd_gpu.py: 1e-4 absolute on y, h_n, c_n, dx, dhx, dcx; 1e-4 of the
reference's largest magnitude on each weight and bias gradient; both parity modes (GEMM modes 0 and 1, forced on every contraction
size).  Outputs and gradients are pre-filled with NaN; every test asserts from the enqueue-order log that the only sweeps launched were
the expected instances, one per layer and pass.  Every check prints its figures first ('local-lstm-train ...'; pytest -s shows them).

The data of a case and the guard that its state matters (on the reference alone) need no GPU: they live in
tests/local_lstm_train_cases.py, and tests/test_local_lstm_train_cpu.py runs the guard on the same cases.
Run on the MI355X box:  python -m pytest tests/test_local_lstm_train_gpu.py -m gpu -q"""
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

from local_lstm_train_cases import (ATOL, F, H, RTOL, Data, case_rng, dense_cases, dense_data, ragged_data, relerr,  # noqa: F401
                                     trap_a_data)

NAN = float('nan')


# ----------------------------------------------------------------------------- device side
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


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


@pytest.fixture(params=['f32', 'bf16x3'])
def gemm_mode(request):
    """Both precision modes of the parity path (forced on every contraction size), as in tests/test_local_lstm_gpu.py."""
    L.set_gemm_mode(0 if request.param == 'f32' else 1, 0)
    yield request.param
    L.set_gemm_mode(1, 1 << 28)


class launched:
    """The sweeps enqueued inside the block, from the enqueue-order log (the instance log keeps recording for tests/conftest.py)."""

    def __enter__(self):
        L.order_log_enable(True)
        L.order_log_read(reset=True)
        return self

    def __exit__(self, *exc):
        log = L.order_log_read(reset=True)
        L.order_log_enable(False)
        self.sweeps = [re.sub(r'^\(|\)$', '', e[2:]) for e in log if e.startswith('K ') and re.search(r'(gru|lstm)2?_(fwd|bwd)_', e)]


def inst(kernel, split, ragged):
    return '%s<%s, %s>' % (kernel, 'true' if split else 'false', 'true' if ragged else 'false')


def worst(e):
    return max(e, key=lambda v: float('inf') if v[0] != v[0] else v[0])


def compare(what, outs, grads=(), atol=ATOL, rtol=RTOL):
    """outs: (name, device value as float64, reference), absolute; grads: the same, relative to the reference's largest magnitude.
    Every figure is printed before any assertion."""
    ea = [(float(np.abs(a - b).max()) if np.isfinite(a).all() else NAN, n) for n, a, b in outs]
    er = [(float(relerr(a, b)) if np.isfinite(a).all() else NAN, n) for n, a, b in grads]
    print(f'local-lstm-train {what}: ' + ', '.join(f'{n} {e:.2e}' for e, n in ea) + ' | ' + ', '.join(f'{n} {e:.2e}' for e, n in er))
    print(f'local-lstm-train {what}:' + (f' worst abs {worst(ea)[0]:.3e} ({worst(ea)[1]})' if ea else '') +
          (f' worst rel {worst(er)[0]:.3e} ({worst(er)[1]})' if er else ''))
    for e, n in ea:
        assert e < atol, f'{what}: {n}: {e:.3e}'
    for (e, n), (_, _, b) in zip(er, grads):
        assert np.abs(b).max() > 0, f'{n}: the reference gradient is trivially zero'
        assert e < rtol, f'{what}: {n}: {e:.3e}'


class Run:
    """Device side of a case: one Rnn on impl (9 unless said), forward / backward with every output NaN-filled, and the sweeps each launched."""

    def __init__(self, data, impl=9, run=None, seed=4321):
        d = self.d = data
        self.impl, self.seed = impl, seed
        self.rnn = L.Rnn(L.CELL_LSTM, d.B, d.T, F, H, d.Lyr, d.dirs, L.RUN_TRAIN if run is None else run, d.p, L.POOL_NONE, DEV, impl=impl)
        assert (self.rnn.status_word() is None) == (impl in (8, 9))
        self.Wd = [dev(d.P[k]) for k in d.names]
        self.xd = dev(d.x)
        self.ld = None if d.n is None else idev(d.n)
        self.K = d.Lyr * d.dirs

    def forward(self, hx=True, cx=True, hxd=None, cxd=None):
        d = self.d
        self.rnn.reserve.fill_(NAN)
        self.y, self.h_n, self.c_n = nans(d.B, d.T, d.dirs * H), nans(self.K, d.B, H), nans(self.K, d.B, H)
        self.hxd = hxd if hxd is not None else (dev(d.hx) if hx else None)
        self.cxd = cxd if cxd is not None else (dev(d.cx) if cx else None)
        plain = self.impl not in (8, 9)          # (a cluster descriptor takes no state member, c_n included)
        st = {} if plain else dict(hx=self.hxd, cx=self.cxd, c_n=self.c_n)
        with launched() as k:
            if self.ld is not None and not plain:
                self.rnn.forward_state_varlen(self.xd, self.Wd, self.ld, seed=self.seed, y=self.y, h_n=self.h_n, **st)
            else:
                self.rnn.forward(self.xd, self.Wd, seed=self.seed, y=self.y, h_n=self.h_n, lengths=self.ld, **st)
        self.rnn.check()
        self.fwd_sweeps = k.sweeps
        return self

    def masks(self):
        """The inter-layer dropout masks as the device applied them, read back from dropout(y) (a dead position's y is 0: its mask is not used)."""
        d = self.d
        if d.p <= 0:
            return None
        m = [(host(self.rnn.layer_output_dropped(l)) != 0) / (1.0 - d.p) for l in range(d.Lyr - 1)]
        for l, mk in enumerate(m):
            live = host(self.rnn.layer_output(l)) != 0
            assert 0.3 < (mk[live] == 0).mean() < 0.7 or live.sum() < 64, 'the mask drops about half'
        return m

    def backward(self, dy=True, dhn=True, dcn=True, want=True, dhn_t=None, dcn_t=None, dhx_t=None, dcx_t=None):
        d = self.d
        self.Gd = [torch.full_like(w, NAN) for w in self.Wd]
        self.dx = nans(d.B, d.T, F)
        self.dhnd = dhn_t if dhn_t is not None else (dev(d.dhn) if dhn else None)
        self.dcnd = dcn_t if dcn_t is not None else (dev(d.dcn) if dcn else None)
        self.dhx = dhx_t if dhx_t is not None else (nans(self.K, d.B, H) if want else None)
        self.dcx = dcx_t if dcx_t is not None else (nans(self.K, d.B, H) if want else None)
        kw = dict(dy=dev(d.dy) if dy else None, dh_n=self.dhnd, dx=self.dx)
        st = dict(hx=self.hxd, cx=self.cxd, dc_n=self.dcnd, dhx=self.dhx, dcx=self.dcx)
        any_state = any(v is not None for v in st.values())
        with launched() as k:
            if self.ld is not None and any_state:
                self.rnn.backward_state_varlen(self.xd, self.Wd, self.Gd, self.ld, **kw, **st)
            elif any_state:
                self.rnn.backward(self.xd, self.Wd, self.Gd, **kw, **st)
            else:
                self.rnn.backward(self.xd, self.Wd, self.Gd, lengths=self.ld, **kw)
        self.rnn.check()
        self.bwd_sweeps = k.sweeps
        return self

    def check_instances(self, split, backward=True):
        d = self.d
        assert self.fwd_sweeps == [inst('lstm_fwd_save_local', split, d.n is not None)] * d.Lyr, self.fwd_sweeps
        if backward:
            assert self.bwd_sweeps == [inst('lstm_bwd_local', split, d.n is not None)] * d.Lyr, self.bwd_sweeps

    def fwd_pairs(self, ref):
        return [('y', host(self.y), ref['y']), ('h_n', host(self.h_n), ref['h_n']), ('c_n', host(self.c_n), ref['c_n'])] + \
               [(f'layer {l} output', host(self.rnn.layer_output(l)), ref['ys'][l]) for l in range(self.d.Lyr)]

    def bwd_pairs(self, ref):
        outs = [('dx', host(self.dx), ref['dx'])]
        if self.dhx is not None:
            outs += [('dhx', host(self.dhx), ref['dhx']), ('dcx', host(self.dcx), ref['dcx'])]
        return outs, [(k.split('.', 1)[1], host(g), ref['G'][k]) for k, g in zip(self.d.names, self.Gd)]

    def tensors(self):
        """Every output and gradient of the last forward + backward, by name."""
        t = dict(y=self.y, h_n=self.h_n, c_n=self.c_n, dx=self.dx)
        if self.dhx is not None:
            t.update(dhx=self.dhx, dcx=self.dcx)
        t.update({k: g for k, g in zip(self.d.names, self.Gd)})
        return t


def same_bits(what, a, b, but=()):
    """Every tensor of a finite and bit-identical to b's; `but`: names left to the caller.  All names are looked at before any assertion."""
    for n in a:
        assert torch.isfinite(a[n]).all(), (what, n)
    differ = [n for n in a if n not in but and not np.array_equal(bits(a[n]), bits(b[n]))]
    print(f'local-lstm-train {what}: {len(a) - len(but)} tensors compared bit for bit, differing: {differ}')
    assert not differ, f'{what}: {differ} differ'


# ----------------------------------------------------------------------------- dense parity, full state, all gradient sources
@pytest.mark.parametrize('case', dense_cases(), ids=lambda c: '-'.join(str(v) for v in c))
def test_dense_parity_with_the_whole_state(case, gemm_mode):
    d = dense_data(case)
    r = Run(d).forward()
    masks = r.masks()
    d.state_guard(masks=masks)
    ref = d.ref(masks=masks)
    r.backward()
    r.check_instances(gemm_mode == 'bf16x3')
    outs, grads = r.bwd_pairs(ref)
    compare(f'dense {case} {gemm_mode}', r.fwd_pairs(ref) + outs, grads)


# ----------------------------------------------------------------------------- each gradient source and each state member alone
SOURCES = [dict(dy=True, dhn=False, dcn=False), dict(dy=False, dhn=True, dcn=False), dict(dy=False, dhn=False, dcn=True)]


@pytest.mark.parametrize('dirs', [2, 1])
def test_each_gradient_source_alone(dirs, gemm_mode):
    """One forward, one backward per source: dy | dh_n | dc_n (the last one enters through the state call alone)."""
    d = Data(5, 4, 2, dirs, p=0.5, tag=3)
    r = Run(d).forward()
    masks = r.masks()
    for src in SOURCES:
        ref = d.ref(masks=masks, **src)
        r.backward(**src)
        r.check_instances(gemm_mode == 'bf16x3')
        outs, grads = r.bwd_pairs(ref)
        compare(f'source {[k for k, v in src.items() if v][0]} dirs={dirs} {gemm_mode}', outs, grads)


@pytest.mark.parametrize('members', [(True, False), (False, True), (False, False)], ids=['hx', 'cx', 'none'])
@pytest.mark.parametrize('want', [True, False], ids=['dhx-dcx', 'no-dhx'])
def test_each_state_member_alone(members, want, gemm_mode):
    """hx alone | cx alone | neither, with dhx / dcx asked for or not (not asked: the last step's matrix product is skipped)."""
    hx, cx = members
    d = Data(5, 4, 2, 2, tag=4)
    if hx or cx:
        d.state_guard(hx, cx)
    r = Run(d).forward(hx, cx)
    ref = d.ref(hx, cx)
    r.backward(want=want)
    r.check_instances(gemm_mode == 'bf16x3')
    outs, grads = r.bwd_pairs(ref)
    compare(f'members hx={int(hx)} cx={int(cx)} want={int(want)} {gemm_mode}', r.fwd_pairs(ref) + outs, grads)


# ----------------------------------------------------------------------------- lengths
@pytest.mark.parametrize('dirs', [2, 1])
def test_ragged_parity_and_the_pass_through(dirs, gemm_mode):
    """Lengths 0 .. T in every mix, p = 0.5, the whole state.  A row of length 0 returns dhx = dh_n and dcx = dc_n bit for bit; dx and the
    outputs are exactly 0 at dead positions (the dy given there is not zero: it is ignored, not added)."""
    d = ragged_data(dirs)
    assert (d.n == 0).any() and (d.n == 1).any() and (d.n == d.T).any() and np.abs(d.dy[d.pad]).min() > 0
    r = Run(d).forward()
    masks = r.masks()
    d.state_guard(masks=masks)
    ref = d.ref(masks=masks)
    r.backward()
    r.check_instances(gemm_mode == 'bf16x3')
    outs, grads = r.bwd_pairs(ref)
    compare(f'ragged dirs={dirs} {gemm_mode}', r.fwd_pairs(ref) + outs, grads)
    empty = d.n == 0
    assert np.array_equal(bits(r.dhx)[:, empty], bits(r.dhnd)[:, empty]), 'len 0: dhx is dh_n bit for bit'
    assert np.array_equal(bits(r.dcx)[:, empty], bits(r.dcnd)[:, empty]), 'len 0: dcx is dc_n bit for bit'
    assert np.array_equal(bits(r.h_n)[:, empty], bits(r.hxd)[:, empty]) and np.array_equal(bits(r.c_n)[:, empty], bits(r.cxd)[:, empty])
    assert not (host(r.dx)[d.pad] != 0).any() and not bits(r.y)[d.pad].any()


def test_ragged_without_a_state(gemm_mode):
    """dep_rnn_forward_varlen / dep_rnn_backward_varlen: the plain ragged pair on the same instances."""
    d = ragged_data(2)
    r = Run(d).forward(False, False)
    masks = r.masks()
    ref = d.ref(False, False, dcn=False, masks=masks)
    r.backward(dcn=False, want=False)
    r.check_instances(gemm_mode == 'bf16x3')
    outs, grads = r.bwd_pairs(ref)
    compare(f'ragged plain {gemm_mode}', r.fwd_pairs(ref) + outs, grads)


def test_reverse_direction_starts_inside_the_padding_from_cx(gemm_mode):
    """c_prev of a row's first forward step is cx: for direction 1 of a ragged row that step is t = len - 1, and the saved c at t = len is
    the dead position's 0.  The guard: on the reference, dropping cx moves the results by more than 100 bars."""
    d = trap_a_data()
    d.state_guard(hx=False, cx=True)
    r = Run(d).forward(False, True)
    ref = d.ref(False, True)
    r.backward()
    r.check_instances(gemm_mode == 'bf16x3')
    outs, grads = r.bwd_pairs(ref)
    compare(f'cx inside the padding {gemm_mode}', r.fwd_pairs(ref) + outs, grads)


@pytest.mark.parametrize('hx', [False, True], ids=['cx', 'hx-cx'])
@pytest.mark.parametrize('dirs', [2, 1])
def test_all_lengths_T_gives_the_dense_instances_bits(dirs, hx, gemm_mode):
    """Every output and gradient of the ragged instances at full lengths is the dense instances', bit for bit (cx, dh_n, dc_n, dhx, dcx
    all in play).  With hx as well, the one thing outside the sweeps that differs between the two calls is the hx term of dW_hh behind them
    -- a GEMM over the rows of one time step in the dense call, the gathering kernel dep_state_dwhh_ragged in the ragged one, as on
    every plan that takes hx with lengths -- so there dW_hh is held to the bar against the dense call and everything else to its bits."""
    B, T = 19, 7
    res, runs = [], []
    for lengths in (None, np.full(B, T)):
        d = Data(B, T, 2, dirs, lengths=lengths, p=0.5, tag=5)
        r = Run(d).forward(hx, True).backward()
        r.check_instances(gemm_mode == 'bf16x3')
        res.append(r.tensors()); runs.append(r)
    whh = [k for k in d.names if '.weight_hh_' in k] if hx else []
    same_bits(f'all lengths T dirs={dirs} hx={int(hx)} {gemm_mode}', res[1], res[0], but=whh)
    if hx:
        compare(f'all lengths T, dW_hh with the hx term dirs={dirs} {gemm_mode}', [], [(k.split('.', 1)[1], host(res[1][k]), host(res[0][k])) for k in whh])


# ----------------------------------------------------------------------------- pins to code that is already tested
@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_training_forward_is_the_dropout_only_forward_of_impl8_bit_for_bit(ragged, gemm_mode):
    """The saving instance is the same arithmetic with stores added: y, dropout(y), h_n, c_n equal an impl = 8 DEP_RUN_DROPOUT_ONLY forward's."""
    d = ragged_data(2) if ragged else Data(17, 5, 2, 2, p=0.5, tag=6)
    r9 = Run(d).forward()
    r8 = Run(d, impl=8, run=L.RUN_DROPOUT_ONLY).forward()
    assert r8.fwd_sweeps == [inst('lstm_fwd_local', gemm_mode == 'bf16x3', ragged)] * d.Lyr, r8.fwd_sweeps
    r9.check_instances(gemm_mode == 'bf16x3', backward=False)
    a = dict(y=r9.y, h_n=r9.h_n, c_n=r9.c_n, ydrop=r9.rnn.layer_output_dropped(0))
    b = dict(y=r8.y, h_n=r8.h_n, c_n=r8.c_n, ydrop=r8.rnn.layer_output_dropped(0))
    same_bits('train forward against impl 8', a, b)


@pytest.mark.parametrize('run', ['eval', 'dropout_only'])
def test_forwards_no_backward_follows_are_impl8s(run, gemm_mode):
    d = Data(17, 5, 2, 2, p=0.5 if run == 'dropout_only' else 0.0, tag=7)
    mode = L.RUN_DROPOUT_ONLY if run == 'dropout_only' else L.RUN_EVAL
    r9, r8 = Run(d, run=mode).forward(), Run(d, impl=8, run=mode).forward()
    want = [inst('lstm_fwd_local', gemm_mode == 'bf16x3', False)] * d.Lyr
    assert r9.fwd_sweeps == want and r8.fwd_sweeps == want, (r9.fwd_sweeps, r8.fwd_sweeps)
    same_bits(f'{run} forward against impl 8', dict(y=r9.y, h_n=r9.h_n, c_n=r9.c_n), dict(y=r8.y, h_n=r8.h_n, c_n=r8.c_n))


def test_gradients_agree_with_the_cluster_sweeps(gemm_mode):
    """Without a state, against impl = 3 (lstm_fwd_cluster / lstm_bwd_cluster): every output and gradient within twice the bar."""
    d = Data(40, 6, 2, 2, p=0.5, tag=8)
    r9 = Run(d).forward(False, False).backward(dcn=False, want=False)
    r9.check_instances(gemm_mode == 'bf16x3')
    r3 = Run(d, impl=3)
    r3.forward(False, False).backward(dcn=False, want=False)
    assert r3.bwd_sweeps and all(s.startswith('lstm_bwd_cluster<') for s in r3.bwd_sweeps), r3.bwd_sweeps
    assert np.array_equal(host(r9.rnn.layer_output_dropped(0)) == 0, host(r3.rnn.layer_output_dropped(0)) == 0), 'the dropped positions are the same'
    outs = [(n, host(getattr(r9, n)), host(getattr(r3, n))) for n in ('y', 'h_n', 'dx')]
    grads = [(k.split('.', 1)[1], host(a), host(b)) for k, a, b in zip(d.names, r9.Gd, r3.Gd)]
    compare(f'against impl = 3 {gemm_mode}', outs, grads, atol=2 * ATOL, rtol=2 * RTOL)


# ----------------------------------------------------------------------------- in-place state gradients
@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
def test_dhx_and_dcx_may_be_the_buffers_of_dh_n_and_dc_n(ragged, gemm_mode):
    """A lane reads only its own slice of dh_n / dc_n before it stores dhx / dcx there: the same bits as with separate buffers."""
    d = ragged_data(2) if ragged else Data(17, 3, 2, 2, tag=9)
    r = Run(d).forward().backward()
    apart = {k: v.clone() for k, v in r.tensors().items()}
    dhn_t, dcn_t = dev(d.dhn), dev(d.dcn)
    r.forward().backward(dhn_t=dhn_t, dcn_t=dcn_t, dhx_t=dhn_t, dcx_t=dcn_t)
    r.check_instances(gemm_mode == 'bf16x3')
    same_bits('in place', r.tensors(), apart)


# ----------------------------------------------------------------------------- independence
def test_two_streams_give_the_bits_of_two_steps_in_turn(gemm_mode):
    """Two training steps (forward + backward) on two streams, each with its own Rnn: nothing is shared, so what runs beside a sweep
    cannot change its result.  One run, no repetition."""
    data = [Data(40, 6, 2, 2, p=0.5, tag=10 + i) for i in range(2)]
    runs = [Run(dd) for dd in data]
    turn = []
    for r in runs:
        r.forward().backward()
        torch.cuda.synchronize()
        r.check_instances(gemm_mode == 'bf16x3')
        turn.append({k: bits(v) for k, v in r.tensors().items()})
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    for r, s in zip(runs, streams):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            r.forward().backward()
    torch.cuda.synchronize()
    for r, t in zip(runs, turn):
        for n, v in r.tensors().items():
            assert np.isfinite(host(v)).all(), n
            assert np.array_equal(bits(v), t[n]), n
