"""impl = 9, "the exchange-free per-layer LSTM sweeps, forward and backward", the parts that need no GPU: which descriptors exist, that
they have no exchange buffer, where the reserve keeps what, and the refusals made before any HIP call (include/dep_rnn.h); and, on the
float64 reference alone, that the state of the GPU test's cases matters by more than 100 bars.
Every test here fails on the commit in front of impl = 9, where the value is a plain tile-sweep descriptor without the rules."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = C.c_size_t(-1).value
FAKE = 0x1000           # a non-NULL pointer: the refusals under test come before anything reads it
ERR_ARG = -1
SHAPES = ((4, 3, 2), (517, 2, 1), (3, 2, 8))
H = 128


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib
    return _lib, _lib.load()


def desc(_lib, run, B=4, T=3, Lyr=2, p=0.0, impl=9, cell=None, dirs=2, F=8, H=H):
    return _lib.RnnDesc(_lib.CELL_LSTM if cell is None else cell, B, T, F, H, Lyr, dirs, run, p, 0, 0, impl)


def fwd(so, d, st, lengths=None):
    s = None if st is None else C.byref(st)
    if lengths is None:
        return so.dep_rnn_forward_state(C.byref(d), None, None, None, None, None, s, None, 0, None, 0, None)
    return so.dep_rnn_forward_state_varlen(C.byref(d), None, lengths, None, None, None, None, s, None, 0, None, 0, None)


def backward_calls(_lib, so, d, sg=None):
    """Every backward entry point, with the arguments its own pre-checks want (lengths, a grad-sync struct) non-NULL."""
    gs = _lib.GradSync()
    gs.comm, gs.comm_stream = FAKE, FAKE + 16          # (a communication stream other than the call's, which is NULL)
    g = C.byref(gs)
    sg = _lib.RnnStateGrad(FAKE, None, None, None, None) if sg is None else sg
    tail = (None, None, None, 0, None, 0, None)      # dweights, dx, reserve, bytes, workspace, bytes, stream
    return [
        ('dep_rnn_backward', lambda: so.dep_rnn_backward(C.byref(d), None, None, None, None, None, *tail)),
        ('dep_rnn_backward_varlen', lambda: so.dep_rnn_backward_varlen(C.byref(d), None, FAKE, None, None, None, None, *tail)),
        ('dep_rnn_backward_state', lambda: so.dep_rnn_backward_state(C.byref(d), None, None, None, None, None, C.byref(sg), *tail, None)),
        ('dep_rnn_backward_state (no state)', lambda: so.dep_rnn_backward_state(C.byref(d), None, None, None, None, None, None, *tail, None)),
        ('dep_rnn_backward_state_varlen', lambda: so.dep_rnn_backward_state_varlen(C.byref(d), None, FAKE, None, None, None, None, C.byref(sg), *tail, None)),
        ('dep_rnn_backward_overlapped', lambda: so.dep_rnn_backward_overlapped(C.byref(d), None, None, None, None, None, *tail, g)),
        ('dep_rnn_backward_overlapped_varlen', lambda: so.dep_rnn_backward_overlapped_varlen(C.byref(d), None, FAKE, None, None, None, None, *tail, g)),
    ]


def test_the_binding_and_the_header_name_the_value(lib):
    _lib, _ = lib
    assert _lib.IMPL_LOCAL_LSTM_TRAIN == 9 and _lib.IMPL_LOCAL_LSTM == 8
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    assert '9 the exchange-free per-layer LSTM sweeps, forward and backward' in header
    assert 'on an impl = 9 descriptor (the exchange-free per-layer LSTM sweeps, forward and backward) every member is accepted' in header


@pytest.mark.parametrize('dirs', (1, 2))
def test_impl9_exists_in_all_three_run_modes_without_an_exchange_buffer_on_impl3s_offsets(lib, dirs):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        for B, T, Lyr in SHAPES:
            for p in ((0.0,) if run == _lib.RUN_EVAL else (0.0, 0.5)):
                d9 = desc(_lib, run, B, T, Lyr, p=p, dirs=dirs)
                d3 = desc(_lib, run, B, T, Lyr, p=p, dirs=dirs, impl=3)
                assert so.dep_rnn_reserve_bytes(C.byref(d9)) > 0 and so.dep_rnn_workspace_bytes(C.byref(d9)) > 0, (run, B, T, Lyr)
                assert so.dep_rnn_workspace_xbuf_offset(C.byref(d9)) == NONE
                assert so.dep_rnn_workspace_xbuf_offset(C.byref(d3)) != NONE
                for l in range(Lyr):
                    assert so.dep_rnn_reserve_y_offset(C.byref(d9), l) == so.dep_rnn_reserve_y_offset(C.byref(d3), l), (run, l)
                    assert so.dep_rnn_reserve_ydrop_offset(C.byref(d9), l) == so.dep_rnn_reserve_ydrop_offset(C.byref(d3), l), (run, l)
                assert so.dep_rnn_reserve_y_offset(C.byref(d9), Lyr - 1) != NONE
                assert so.dep_rnn_workspace_bytes(C.byref(d9)) < so.dep_rnn_workspace_bytes(C.byref(d3))
                if run != _lib.RUN_TRAIN:       # the forwards no backward follows: impl = 8's sizes
                    d8 = desc(_lib, run, B, T, Lyr, p=p, dirs=dirs, impl=8)
                    assert so.dep_rnn_reserve_bytes(C.byref(d9)) == so.dep_rnn_reserve_bytes(C.byref(d8))
                    assert so.dep_rnn_workspace_bytes(C.byref(d9)) == so.dep_rnn_workspace_bytes(C.byref(d8))
        # the status query needs no device on a plan without an exchange buffer
        assert so.dep_rnn_status(C.byref(desc(_lib, run, dirs=dirs)), FAKE, None) == 0


@pytest.mark.parametrize('dirs', (1, 2))
def test_a_training_reserve_keeps_the_gates_the_cell_state_and_both_weight_images(lib, dirs):
    _lib, so = lib
    for B, T, Lyr in SHAPES:
        for p in (0.0, 0.5):
            train = so.dep_rnn_reserve_bytes(C.byref(desc(_lib, _lib.RUN_TRAIN, B, T, Lyr, p=p, dirs=dirs)))
            donly = so.dep_rnn_reserve_bytes(C.byref(desc(_lib, _lib.RUN_DROPOUT_ONLY, B, T, Lyr, p=p, dirs=dirs)))
            saved = Lyr * B * T * dirs * (4 * H + H) * 4                 # fp32 activated gates and c of every layer
            images = Lyr * dirs * 4 * H * H * 4                          # the backward's W_hh image beside the forward's
            assert train >= donly + saved + images, (B, T, Lyr, p, train, donly)


BAD = [('gru', {}), ('H', {'H': 64}), ('H', {'H': 256}), ('L', {'Lyr': 9})]


@pytest.mark.parametrize('what,kw', BAD, ids=[w + ''.join(str(v) for v in k.values()) for w, k in BAD])
def test_every_other_impl9_descriptor_is_bad_with_the_rule(lib, what, kw):
    _lib, so = lib
    for dirs in (1, 2):
        for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
            d = desc(_lib, run, dirs=dirs, cell=_lib.CELL_GRU if what == 'gru' else None, **kw)
            for query in (so.dep_rnn_reserve_bytes, so.dep_rnn_workspace_bytes):
                assert query(C.byref(d)) == 0
                msg = so.dep_last_error().decode()
                assert 'impl = 9' in msg and 'exchange-free' in msg and 'H = 128' in msg, msg
            assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) == NONE
            assert so.dep_rnn_reserve_y_offset(C.byref(d), 0) == NONE
            calls = [('dep_rnn_forward', lambda: so.dep_rnn_forward(C.byref(d), None, None, None, None, None, None, 0, None, 0, None)),
                     ('dep_rnn_forward', lambda: so.dep_rnn_forward_varlen(C.byref(d), None, FAKE, None, None, None, None, None, 0, None, 0, None)),
                     ('dep_rnn_forward', lambda: fwd(so, d, _lib.RnnState(FAKE, FAKE, FAKE))),
                     ('dep_rnn_forward', lambda: fwd(so, d, None, lengths=FAKE))]
            calls += [('dep_rnn_backward', c) for _, c in backward_calls(_lib, so, d)]
            for who, call in calls:
                assert call() == ERR_ARG
                msg = so.dep_last_error().decode()
                assert who in msg and 'impl = 9' in msg and f'H = {d.H}' in msg and f'run mode = {run}' in msg, msg
        with pytest.raises(_lib.DepError, match='impl = 9'):
            _lib.Rnn(d.cell, 4, 3, 8, d.H, d.L, dirs, _lib.RUN_TRAIN, 0.0, 0, 'cpu', impl=9)


def test_every_backward_entry_point_and_state_member_passes_the_impl_rules(lib):
    """A DEP_RUN_TRAIN descriptor: every entry point, with any state member, gets as far as the plain call's own argument checks (x,
    weights, dweights, reserve and workspace are NULL), where impl = 8 stops at "no backward" and impl = 3 at the state rule."""
    _lib, so = lib
    members = [_lib.RnnStateGrad(*[FAKE if i == k else None for i in range(5)]) for k in range(5)] + [_lib.RnnStateGrad(FAKE, FAKE, FAKE, FAKE, FAKE)]
    for dirs in (1, 2):
        d = desc(_lib, _lib.RUN_TRAIN, dirs=dirs, p=0.5)
        for sg in members:
            for who, call in backward_calls(_lib, so, d, sg):
                assert call() == ERR_ARG, who
                msg = so.dep_last_error().decode()
                assert 'bad argument: x && weights' in msg and 'impl = 9' not in msg, (who, msg)
        d3 = desc(_lib, _lib.RUN_TRAIN, dirs=dirs, impl=3)
        assert so.dep_rnn_backward_state(C.byref(d3), None, None, None, None, None, C.byref(members[-1]), None, None, None, 0, None, 0, None, None) == ERR_ARG
        assert 'recurrent state' in so.dep_last_error().decode()


def test_the_state_is_accepted_by_every_forward(lib):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        for dirs in (1, 2):
            d = desc(_lib, run, dirs=dirs, p=0.5 if run else 0.0)
            for lengths in (None, FAKE):
                for st in (_lib.RnnState(FAKE, FAKE, FAKE), _lib.RnnState(None, FAKE, None), _lib.RnnState(None, None, FAKE),
                           _lib.RnnState(FAKE, None, None), None):
                    assert fwd(so, d, st, lengths) == ERR_ARG
                    msg = so.dep_last_error().decode()
                    assert 'bad argument: x && weights' in msg and 'impl = 9' not in msg, msg


def test_training_runs_in_the_parity_modes_only(lib):
    """The training forward and every backward entry point are refused in GEMM modes 2 / 3 with the rule naming impl = 9, before any
    launch; the forwards no backward follows run in all four modes, as on impl = 8."""
    _lib, so = lib
    try:
        for m in (2, 3):
            _lib.set_gemm_mode(m, 0)
            d = desc(_lib, _lib.RUN_TRAIN, p=0.5)
            for lengths in (None, FAKE):
                assert fwd(so, d, None, lengths) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert 'dep_rnn_forward' in msg and 'impl = 9' in msg and 'GEMM modes 0 and 1 only' in msg and f'current mode is {m}' in msg, msg
            for who, call in backward_calls(_lib, so, d):
                assert call() == ERR_ARG, who
                msg = so.dep_last_error().decode()
                assert 'dep_rnn_backward' in msg and 'impl = 9' in msg and 'GEMM modes 0 and 1 only' in msg and f'current mode is {m}' in msg, (who, msg)
            for run in (_lib.RUN_EVAL, _lib.RUN_DROPOUT_ONLY):
                assert fwd(so, desc(_lib, run), None) == ERR_ARG and 'bad argument: x && weights' in so.dep_last_error().decode()
        for m in (0, 1):
            _lib.set_gemm_mode(m, 0)
            assert fwd(so, desc(_lib, _lib.RUN_TRAIN), None) == ERR_ARG and 'bad argument: x && weights' in so.dep_last_error().decode()
    finally:
        _lib.set_gemm_mode(1, 1 << 28)


def test_a_backward_needs_a_training_descriptor(lib):
    """DEP_RUN_EVAL / DEP_RUN_DROPOUT_ONLY descriptors: the existing run-mode message, in every GEMM mode."""
    _lib, so = lib
    try:
        for m in (1, 2):
            _lib.set_gemm_mode(m, 0)
            for run in (_lib.RUN_EVAL, _lib.RUN_DROPOUT_ONLY):
                d = desc(_lib, run, p=0.5 if run else 0.0)
                for who, call in backward_calls(_lib, so, d):
                    if m == 2 and 'varlen' in who:
                        continue          # (a ragged call in mode 2 meets the ragged-mode rule first, as on every plan)
                    assert call() == ERR_ARG, who
                    msg = so.dep_last_error().decode()
                    assert f"the descriptor's run mode is {run}" in msg and 'DEP_RUN_TRAIN' in msg, (who, msg)
    finally:
        _lib.set_gemm_mode(1, 1 << 28)


def test_the_instance_table_lists_the_new_rows_and_keeps_the_old(lib):
    _lib, _ = lib
    table = [r.strip('()') for r in _lib.instance_table_read()]
    four = lambda k: sorted(f'{k}<{s}, {r}>' for s in ('false', 'true') for r in ('false', 'true'))
    for kernel in ('lstm_fwd_save_local', 'lstm_bwd_local'):
        assert sorted(r for r in table if r.startswith(kernel + '<')) == four(kernel), kernel
    assert sorted(r for r in table if 'lstm_fwd_local' in r) == four('lstm_fwd_local')
    assert len([r for r in table if '_local<' in r]) == 12


def test_the_models_training_choice_is_checked_without_a_gpu(lib):
    _lib, _ = lib
    from icassp2022_depression_amd import models, text_bilstm_perm, text_bilstm_whole
    assert models._local_lstm_train_choice(None, 'x', 1024, 128, 2) == _lib.IMPL_AUTO
    assert models._local_lstm_train_choice(9, 'x', 1024, 128, 2) == _lib.IMPL_LOCAL_LSTM_TRAIN
    for bad in (0, 3, 7, 8, '9', True, 9.0):
        with pytest.raises(_lib.DepError, match="train_impl.*exchange-free"):
            models._local_lstm_train_choice(bad, "config['train_impl']", 1024, 128, 2)
    with pytest.raises(_lib.DepError, match='impl = 9'):          # the descriptor does not exist at this width
        models._local_lstm_train_choice(9, "config['train_impl']", 1024, 256, 2)
    assert text_bilstm_whole.config['train_impl'] is None and text_bilstm_perm.config['train_impl'] is None
    assert models._local_lstm_choice(None, 'x', 1024, 128, 2) == _lib.IMPL_AUTO          # the forward-only helper is as it was
    with pytest.raises(_lib.DepError, match='exchange-free'):
        models._local_lstm_choice(9, 'x', 1024, 128, 2)


# ----------------------------------------------------------------------------- the GPU test's cases, on the reference alone
def test_the_state_of_the_gpu_tests_cases_matters_by_more_than_100_bars():
    """dW_hh, dx and dhx of the float64 reference with the state against without it, on the very data tests/test_local_lstm_train_gpu.py
    uses (tests/local_lstm_train_cases.py) (without the dropout masks, which come from the device there; that file asserts the same with them)."""
    import local_lstm_train_cases as G
    figs = {str(c): G.dense_data(c).state_guard() for c in G.dense_cases()}
    figs.update({f'ragged dirs={dirs}': G.ragged_data(dirs).state_guard() for dirs in (2, 1)})
    figs['cx inside the padding'] = G.trap_a_data().state_guard(hx=False, cx=True)
    d = G.Data(5, 4, 2, 2, tag=4)
    figs['hx alone'], figs['cx alone'] = d.state_guard(True, False), d.state_guard(False, True)
    for k, v in figs.items():
        print(f'local-lstm-train guard {k}: dW_hh {v[0]:.0f}, dx {v[1]:.0f}, dhx {v[2]:.0f} bars')
    # trap (a) is a case at all: rows whose reverse direction starts inside the padding
    t = G.trap_a_data()
    assert (t.n < t.T).sum() >= 2 and (t.n > 0).all()
