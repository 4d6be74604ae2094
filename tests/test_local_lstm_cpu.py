"""impl = 8, "the exchange-free per-layer LSTM forward", the parts that need no GPU: which descriptors exist, that they have no
exchange buffer, that y / dropout(y) sit where impl = 3 has them, and the refusals made before any HIP call (include/dep_rnn.h).
Every test here fails on the commit in front of impl = 8, where the value is a bad descriptor or a plain tile-sweep one."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = C.c_size_t(-1).value
FAKE = 0x1000           # a non-NULL pointer: the refusals under test come before anything reads it
ERR_ARG = -1
SHAPES = ((4, 3, 2), (517, 2, 1), (3, 2, 8))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib
    return _lib, _lib.load()


def desc(_lib, run, B=4, T=3, Lyr=2, p=0.0, impl=8, cell=None, dirs=2, F=8, H=128):
    return _lib.RnnDesc(_lib.CELL_LSTM if cell is None else cell, B, T, F, H, Lyr, dirs, run, p, 0, 0, impl)


def fwd(so, d, st, lengths=None):
    s = None if st is None else C.byref(st)
    if lengths is None:
        return so.dep_rnn_forward_state(C.byref(d), None, None, None, None, None, s, None, 0, None, 0, None)
    return so.dep_rnn_forward_state_varlen(C.byref(d), None, lengths, None, None, None, None, s, None, 0, None, 0, None)


def backward_calls(_lib, so, d):
    """Every backward entry point, with the arguments its own pre-checks want (lengths, a grad-sync struct) non-NULL."""
    gs = _lib.GradSync()
    gs.comm, gs.comm_stream = FAKE, FAKE + 16          # (a communication stream other than the call's, which is NULL)
    g = C.byref(gs)
    sg = _lib.RnnStateGrad(FAKE, None, None, None, None)
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
    assert _lib.IMPL_LOCAL_LSTM == 8
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    assert '8 the exchange-free per-layer LSTM forward' in header
    assert 'on an impl = 8 descriptor (the exchange-free per-layer LSTM forward) hx, cx and c_n are accepted' in header
    # the health comment lists the impls that have an exchange buffer: 8 is not one of them
    assert 'desc.impl 0/3/4/5/6/7 with a' in header


@pytest.mark.parametrize('dirs', (1, 2))
def test_impl8_exists_without_an_exchange_buffer_on_impl3s_offsets(lib, dirs):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_DROPOUT_ONLY):
        for B, T, Lyr in SHAPES:
            for p in ((0.0,) if run == _lib.RUN_EVAL else (0.0, 0.5)):
                d8 = desc(_lib, run, B, T, Lyr, p=p, dirs=dirs)
                d3 = desc(_lib, run, B, T, Lyr, p=p, dirs=dirs, impl=3)
                assert so.dep_rnn_reserve_bytes(C.byref(d8)) > 0 and so.dep_rnn_workspace_bytes(C.byref(d8)) > 0, (run, B, T, Lyr)
                assert so.dep_rnn_workspace_xbuf_offset(C.byref(d8)) == NONE
                assert so.dep_rnn_workspace_xbuf_offset(C.byref(d3)) != NONE
                kept = 0
                for l in range(Lyr):
                    assert so.dep_rnn_reserve_y_offset(C.byref(d8), l) == so.dep_rnn_reserve_y_offset(C.byref(d3), l), (run, l)
                    assert so.dep_rnn_reserve_ydrop_offset(C.byref(d8), l) == so.dep_rnn_reserve_ydrop_offset(C.byref(d3), l), (run, l)
                    kept += so.dep_rnn_reserve_y_offset(C.byref(d8), l) != NONE
                assert so.dep_rnn_reserve_y_offset(C.byref(d8), Lyr - 1) != NONE and kept >= 1
                # the packed forward weight image is in the reserve: one (4H x H) image per (layer, direction) on top of the sequences
                assert so.dep_rnn_reserve_bytes(C.byref(d8)) >= (kept * B * T * dirs * 128 + Lyr * dirs * 4 * 128 * 128) * 4
                # no exchange buffer: the workspace is smaller than the cluster descriptor's
                assert so.dep_rnn_workspace_bytes(C.byref(d8)) < so.dep_rnn_workspace_bytes(C.byref(d3))
    # the status query needs no device on a plan without an exchange buffer
    assert so.dep_rnn_status(C.byref(desc(_lib, _lib.RUN_EVAL, dirs=dirs)), FAKE, None) == 0


BAD = [('train', {}), ('gru', {}), ('H', {'H': 64}), ('H', {'H': 256}), ('L', {'Lyr': 9})]


@pytest.mark.parametrize('what,kw', BAD, ids=[w + ''.join(str(v) for v in k.values()) for w, k in BAD])
def test_every_other_impl8_descriptor_is_bad_with_the_rule(lib, what, kw):
    _lib, so = lib
    for dirs in (1, 2):
        run = _lib.RUN_TRAIN if what == 'train' else _lib.RUN_EVAL
        d = desc(_lib, run, dirs=dirs, cell=_lib.CELL_GRU if what == 'gru' else None, **kw)
        for query in (so.dep_rnn_reserve_bytes, so.dep_rnn_workspace_bytes):
            assert query(C.byref(d)) == 0
            msg = so.dep_last_error().decode()
            assert 'impl = 8' in msg and 'exchange-free' in msg and 'H = 128' in msg, msg
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
            assert who in msg and 'impl = 8' in msg and f'H = {d.H}' in msg and f'run mode = {run}' in msg, msg
        with pytest.raises(_lib.DepError, match='impl = 8'):
            _lib.Rnn(d.cell, 4, 3, 8, d.H, d.L, dirs, run, 0.0, 0, 'cpu', impl=8)


def test_every_backward_entry_point_is_refused_before_any_launch(lib):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_DROPOUT_ONLY):
        for dirs in (1, 2):
            d = desc(_lib, run, dirs=dirs, p=0.5 if run else 0.0)
            for who, call in backward_calls(_lib, so, d):
                assert call() == ERR_ARG, who
                msg = so.dep_last_error().decode()
                assert 'dep_rnn_backward' in msg and 'impl = 8' in msg and 'no backward' in msg, (who, msg)


def test_the_state_is_accepted_by_the_forward_state_calls(lib):
    """hx, cx and c_n pass the state rule: the call gets as far as the plain call's own argument checks (x, weights, reserve and
    workspace are NULL), dense and ragged, in both run modes."""
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_DROPOUT_ONLY):
        for dirs in (1, 2):
            d = desc(_lib, run, dirs=dirs, p=0.5 if run else 0.0)
            for lengths in (None, FAKE):
                for st in (_lib.RnnState(FAKE, FAKE, FAKE), _lib.RnnState(None, FAKE, None), _lib.RnnState(None, None, FAKE),
                           _lib.RnnState(FAKE, None, None), None):
                    assert fwd(so, d, st, lengths) == ERR_ARG
                    msg = so.dep_last_error().decode()
                    assert 'bad argument: x && weights' in msg and 'impl = 8' not in msg, msg
    # ... where the cluster BiLSTM descriptor refuses them
    d3 = desc(_lib, _lib.RUN_EVAL, impl=3)
    assert fwd(so, d3, _lib.RnnState(FAKE, FAKE, FAKE)) == ERR_ARG and 'recurrent state' in so.dep_last_error().decode()


def test_the_single_product_modes(lib):
    """A ragged call runs in modes 0 and 1 only, as on every plan; a dense forward runs in all four."""
    _lib, so = lib
    d = desc(_lib, _lib.RUN_EVAL)
    try:
        for m in (2, 3):
            _lib.set_gemm_mode(m, 0)
            assert fwd(so, d, None, lengths=FAKE) == ERR_ARG
            msg = so.dep_last_error().decode()
            assert 'GEMM modes 0 and 1 only' in msg and f'current mode is {m}' in msg, msg
            assert fwd(so, d, None) == ERR_ARG and 'bad argument: x && weights' in so.dep_last_error().decode()
    finally:
        _lib.set_gemm_mode(1, 1 << 28)


def test_the_instance_table_lists_the_four_rows(lib):
    _lib, _ = lib
    rows = [r.strip('()') for r in _lib.instance_table_read() if 'lstm_fwd_local' in r]
    assert sorted(rows) == sorted(f'lstm_fwd_local<{s}, {r}>' for s in ('false', 'true') for r in ('false', 'true')), rows


def test_model_choices_are_checked_without_a_gpu(lib):
    _lib, _ = lib
    from icassp2022_depression_amd import models
    assert models._local_lstm_choice(None, 'x', 1024, 128, 2) == _lib.IMPL_AUTO
    assert models._local_lstm_choice(8, 'x', 1024, 128, 2) == _lib.IMPL_LOCAL_LSTM
    for bad in (0, 3, 7, 9, '8', True, 8.0):
        with pytest.raises(_lib.DepError, match='exchange-free'):
            models._local_lstm_choice(bad, "config['text_impl']", 1024, 128, 2)
    with pytest.raises(_lib.DepError, match='impl = 8'):          # the descriptor does not exist at this width
        models._local_lstm_choice(8, "config['text_impl']", 1024, 256, 2)
    from icassp2022_depression_amd import fuse_net, fuse_net_whole
    assert fuse_net.config['text_impl'] is None and fuse_net_whole.config['text_impl'] is None
