"""impl = 5, "the per-layer cluster sweeps, state through training", the parts that need no GPU: the descriptor exists exactly where
impl = 4 does, with impl = 4's layout queries, and the state rule of the entry points (include/dep_rnn.h): hx in a DEP_RUN_TRAIN
forward and hx / dhx in both backward state calls pass it, the cell state stays the LSTM's, and a state-bearing backward is refused in
GEMM modes 2 / 3 before any HIP call."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = C.c_size_t(-1).value
FAKE = 0x1000           # a non-NULL pointer: the refusals under test come before anything reads it
ERR_ARG = -1
HS = (64, 128, 256, 512)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib
    return _lib, _lib.load()


def gru(_lib, impl, H, run, B=4, T=3, Lyr=2, p=0.0, pool=0):
    return _lib.RnnDesc(_lib.CELL_GRU, B, T, 8, H, Lyr, 1, run, p, 0, pool, impl)


def on_the_cluster_layout(_lib, so, d):
    """The descriptor is planned onto the per-layer cluster sweeps, not silently onto the tile sweeps (which take a state on any impl
    without a cluster layout): it has an exchange buffer, at impl = 4's offset, and impl = 4's sizes."""
    d4 = _lib.RnnDesc(d.cell, d.B, d.T, d.F, d.H, d.L, d.dirs, d.training, d.dropout_p, 0, d.pool, 4)
    off = so.dep_rnn_workspace_xbuf_offset(C.byref(d))
    return off != NONE and off == so.dep_rnn_workspace_xbuf_offset(C.byref(d4)) and \
        so.dep_rnn_workspace_bytes(C.byref(d)) == so.dep_rnn_workspace_bytes(C.byref(d4)) > 0


def fwd(so, desc, st, lengths=None):
    s = None if st is None else C.byref(st)
    if lengths is None:
        return so.dep_rnn_forward_state(C.byref(desc), None, None, None, None, None, s, None, 0, None, 0, None)
    return so.dep_rnn_forward_state_varlen(C.byref(desc), None, lengths, None, None, None, None, s, None, 0, None, 0, None)


def bwd(so, desc, st, lengths=None):
    s = None if st is None else C.byref(st)
    if lengths is None:
        return so.dep_rnn_backward_state(C.byref(desc), None, None, None, None, None, s, None, None, None, 0, None, 0, None, None)
    return so.dep_rnn_backward_state_varlen(C.byref(desc), None, lengths, None, None, None, None, s, None, None, None, 0, None, 0, None, None)


def test_the_binding_names_the_value(lib):
    _lib, _ = lib
    assert _lib.IMPL_CLUSTER_PER_LAYER_STATE == 5 and _lib.IMPL_CLUSTER_PER_LAYER == 4
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    assert '5 the per-layer cluster sweeps, state through training' in header


@pytest.mark.parametrize('H', HS)
def test_impl5_exists_where_impl4_does_with_the_same_layout(lib, H):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        for B, T, Lyr in ((4, 3, 2), (517, 2, 1), (5, 1, 3)):
            p = 0.5 if run else 0.0
            d5, d4 = gru(_lib, 5, H, run, B, T, Lyr, p=p), gru(_lib, 4, H, run, B, T, Lyr, p=p)
            assert so.dep_rnn_reserve_bytes(C.byref(d5)) == so.dep_rnn_reserve_bytes(C.byref(d4)) > 0, (H, run, B)
            assert so.dep_rnn_workspace_bytes(C.byref(d5)) == so.dep_rnn_workspace_bytes(C.byref(d4)) > 0, (H, run, B)
            assert so.dep_rnn_workspace_xbuf_offset(C.byref(d5)) == so.dep_rnn_workspace_xbuf_offset(C.byref(d4)) != NONE
            for l in range(Lyr):
                assert so.dep_rnn_reserve_y_offset(C.byref(d5), l) == so.dep_rnn_reserve_y_offset(C.byref(d4), l)
                assert so.dep_rnn_reserve_ydrop_offset(C.byref(d5), l) == so.dep_rnn_reserve_ydrop_offset(C.byref(d4), l)


BAD = [('lstm', 128, 2), ('lstm', 128, 1), ('lstm', 256, 1), ('gru', 256, 2), ('gru', 64, 2), ('gru', 16, 1), ('gru', 48, 1), ('gru', 96, 1)]


@pytest.mark.parametrize('cell,H,dirs', BAD)
def test_every_other_impl5_descriptor_is_bad_with_the_rule(lib, cell, H, dirs):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN):
        d = _lib.RnnDesc(_lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM, 4, 3, 8, H, 2, dirs, run, 0.0, 0, 0, 5)
        for query in (so.dep_rnn_reserve_bytes, so.dep_rnn_workspace_bytes):
            assert query(C.byref(d)) == 0
            msg = so.dep_last_error().decode()
            assert 'impl = 5' in msg and 'unidirectional GRU' in msg and '{64, 128, 256, 512}' in msg, msg
        assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) == NONE
        assert so.dep_rnn_reserve_y_offset(C.byref(d), 0) == NONE
        calls = [('dep_rnn_forward', lambda: so.dep_rnn_forward(C.byref(d), None, None, None, None, None, None, 0, None, 0, None)),
                 ('dep_rnn_backward', lambda: so.dep_rnn_backward(C.byref(d), None, None, None, None, None, None, None, None, 0, None, 0, None)),
                 ('dep_rnn_forward', lambda: fwd(so, d, _lib.RnnState(FAKE, None, None))),
                 ('dep_rnn_backward', lambda: bwd(so, d, _lib.RnnStateGrad(FAKE, None, None, FAKE, None))),
                 ('dep_rnn_forward', lambda: fwd(so, d, None, lengths=FAKE)),
                 ('dep_rnn_backward', lambda: bwd(so, d, None, lengths=FAKE))]
        for who, call in calls:
            assert call() == ERR_ARG
            msg = so.dep_last_error().decode()
            assert who in msg and 'impl = 5' in msg and f'H = {H}' in msg and f'dirs = {dirs}' in msg, msg
    with pytest.raises(_lib.DepError, match='impl = 5'):
        _lib.Rnn(_lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM, 4, 3, 8, H, 2, dirs, False, 0.0, 0, 'cpu', impl=5)


@pytest.mark.parametrize('H', HS)
def test_hx_in_every_forward_passes_the_state_rule(lib, H):
    """DEP_RUN_TRAIN included: the call gets as far as the plain call's own argument checks (x, weights are NULL)."""
    _lib, so = lib
    for run in (_lib.RUN_TRAIN, _lib.RUN_EVAL, _lib.RUN_DROPOUT_ONLY):
        d = gru(_lib, 5, H, run, p=0.5 if run else 0.0)
        assert on_the_cluster_layout(_lib, so, d)
        for lengths in (None, FAKE):
            for st in (_lib.RnnState(FAKE, None, None), _lib.RnnState(None, None, None), None):
                assert fwd(so, d, st, lengths) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert 'bad argument: x && weights' in msg and 'impl = ' not in msg and 'cluster exchange buffer' not in msg, msg


@pytest.mark.parametrize('H', HS)
def test_hx_and_dhx_in_both_backward_state_calls_pass_the_state_rule(lib, H):
    _lib, so = lib
    d = gru(_lib, 5, H, _lib.RUN_TRAIN)
    assert on_the_cluster_layout(_lib, so, d)
    for mode in (0, 1):
        _lib.set_gemm_mode(mode, 0)
        try:
            for lengths in (None, FAKE):
                for members in (('hx',), ('dhx',), ('hx', 'dhx')):
                    sg = _lib.RnnStateGrad(None, None, None, None, None)
                    for m in members:
                        setattr(sg, m, FAKE)
                    assert bwd(so, d, sg, lengths) == ERR_ARG
                    msg = so.dep_last_error().decode()
                    assert 'bad argument: x && weights' in msg and 'impl = ' not in msg and 'takes no state' not in msg, (members, msg)
        finally:
            _lib.set_gemm_mode(1, 1 << 28)


@pytest.mark.parametrize('H', HS)
def test_the_cell_state_stays_the_lstms(lib, H):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN):
        d = gru(_lib, 5, H, run)
        assert on_the_cluster_layout(_lib, so, d)
        for member in ('cx', 'c_n'):
            st = _lib.RnnState(None, None, None)
            setattr(st, member, FAKE)
            for lengths in (None, FAKE):
                assert fwd(so, d, st, lengths) == ERR_ARG and "LSTM's cell state" in so.dep_last_error().decode()
        for member in ('cx', 'dc_n', 'dcx'):
            sg = _lib.RnnStateGrad(None, None, None, None, None)
            setattr(sg, member, FAKE)
            for lengths in (None, FAKE):
                assert bwd(so, d, sg, lengths) == ERR_ARG and "LSTM's cell state" in so.dep_last_error().decode()


@pytest.mark.parametrize('mode', [2, 3])
def test_a_state_bearing_backward_is_refused_in_the_single_product_modes(lib, mode):
    _lib, so = lib
    _lib.set_gemm_mode(mode, 0)
    try:
        for H in HS:
            d = gru(_lib, 5, H, _lib.RUN_TRAIN)
            for member in ('hx', 'dhx'):
                sg = _lib.RnnStateGrad(None, None, None, None, None)
                setattr(sg, member, FAKE)
                assert bwd(so, d, sg) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert 'dep_rnn_backward_state' in msg and 'impl = 5' in msg and 'GEMM modes 0 and 1 only' in msg and \
                    f'the current mode is {mode}' in msg, msg
            # the plain call on the same descriptor is not a state call: it gets to its own argument checks
            assert bwd(so, d, None) == ERR_ARG and 'bad argument: x && weights' in so.dep_last_error().decode()
            # ... and so does the forward with hx (the forward kernel has no storage variant)
            assert fwd(so, d, _lib.RnnState(FAKE, None, None)) == ERR_ARG and 'bad argument: x && weights' in so.dep_last_error().decode()
    finally:
        _lib.set_gemm_mode(1, 1 << 28)


def test_impl4_keeps_its_refusals(lib):
    """The published contract of impl = 4 (tests/test_state_cluster_cpu.py) next to the new value."""
    _lib, so = lib
    d4, d5 = gru(_lib, 4, 256, _lib.RUN_TRAIN), gru(_lib, 5, 256, _lib.RUN_TRAIN)
    assert on_the_cluster_layout(_lib, so, d5)
    assert fwd(so, d4, _lib.RnnState(FAKE, None, None)) == ERR_ARG and 'impl = 4' in so.dep_last_error().decode()
    assert bwd(so, d4, _lib.RnnStateGrad(FAKE, None, None, FAKE, None)) == ERR_ARG and 'cluster backward takes no state' in so.dep_last_error().decode()
    assert fwd(so, d5, _lib.RnnState(FAKE, None, None)) == ERR_ARG and 'x && weights' in so.dep_last_error().decode()
