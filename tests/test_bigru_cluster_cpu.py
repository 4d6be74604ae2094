"""impl = 6, "the per-layer cluster forward of a bidirectional GRU", the parts that need no GPU: which descriptors exist, that the
workspace has an exchange buffer while impl = 0 keeps none, that the reserve is laid out as impl = 2's (the tile-MFMA backward reads
what the cluster forward wrote), and the refusals made before any HIP call (include/dep_rnn.h)."""
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


def bigru(_lib, H, run, B=4, T=3, Lyr=2, p=0.0, pool=0, impl=6, cell=None, dirs=2):
    return _lib.RnnDesc(_lib.CELL_GRU if cell is None else cell, B, T, 8, H, Lyr, dirs, run, p, 0, pool, impl)


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


def test_the_binding_and_the_header_name_the_value(lib):
    _lib, _ = lib
    assert _lib.IMPL_CLUSTER_BIGRU == 6
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    assert '6 the per-layer cluster forward of a bidirectional GRU' in header


@pytest.mark.parametrize('H', HS)
def test_impl6_exists_for_the_bidirectional_gru_with_an_exchange_buffer(lib, H):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        for B, T, Lyr in ((4, 3, 2), (517, 2, 1), (5, 1, 3), (3, 2, 8)):
            d = bigru(_lib, H, run, B, T, Lyr, p=0.5 if run else 0.0)
            assert so.dep_rnn_reserve_bytes(C.byref(d)) > 0 and so.dep_rnn_workspace_bytes(C.byref(d)) > 0, (H, run, B)
            assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) != NONE, (H, run, B)
            if H <= 256:      # the same descriptor on impl = 0 keeps none (tests/test_bigru_gpu.py pins the plan that follows from it)
                d0 = bigru(_lib, H, run, B, T, Lyr, p=d.dropout_p, impl=0)
                assert so.dep_rnn_workspace_bytes(C.byref(d0)) > 0
                assert so.dep_rnn_workspace_xbuf_offset(C.byref(d0)) == NONE
                assert so.dep_rnn_workspace_bytes(C.byref(d)) > so.dep_rnn_workspace_bytes(C.byref(d0))
    assert so.dep_rnn_workspace_bytes(C.byref(bigru(_lib, H, 0, Lyr=9))) == 0       # L <= MAXL, as for every descriptor


@pytest.mark.parametrize('H', (64, 128, 256))
def test_the_reserve_is_laid_out_as_impl_2s(lib, H):
    """Every layer's y and dropout(y) sit at impl = 2's offsets and the reserve has impl = 2's size: the saved gates and weight images
    between them are where gru_bwd_mfma<.., true> reads them."""
    _lib, so = lib
    for run in (_lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY, _lib.RUN_EVAL):
        for B, T, Lyr, p in ((4, 3, 2, 0.0), (19, 5, 3, 0.5), (517, 2, 1, 0.0)):
            d6 = bigru(_lib, H, run, B, T, Lyr, p=p if run else 0.0, pool=1)
            d2 = bigru(_lib, H, run, B, T, Lyr, p=d6.dropout_p, pool=1, impl=2)
            assert so.dep_rnn_reserve_bytes(C.byref(d6)) == so.dep_rnn_reserve_bytes(C.byref(d2)) > 0
            for l in range(Lyr):
                assert so.dep_rnn_reserve_y_offset(C.byref(d6), l) == so.dep_rnn_reserve_y_offset(C.byref(d2), l), (run, l)
                assert so.dep_rnn_reserve_ydrop_offset(C.byref(d6), l) == so.dep_rnn_reserve_ydrop_offset(C.byref(d2), l), (run, l)
            if run == _lib.RUN_TRAIN:
                assert so.dep_rnn_reserve_y_offset(C.byref(d6), Lyr - 1) != NONE


BAD = [('gru', 64, 1), ('gru', 256, 1), ('lstm', 128, 2), ('lstm', 128, 1), ('gru', 16, 2), ('gru', 96, 2), ('gru', 192, 2), ('gru', 1024, 2)]


@pytest.mark.parametrize('cell,H,dirs', BAD)
def test_every_other_impl6_descriptor_is_bad_with_the_rule(lib, cell, H, dirs):
    _lib, so = lib
    ck = _lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN):
        d = bigru(_lib, H, run, cell=ck, dirs=dirs)
        for query in (so.dep_rnn_reserve_bytes, so.dep_rnn_workspace_bytes):
            assert query(C.byref(d)) == 0
            msg = so.dep_last_error().decode()
            assert 'impl = 6' in msg and 'bidirectional GRU' in msg and '{64, 128, 256, 512}' in msg, msg
        assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) == NONE
        assert so.dep_rnn_reserve_y_offset(C.byref(d), 0) == NONE
        calls = [('dep_rnn_forward', lambda: so.dep_rnn_forward(C.byref(d), None, None, None, None, None, None, 0, None, 0, None)),
                 ('dep_rnn_backward', lambda: so.dep_rnn_backward(C.byref(d), None, None, None, None, None, None, None, None, 0, None, 0, None)),
                 ('dep_rnn_forward', lambda: fwd(so, d, _lib.RnnState(FAKE, None, None))),
                 ('dep_rnn_forward', lambda: fwd(so, d, None, lengths=FAKE)),
                 ('dep_rnn_backward', lambda: bwd(so, d, None, lengths=FAKE))]
        for who, call in calls:
            assert call() == ERR_ARG
            msg = so.dep_last_error().decode()
            assert who in msg and 'impl = 6' in msg and f'H = {H}' in msg and f'dirs = {dirs}' in msg, msg
    with pytest.raises(_lib.DepError, match='impl = 6'):
        _lib.Rnn(ck, 4, 3, 8, H, 2, dirs, False, 0.0, 0, 'cpu', impl=6)


def test_the_messages_of_the_other_bigru_refusals_stay(lib):
    _lib, so = lib
    for impl, H in ((1, 64), (3, 64), (0, 80), (2, 512)):
        d = bigru(_lib, H, _lib.RUN_EVAL, impl=impl)
        assert so.dep_rnn_reserve_bytes(C.byref(d)) == 0
        msg = so.dep_last_error().decode()
        assert msg.startswith('dep_rnn_reserve_bytes: a bidirectional GRU (dirs = 2) runs the tile-MFMA sweeps only: impl must be 0 or 2') and \
            msg.endswith(f'got H = {H}, impl = {impl}'), msg


@pytest.mark.parametrize('H', HS)
def test_hx_passes_the_state_rule_in_every_run_mode(lib, H):
    """The call gets as far as the plain call's own argument checks (x, weights, reserve and workspace are NULL)."""
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        d = bigru(_lib, H, run, p=0.5 if run else 0.0)
        for lengths in (None, FAKE):
            for st in (_lib.RnnState(FAKE, None, None), _lib.RnnState(None, None, None), None):
                assert fwd(so, d, st, lengths) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert 'bad argument: x && weights' in msg and 'impl = 6' not in msg and 'cluster exchange buffer' not in msg, msg
    # hx / dhx in a backward go to the tile-MFMA backward: the state rule lets them through where that backward exists
    if H <= 256:
        d = bigru(_lib, H, _lib.RUN_TRAIN)
        for lengths in (None, FAKE):
            for member in ('hx', 'dhx'):
                sg = _lib.RnnStateGrad(None, None, None, None, None)
                setattr(sg, member, FAKE)
                assert bwd(so, d, sg, lengths) == ERR_ARG
                assert 'bad argument: x && weights' in so.dep_last_error().decode()


@pytest.mark.parametrize('H', HS)
def test_the_cell_state_stays_the_lstms(lib, H):
    _lib, so = lib
    d = bigru(_lib, H, _lib.RUN_EVAL)
    for member in ('cx', 'c_n'):
        st = _lib.RnnState(None, None, None)
        setattr(st, member, FAKE)
        for lengths in (None, FAKE):
            assert fwd(so, d, st, lengths) == ERR_ARG and "LSTM's cell state" in so.dep_last_error().decode()
    if H <= 256:
        d = bigru(_lib, H, _lib.RUN_TRAIN)
        for member in ('cx', 'dc_n', 'dcx'):
            sg = _lib.RnnStateGrad(None, None, None, None, None)
            setattr(sg, member, FAKE)
            assert bwd(so, d, sg) == ERR_ARG and "LSTM's cell state" in so.dep_last_error().decode()


def test_h512_has_the_forward_only(lib):
    """The backward of impl = 6 is the tile-MFMA BiGRU backward, which tiles H up to 256."""
    _lib, so = lib
    d = bigru(_lib, 512, _lib.RUN_TRAIN)
    assert so.dep_rnn_reserve_bytes(C.byref(d)) > 0
    for call in (lambda: so.dep_rnn_backward(C.byref(d), None, None, None, None, None, None, None, None, 0, None, 0, None),
                 lambda: bwd(so, d, _lib.RnnStateGrad(FAKE, None, None, None, None)), lambda: bwd(so, d, None, lengths=FAKE)):
        assert call() == ERR_ARG
        msg = so.dep_last_error().decode()
        assert 'dep_rnn_backward' in msg and 'impl = 6' in msg and 'H = 512' in msg and 'forward only' in msg, msg


def test_a_ragged_call_stays_limited_to_the_parity_modes(lib):
    _lib, so = lib
    d = bigru(_lib, 128, _lib.RUN_TRAIN)
    try:
        for m in (2, 3):
            _lib.set_gemm_mode(m, 0)
            assert fwd(so, d, None, lengths=FAKE) == ERR_ARG
            msg = so.dep_last_error().decode()
            assert 'GEMM modes 0 and 1 only' in msg and f'current mode is {m}' in msg, msg
            assert bwd(so, d, None, lengths=FAKE) == ERR_ARG
            assert 'GEMM modes 0 and 1 only' in so.dep_last_error().decode()
    finally:
        _lib.set_gemm_mode(1, 1 << 28)
