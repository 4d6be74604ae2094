"""impl = 4, "the per-layer cluster sweeps", the parts that need no GPU: which descriptors exist, their layout queries, and the
refusals the state calls make on them before any HIP call (include/dep_rnn.h).  The layout queries of impl 0 / 3 at the same shapes
are held against tests/golden/rnn_layout_before_impl4.json, recorded from the library before impl = 4 existed."""
import ctypes as C
import json
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


def gru4(_lib, H, run, B=4, T=3, Lyr=2, p=0.0, pool=0):
    return _lib.RnnDesc(_lib.CELL_GRU, B, T, 8, H, Lyr, 1, run, p, 0, pool, _lib.IMPL_CLUSTER_PER_LAYER)


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
    assert _lib.IMPL_CLUSTER_PER_LAYER == 4
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    assert '4 the per-layer cluster sweeps' in header


@pytest.mark.parametrize('H', HS)
def test_impl4_exists_for_the_unidirectional_gru_with_a_cluster_layout(lib, H):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        for B, T, Lyr in ((4, 3, 2), (517, 2, 1), (5, 1, 3)):
            d = gru4(_lib, H, run, B, T, Lyr, p=0.5 if run else 0.0)
            assert so.dep_rnn_reserve_bytes(C.byref(d)) > 0 and so.dep_rnn_workspace_bytes(C.byref(d)) > 0, (H, run, B)
            assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) != NONE, (H, run, B)
            # the cluster layout without the fused two-layer extras, plus the B x H staging area of the T = 1 aliasing rule
            d3 = _lib.RnnDesc(_lib.CELL_GRU, B, T, 8, H, Lyr, 1, run, d.dropout_p, 0, 0, 3)
            assert so.dep_rnn_reserve_bytes(C.byref(d)) == so.dep_rnn_reserve_bytes(C.byref(d3))
            assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) == so.dep_rnn_workspace_xbuf_offset(C.byref(d3))
            if not (H == 256 and Lyr == 2):                # (no fused two-layer part on the impl 3 side either)
                assert so.dep_rnn_workspace_bytes(C.byref(d)) == so.dep_rnn_workspace_bytes(C.byref(d3)) + (B * H + 63) // 64 * 64 * 4
            else:
                assert so.dep_rnn_workspace_bytes(C.byref(d)) < so.dep_rnn_workspace_bytes(C.byref(d3))


BAD = [('lstm', 128, 2), ('lstm', 128, 1), ('lstm', 256, 1), ('gru', 256, 2), ('gru', 64, 2), ('gru', 16, 1), ('gru', 48, 1), ('gru', 96, 1)]


@pytest.mark.parametrize('cell,H,dirs', BAD)
def test_every_other_impl4_descriptor_is_bad_with_the_rule(lib, cell, H, dirs):
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN):
        d = _lib.RnnDesc(_lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM, 4, 3, 8, H, 2, dirs, run, 0.0, 0, 0, 4)
        for query in (so.dep_rnn_reserve_bytes, so.dep_rnn_workspace_bytes):
            assert query(C.byref(d)) == 0
            msg = so.dep_last_error().decode()
            assert 'impl = 4' in msg and 'unidirectional GRU' in msg and '{64, 128, 256, 512}' in msg, msg
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
            assert who in msg and 'impl = 4' in msg and f'H = {H}' in msg and f'dirs = {dirs}' in msg, msg
    with pytest.raises(_lib.DepError, match='impl = 4'):
        _lib.Rnn(_lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM, 4, 3, 8, H, 2, dirs, False, 0.0, 0, 'cpu', impl=4)


@pytest.mark.parametrize('H', HS)
def test_hx_in_train_mode_and_any_state_in_a_backward_are_refused_with_the_rule(lib, H):
    _lib, so = lib
    d = gru4(_lib, H, _lib.RUN_TRAIN)
    for lengths, who in ((None, 'dep_rnn_forward_state'), (FAKE, 'dep_rnn_forward_state_varlen')):
        assert fwd(so, d, _lib.RnnState(FAKE, None, None), lengths) == ERR_ARG
        msg = so.dep_last_error().decode()
        assert who in msg and 'impl = 4' in msg and 'DEP_RUN_EVAL' in msg and 'DEP_RUN_DROPOUT_ONLY' in msg and f'H = {H}' in msg, msg
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        d = gru4(_lib, H, run)
        for lengths, who in ((None, 'dep_rnn_backward_state'), (FAKE, 'dep_rnn_backward_state_varlen')):
            for member in ('hx', 'dhx'):
                sg = _lib.RnnStateGrad(None, None, None, None, None)
                setattr(sg, member, FAKE)
                assert bwd(so, d, sg, lengths) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert who in msg and 'impl = 4' in msg and 'cluster backward takes no state' in msg, (member, msg)
    # the cell state stays the LSTM's
    d = gru4(_lib, H, _lib.RUN_EVAL)
    for member in ('cx', 'c_n'):
        st = _lib.RnnState(None, None, None)
        setattr(st, member, FAKE)
        assert fwd(so, d, st) == ERR_ARG and "LSTM's cell state" in so.dep_last_error().decode()
    for member in ('cx', 'dc_n', 'dcx'):
        sg = _lib.RnnStateGrad(None, None, None, None, None)
        setattr(sg, member, FAKE)
        assert bwd(so, d, sg) == ERR_ARG and "LSTM's cell state" in so.dep_last_error().decode()


@pytest.mark.parametrize('H', HS)
def test_hx_in_the_modes_no_backward_follows_passes_the_state_rule(lib, H):
    """EVAL / DROPOUT_ONLY: the call gets as far as the plain call's own argument checks (x, weights, reserve and workspace are NULL)."""
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_DROPOUT_ONLY):
        d = gru4(_lib, H, run, p=0.5 if run else 0.0)
        for lengths in (None, FAKE):
            for st in (_lib.RnnState(FAKE, None, None), _lib.RnnState(None, None, None), None):
                assert fwd(so, d, st, lengths) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert 'bad argument: x && weights' in msg and 'impl = 4' not in msg and 'cluster exchange buffer' not in msg, msg


def test_layout_of_impl_0_and_3_is_the_parents(lib):
    _lib, so = lib
    cases = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'rnn_layout_before_impl4.json')))['cases']
    assert len(cases) == 32 and {c['desc'][4] for c in cases} == set(HS) and {c['desc'][10] for c in cases} == {0, 3}
    fix = lambda v: -1 if v == NONE else int(v)
    for c in cases:
        cell, B, T, F, H, L, dirs, run, p, pool, impl = c['desc']
        d = _lib.RnnDesc(cell, B, T, F, H, L, dirs, run, p, 0, pool, impl)
        assert so.dep_rnn_reserve_bytes(C.byref(d)) == c['reserve_bytes'], c['desc']
        assert so.dep_rnn_workspace_bytes(C.byref(d)) == c['workspace_bytes'], c['desc']
        assert [fix(so.dep_rnn_reserve_y_offset(C.byref(d), l)) for l in range(L)] == c['y_offset'], c['desc']
        assert [fix(so.dep_rnn_reserve_ydrop_offset(C.byref(d), l)) for l in range(L)] == c['ydrop_offset'], c['desc']
        assert fix(so.dep_rnn_workspace_xbuf_offset(C.byref(d))) == c['xbuf_offset'], c['desc']


def test_the_refusal_on_impl_0_and_3_points_to_impl_4(lib):
    _lib, so = lib
    d = _lib.RnnDesc(_lib.CELL_GRU, 4, 3, 8, 256, 2, 1, _lib.RUN_EVAL, 0.0, 0, 0, 3)
    assert fwd(so, d, _lib.RnnState(FAKE, None, None)) == ERR_ARG
    msg = so.dep_last_error().decode()
    assert 'cluster exchange buffer' in msg and 'impl = 3' in msg and 'impl = 4' in msg, msg
