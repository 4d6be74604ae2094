"""impl = 7, "the per-layer cluster sweeps of a bidirectional GRU, forward and backward", the parts that need no GPU: which
descriptors exist, that the reserve is impl = 6's byte for byte, the refusals made before any HIP call, and that impl = 6 kept every
size it had (include/dep_rnn.h).

tests/golden/bigru_cluster_layout_parent.json is data only: dep_rnn_reserve_bytes, dep_rnn_workspace_bytes,
dep_rnn_workspace_xbuf_offset and every dep_rnn_reserve_y_offset of a fixed list of impl = 6 descriptors, read from a build of the
commit in front of impl = 7 with the size queries of the binding (a loop over the descriptors below, json.dump of the answers)."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = C.c_size_t(-1).value
FAKE = 0x1000           # a non-NULL pointer: the refusals under test come before anything reads it
ERR_ARG = -1
HS = (64, 128, 256, 512)
SHAPES = ((4, 3, 2), (517, 2, 1), (5, 1, 3), (3, 2, 8))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib
    return _lib, _lib.load()


def bigru(_lib, H, run, B=4, T=3, Lyr=2, p=0.0, pool=0, impl=7, cell=None, dirs=2, F=8):
    return _lib.RnnDesc(_lib.CELL_GRU if cell is None else cell, B, T, F, H, Lyr, dirs, run, p, 0, pool, impl)


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
    assert _lib.IMPL_CLUSTER_BIGRU_TRAIN == 7
    header = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    assert '7 the per-layer cluster sweeps of a bidirectional GRU, forward and backward' in header


@pytest.mark.parametrize('H', HS)
def test_impl7_exists_for_the_bidirectional_gru_with_an_exchange_buffer(lib, H):
    """Fails on the commit in front of impl = 7: the descriptor is a bad one there."""
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        for B, T, Lyr in SHAPES:
            d = bigru(_lib, H, run, B, T, Lyr, p=0.5 if run else 0.0)
            assert so.dep_rnn_reserve_bytes(C.byref(d)) > 0 and so.dep_rnn_workspace_bytes(C.byref(d)) > 0, (H, run, B)
            assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) != NONE, (H, run, B)
    assert so.dep_rnn_workspace_bytes(C.byref(bigru(_lib, H, 0, Lyr=9))) == 0       # L <= MAXL, as for every descriptor


@pytest.mark.parametrize('H', HS)
def test_the_reserve_is_impl_6s(lib, H):
    """Same size, same y / dropout(y) offsets: the forward is impl = 6's, and the backward reads the arrays the tile BiGRU backward
    reads.  The workspace may be larger (the backward's payload), never smaller."""
    _lib, so = lib
    for run in (_lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY, _lib.RUN_EVAL):
        for B, T, Lyr, p in ((4, 3, 2, 0.0), (19, 5, 3, 0.5), (517, 2, 1, 0.0), (3, 2, 8, 0.5)):
            d7 = bigru(_lib, H, run, B, T, Lyr, p=p if run else 0.0, pool=1)
            d6 = bigru(_lib, H, run, B, T, Lyr, p=d7.dropout_p, pool=1, impl=6)
            assert so.dep_rnn_reserve_bytes(C.byref(d7)) == so.dep_rnn_reserve_bytes(C.byref(d6)) > 0
            for l in range(Lyr):
                assert so.dep_rnn_reserve_y_offset(C.byref(d7), l) == so.dep_rnn_reserve_y_offset(C.byref(d6), l), (run, l)
                assert so.dep_rnn_reserve_ydrop_offset(C.byref(d7), l) == so.dep_rnn_reserve_ydrop_offset(C.byref(d6), l), (run, l)
            assert so.dep_rnn_workspace_bytes(C.byref(d7)) >= so.dep_rnn_workspace_bytes(C.byref(d6))
            assert so.dep_rnn_workspace_xbuf_offset(C.byref(d7)) != NONE


BAD = [('gru', 64, 1), ('gru', 256, 1), ('gru', 512, 1), ('lstm', 128, 2), ('lstm', 128, 1), ('gru', 16, 2), ('gru', 96, 2), ('gru', 192, 2), ('gru', 1024, 2)]


@pytest.mark.parametrize('cell,H,dirs', BAD)
def test_every_other_impl7_descriptor_is_bad_with_the_rule(lib, cell, H, dirs):
    _lib, so = lib
    ck = _lib.CELL_GRU if cell == 'gru' else _lib.CELL_LSTM
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN):
        d = bigru(_lib, H, run, cell=ck, dirs=dirs)
        for query in (so.dep_rnn_reserve_bytes, so.dep_rnn_workspace_bytes):
            assert query(C.byref(d)) == 0
            msg = so.dep_last_error().decode()
            assert 'impl = 7' in msg and 'bidirectional GRU' in msg and '{64, 128, 256, 512}' in msg, msg
        assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) == NONE
        assert so.dep_rnn_reserve_y_offset(C.byref(d), 0) == NONE
        calls = [('dep_rnn_forward', lambda: so.dep_rnn_forward(C.byref(d), None, None, None, None, None, None, 0, None, 0, None)),
                 ('dep_rnn_backward', lambda: so.dep_rnn_backward(C.byref(d), None, None, None, None, None, None, None, None, 0, None, 0, None)),
                 ('dep_rnn_forward', lambda: fwd(so, d, _lib.RnnState(FAKE, None, None))),
                 ('dep_rnn_forward', lambda: fwd(so, d, None, lengths=FAKE)),
                 ('dep_rnn_backward', lambda: bwd(so, d, _lib.RnnStateGrad(FAKE, None, None, None, None))),
                 ('dep_rnn_backward', lambda: bwd(so, d, None, lengths=FAKE))]
        for who, call in calls:
            assert call() == ERR_ARG
            msg = so.dep_last_error().decode()
            assert who in msg and 'impl = 7' in msg and f'H = {H}' in msg and f'dirs = {dirs}' in msg, msg
    with pytest.raises(_lib.DepError, match='impl = 7'):
        _lib.Rnn(ck, 4, 3, 8, H, 2, dirs, False, 0.0, 0, 'cpu', impl=7)


@pytest.mark.parametrize('H', HS)
def test_hx_and_dhx_pass_the_state_rule_at_every_h(lib, H):
    """The call gets as far as the plain call's own argument checks (x, weights, reserve and workspace are NULL): forward in every run
    mode, backward at all four H -- H = 512 included, which impl = 6 refuses."""
    _lib, so = lib
    for run in (_lib.RUN_EVAL, _lib.RUN_TRAIN, _lib.RUN_DROPOUT_ONLY):
        d = bigru(_lib, H, run, p=0.5 if run else 0.0)
        for lengths in (None, FAKE):
            for st in (_lib.RnnState(FAKE, None, None), None):
                assert fwd(so, d, st, lengths) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert 'bad argument: x && weights' in msg and 'impl = 7' not in msg, msg
    d = bigru(_lib, H, _lib.RUN_TRAIN)
    for lengths in (None, FAKE):
        for members in (('hx',), ('dhx',), ('hx', 'dhx'), ()):
            sg = _lib.RnnStateGrad(None, None, None, None, None)
            for m in members:
                setattr(sg, m, FAKE)
            assert bwd(so, d, sg, lengths) == ERR_ARG
            msg = so.dep_last_error().decode()
            assert 'bad argument: x && weights' in msg and 'forward only' not in msg, msg
    assert so.dep_rnn_backward(C.byref(d), None, None, None, None, None, None, None, None, 0, None, 0, None) == ERR_ARG
    assert 'bad argument: x && weights' in so.dep_last_error().decode()


@pytest.mark.parametrize('H', HS)
def test_the_cell_state_is_refused_with_the_rule(lib, H):
    _lib, so = lib
    d = bigru(_lib, H, _lib.RUN_TRAIN)
    for member in ('cx', 'c_n'):
        st = _lib.RnnState(None, None, None)
        setattr(st, member, FAKE)
        for lengths in (None, FAKE):
            assert fwd(so, d, st, lengths) == ERR_ARG
            msg = so.dep_last_error().decode()
            assert 'impl = 7' in msg and "LSTM's cell state" in msg, msg
    for member in ('cx', 'dc_n', 'dcx'):
        sg = _lib.RnnStateGrad(None, None, None, None, None)
        setattr(sg, member, FAKE)
        for lengths in (None, FAKE):
            assert bwd(so, d, sg, lengths) == ERR_ARG
            msg = so.dep_last_error().decode()
            assert 'impl = 7' in msg and "LSTM's cell state" in msg, msg


def test_the_single_product_modes(lib):
    """A ragged call runs in modes 0 and 1 only, as on every plan; a dense backward runs in mode 2 (the split instance, single-product
    contractions behind it) and is refused in mode 3, whose contractions read a PK image the bidirectional sweep does not write."""
    _lib, so = lib
    try:
        for H in HS:
            d = bigru(_lib, H, _lib.RUN_TRAIN)
            for m in (2, 3):
                _lib.set_gemm_mode(m, 0)
                assert fwd(so, d, None, lengths=FAKE) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert 'GEMM modes 0 and 1 only' in msg and f'current mode is {m}' in msg, msg
                assert bwd(so, d, None, lengths=FAKE) == ERR_ARG
                msg = so.dep_last_error().decode()
                assert ('GEMM modes 0 and 1 only' in msg) if m == 2 else ('impl = 7' in msg and 'mode 3' in msg), msg
                assert fwd(so, d, None) == ERR_ARG and 'bad argument: x && weights' in so.dep_last_error().decode()      # a dense forward runs
            _lib.set_gemm_mode(2, 0)
            assert bwd(so, d, None) == ERR_ARG and 'bad argument: x && weights' in so.dep_last_error().decode()
            _lib.set_gemm_mode(3, 0)
            for call in (lambda: bwd(so, d, None), lambda: bwd(so, d, _lib.RnnStateGrad(FAKE, None, None, None, None)),
                         lambda: so.dep_rnn_backward(C.byref(d), None, None, None, None, None, None, None, None, 0, None, 0, None)):
                assert call() == ERR_ARG
                msg = so.dep_last_error().decode()
                assert 'dep_rnn_backward' in msg and 'impl = 7' in msg and 'mode 3' in msg, msg
    finally:
        _lib.set_gemm_mode(1, 1 << 28)


def test_impl6_keeps_every_size_it_had(lib):
    _lib, so = lib
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bigru_cluster_layout_parent.json')))
    assert gold['impl'] == 6 and len(gold['rows']) >= 80
    for r in gold['rows']:
        d = bigru(_lib, r['H'], r['run'], r['B'], r['T'], r['L'], p=r['p'], pool=r['pool'], impl=6, F=r['F'])
        assert so.dep_rnn_reserve_bytes(C.byref(d)) == r['reserve_bytes'], r
        assert so.dep_rnn_workspace_bytes(C.byref(d)) == r['workspace_bytes'], r
        assert so.dep_rnn_workspace_xbuf_offset(C.byref(d)) == r['xbuf_offset'], r
        assert [so.dep_rnn_reserve_y_offset(C.byref(d), l) for l in range(r['L'])] == r['y_offsets'], r


def test_impl6_still_has_the_forward_only_at_h512(lib):
    _lib, so = lib
    d = bigru(_lib, 512, _lib.RUN_TRAIN, impl=6)
    assert bwd(so, d, None) == ERR_ARG
    msg = so.dep_last_error().decode()
    assert 'impl = 6' in msg and 'forward only' in msg, msg


def test_the_instance_table_lists_the_sixteen_rows(lib):
    _lib, _ = lib
    rows = [r.strip('()') for r in _lib.instance_table_read()]      # (a row is the kernel expression as the table wrote it, in parentheses)
    rows = [r for r in rows if r.startswith('gru_bwd_cluster_r1<') and r.endswith(', true>') and r.count(',') == 7]
    want = set()
    for ntw, kb in ((1, 4), (2, 4), (4, 4), (8, 0)):
        for split in ('false', 'true'):
            for rag in ('false', 'true'):
                ag = 'true' if (ntw == 4 and split == 'true') else 'false'
                want.add(f'gru_bwd_cluster_r1<{ntw}, {split}, {kb}, false, false, {ag}, {rag}, true>')
    assert set(rows) == want and len(rows) == 16, sorted(rows)
