"""CPU-side checks of the boundary: the C-ABI library builds for gfx950, loads, and exports every symbol
include/dep_rnn.h declares; the ctypes binding covers them all; the product path fails loudly without a GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as g
    g.build()
    return os.path.join(ROOT, 'icassp2022-depression_amd', 'libdep_rnn.so')


def header_symbols():
    src = open(os.path.join(ROOT, 'include', 'dep_rnn.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(dep_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_header_symbol(built):
    out = subprocess.run(['nm', '-D', '--defined-only', built], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (dep_\w+)', out))
    syms = header_symbols()
    assert len(syms) >= 30
    missing = [s for s in syms if s not in exported]
    assert not missing, missing


def test_binding_covers_header(built):
    from icassp2022_depression_amd import _lib
    lib = _lib.load()
    assert lib.dep_arch() == b'gfx950'
    assert sorted(_lib.EXPORTS) == header_symbols()


def test_instance_tables_are_enumerated_without_a_gpu(built):
    """dep_instance_table_read: every row of the cluster families' instance tables under the text the launch-instance log records
    (tests/test_zz_instance_tables_gpu.py holds the list against what the oracle-comparing tests launched)."""
    from icassp2022_depression_amd import _lib
    rows = _lib.instance_table_read()
    assert rows
    assert len(rows) == len(set(rows))
    assert '(gru2_bwd_fused<true, false, true, true>)' in rows        # the name tests/test_step_coverage_gpu.py asserts on
    assert any('gru2_bwd_fused<true, false, true, true>' in r for r in rows)
    # every family is there, switch-selected rows included, and a second read gives the same list
    for name in ('gru_fwd_cluster_r1<2, true>', 'gru_bwd_cluster_r1<8, true, 0>', 'gru_fwd_cluster16<true>', 'lstm_fwd_cluster<true, true, true>',
                 'lstm_bwd_cluster<true, true>', 'gru2_fwd_fused<true, true, false>', 'gru2_bwd_fused<false, false, true, true, true>'):
        assert '(%s)' % name in rows, name
    assert all(r.startswith('(') and r.endswith('>)') for r in rows), rows
    assert _lib.instance_table_read() == rows
    lib = _lib.load()                                                  # the return convention of dep_instance_log_read: bytes needed, truncation
    need = lib.dep_instance_table_read(None, 0)
    assert need == len('\n'.join(rows)) + 2
    import ctypes as C
    buf = C.create_string_buffer(8)
    assert lib.dep_instance_table_read(buf, 8) == need and buf.value == ('\n'.join(rows))[:7].encode()


def test_workspace_queries_run_on_cpu(built):
    import ctypes as C
    from icassp2022_depression_amd import _lib
    lib = _lib.load()
    d = _lib.RnnDesc(_lib.CELL_GRU, 512, 300, 256, 256, 2, 1, 1, 0.5, 0, _lib.POOL_MEAN, 0)
    rb, wb = lib.dep_rnn_reserve_bytes(C.byref(d)), lib.dep_rnn_workspace_bytes(C.byref(d))
    assert rb > 6 * 512 * 300 * 256 * 4 and wb > 512 * 300 * 768 * 4
    bad = _lib.RnnDesc(_lib.CELL_GRU, 4, 4, 4, 4, 2, 2, 0, 0.0, 0, 0, 0)       # bidirectional GRU: not in the path
    assert lib.dep_rnn_reserve_bytes(C.byref(bad)) == 0
    assert lib.dep_gemm_workspace_bytes(1, 0, 768, 256, 153600) > 0              # split-K engaged for dW
    assert lib.dep_gemm_workspace_bytes(0, 1, 153600, 768, 256) == 0


def test_product_path_fails_loudly_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from icassp2022_depression_amd import _lib, audio_gru_whole
    with pytest.raises(_lib.DepError):
        audio_gru_whole.AudioBiLSTM(audio_gru_whole.config)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, 'icassp2022-depression_amd')
    for f in os.listdir(pkg):
        if f.endswith('.py'):
            src = open(os.path.join(pkg, f)).read()
            assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f
