"""What tests/test_clip_cpu.py and tests/test_accum_cpu.py share: the built library for the argument refusals, and a stand-in of the
owner modules plus a recording monkeypatch of nn.L for the optimizer's host logic (no GPU, nothing is launched)."""
import ctypes as C

import pytest
import torch

ERR_ARG = -1
_P = C.c_void_p


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from icassp2022_depression_amd import _lib
    return _lib.load()


def _arrs(ptrs, counts):
    return (_P * len(ptrs))(*ptrs), (C.c_long * len(counts))(*counts)


class _Owner:
    def __init__(self, n, n_live=None):
        self._flat = torch.zeros(n)
        self._flat_grad = torch.zeros(n)
        self._grad_ready = True
        self._n_live = n if n_live is None else n_live


def _params(nn, owner, sizes, dead=()):
    out, off = [], 0
    for i, n in enumerate(sizes):
        p = nn.Parameter(f'p{i}', (n,), owner)
        p.offset = off
        p.live = i not in dead
        p._grad = owner._flat_grad[off:off + n]
        out.append(p)
        off += (n + 3) // 4 * 4
    return out


def name_buffers(names, **owners):
    """names[storage] = 'aP' / 'aG' for name_buffers(names, a=owner): the parameter and the gradient buffer of each owner."""
    for k, o in owners.items():
        names[o._flat.untyped_storage().data_ptr()] = k + 'P'
        names[o._flat_grad.untyped_storage().data_ptr()] = k + 'G'


def record_binding(monkeypatch, adam_logs_p):
    """(nn, log, names): nn.L's optimizer entry points append ('adam' | 'sqnorm' | 'clipped' | 'accum' | 'scale', spans..., the other
    arguments) to log.  A span is (buffer name, start, end) of a tensor; the name is looked up in `names` when the span is COMPARED
    (the accumulators get theirs only after the optimizer made them).  adam_logs_p: the 'adam' entries carry span(p) before span(g)."""
    from icassp2022_depression_amd import nn
    log, names = [], {}

    class span(tuple):
        def __new__(cls, t):
            return super().__new__(cls, (t.untyped_storage().data_ptr(), t.storage_offset(), t.storage_offset() + t.numel()))

        def __eq__(self, other):
            return (names.get(self[0]),) + tuple(self[1:]) == tuple(other)

        def __ne__(self, other):
            return not self == other

        __hash__ = tuple.__hash__

    monkeypatch.setattr(nn.L, 'grad_norm_slots', lambda: 256)
    monkeypatch.setattr(nn.L, 'adam_step', lambda p, g, m, v, *a: log.append(('adam',) + ((span(p),) if adam_logs_p else ()) + (span(g),) + a))
    monkeypatch.setattr(nn.L, 'grad_sqnorm', lambda ranges, partials: log.append(('sqnorm', [span(t) for t in ranges], partials)))
    monkeypatch.setattr(nn.L, 'adam_step_clipped', lambda p, g, m, v, *a: log.append(('clipped', span(p), span(g)) + a))
    monkeypatch.setattr(nn.L, 'grad_clip_scale', lambda *a: log.append(('scale',) + a))
    monkeypatch.setattr(nn.L, 'grad_accumulate', lambda acc, g, scale=1.0, first=False, partials=None:
                        log.append(('accum', [span(t) for t in acc], [span(t) for t in g], scale, first, partials)))
    return nn, log, names
