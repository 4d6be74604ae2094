"""GPU parity of the fused MLP head (csrc/head.hip) at the batch, width and column edges of its three kernels, every template instance included.

The reference is tests/head_ref.py: plain float64, masks from oracle/ref_numpy.py's own Philox (never a device draw), pinned against stock torch
in tests/test_head_ref_cpu.py -- which also shows that a batch row lost at any boundary of a case moves each gradient by more than 100 bars, and
that float32 summation in the weight pass's own order uses about an eighth of the gradient bar at B = 2049.  The bars are those of
tests/test_kernels_gpu.py::test_fused_mlp_head_against_float64_with_the_same_masks: a0 1e-6 absolute; z1, a1, z2, dz1 2e-6 and dW1, db1, dW2,
db2, dx 5e-6 max-norm relative error; the zero patterns of a1 and dz1 equal to the reference's.  The backward is fed the device's own a0, z1, a1
(the forward's outputs, as in a train step) and the reference's backward is computed from the same three arrays, so each pass is judged alone.

Every buffer is guarded.  a0, z1, a1, z2, dz1, dx are B rows inside an all-NaN allocation with 8 further rows: the rows come back finite, the rest
NaN bit for bit.  x, dz2 and the backward's a0, z1, a1 are followed by 8 NaN rows no clamped load may let in.  The gradients are views into one
flat zeroed buffer laid out as nn.Module._finalize lays parameters out (dW1 | db1 | dW2 | db2, each slot padded to 4 floats, 64 floats behind):
the views start as NaN and come back finite, every pad and tail word is still +0.0 -- a stray store there would corrupt a clipped step's global
gradient norm and no tensor comparison would show it.

  A  every template instance: 8 (Hin, H1) pairs x (p, first), B = 5, C = 2
  B  batch edges 1 .. 2049 at (32, 16, 5): row groups of 4, one row per wave, 16 rows in flight, the second staging iteration (513), two and
     three rounds of the weight pass, the last of one row (1025, 2049); 513 / 1025 / 2049 again at (256, 256, 16) with every lane live
  C  C in {0, 1, 3, 4, 5, 15, 16} at (64, 64), B = 37; C = 0 is forward only and bit-equal to the C = 5 run; refused shapes raise
  D  dx omitted: dz1 and the four gradients bit-equal to the run with dx
  E  operands one float into their allocation: accepted bit-equal (scalar accesses) or refused (16-byte loads) with nothing written
  F  a second run gives the same bits
  G  models._MLPHead and models._mlp_feature: the fused and the composed launches (DEP_HEAD_FUSED) on one input, both against head_ref
  H  the instance logs of A to D hold all thirteen kernel instances

Each case prints its figures before asserting ('head-forms ...', pytest -s).  Worst figures of the last device run (one MI355X):
                 a0     z1       a1       z2       dz1      dW1      db1      dW2      db2      dx
  A  instances   0      2.8e-7   3.2e-7   6.3e-7   1.0e-7   9.9e-8   7.6e-8   1.2e-7   6.8e-8   1.4e-7
  B  batch       0      3.7e-7   3.9e-7   1.7e-7   1.3e-7   2.9e-7   2.6e-7   3.7e-7   4.4e-7   1.9e-7
  C  columns     0      1.0e-7   1.2e-7   1.7e-7   1.2e-7   1.4e-7   1.6e-7   1.5e-7   1.6e-7   1.9e-7
  D  no dx       0      2.2e-7   2.4e-7   2.0e-7   5.8e-8   1.8e-7   9.5e-8   1.9e-7   7.0e-7   1.0e-7
  G  models      0      3.2e-7   3.4e-7   2.7e-7   -        1.8e-7   1.3e-7   2.2e-7   1.9e-7   1.8e-7   (fused, composed, one against the other)
  B = 2049: (32, 16, 5) dW1 1.4e-7 db1 1.7e-7 dW2 2.7e-7 db2 2.9e-7; (256, 256, 16) dW1 2.9e-7 db1 2.5e-7 dW2 3.7e-7 db2 2.8e-7 -- the float32
  walk of the CPU test says 1 - 2e-7.  No comparison needed the a-priori summation bound; the worst gradient figure is a seventh of its bar.
  No guard, pad or tail word was written, no refusal wrote anything, and every bit comparison (C = 0, dx omitted, offsets, second run, Hin = 96) held.
Run on the MI355X box:  python -m pytest tests/test_head_forms_gpu.py -m gpu -q -s
"""
import numpy as np
import pytest

import head_ref as H

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L, models, nn
    DEV = torch.device('cuda:0')

NAN = float('nan')
FWD_OUT = ('a0', 'z1', 'a1', 'z2')
BWD_OUT = ('dz1', 'dW1', 'db1', 'dW2', 'db2', 'dx')
GRADS = ('dW1', 'db1', 'dW2', 'db2')
WORST = {}                                                            # section -> {quantity: worst figure}, printed by the closing test


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)          # (a copy: the cases' arrays are read-only)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


class Rows:
    """`rows` x `width` floats `off` floats into an all-NaN allocation that goes on for GUARD further rows.  data: the rows' values (an input);
    None leaves them NaN (an output)."""

    def __init__(self, rows, width, data=None, off=0):
        self.buf = torch.full((off + (rows + H.GUARD) * width,), NAN, device=DEV)
        self.lo, self.hi = off, off + rows * width
        self.v = self.buf[self.lo:self.hi].view(rows, width)
        if data is not None:
            self.v.copy_(dev(data))
        self.nanbits = int(bits(torch.full((1,), NAN))[0])

    def guards_intact(self):
        b = bits(self.buf)
        return bool((b[:self.lo] == self.nanbits).all()) and bool((b[self.hi:] == self.nanbits).all())

    def untouched(self):
        return bool((bits(self.buf) == self.nanbits).all())


class FlatGrads:
    """dW1 | db1 | dW2 | db2 as views into one flat zeroed buffer, each slot padded to a multiple of 4 floats, 64 zero floats behind the last:
    the layout of nn.Module._finalize.  The views start as NaN; the pads and the tail are +0.0 and must stay so."""

    def __init__(self, Hin, H1, C):
        shapes = dict(dW1=(H1, Hin), db1=(H1,), dW2=(C, H1), db2=(C,))
        off, self.at = 0, {}
        for k in GRADS:
            n = int(np.prod(shapes[k]))
            self.at[k] = (off, n)
            off += (n + 3) // 4 * 4
        self.buf = torch.zeros(off + 64, device=DEV)
        self.pad = torch.ones(off + 64, dtype=torch.bool, device=DEV)
        self.v = {}
        for k, (o, n) in self.at.items():
            self.v[k] = self.buf[o:o + n].view(shapes[k])
            self.v[k].fill_(NAN)
            self.pad[o:o + n] = False
        assert int(self.pad.sum()) == 64 + (-C) % 4

    def pads_zero(self):
        return not bool(bits(self.buf)[self.pad].any())

    def untouched(self):
        return self.pads_zero() and bool(torch.isnan(self.buf[~self.pad]).all())


def weights(d):
    return tuple(None if d[k] is None else dev(d[k]) for k in ('W1', 'b1', 'W2', 'b2'))


def run_forward(c, off=()):
    """The forward of case c into guarded buffers; off: names of the operands that start one float into their allocation.  -> dict of Rows."""
    d = H.inputs(c)
    W1, b1, W2, b2 = weights(d)
    use0 = bool(c.first and c.p > 0)
    o = lambda k: int(k in off)
    r = dict(x=Rows(c.B, c.Hin, d['x'], o('x')), z1=Rows(c.B, c.H1, off=o('z1')), a1=Rows(c.B, c.H1, off=o('a1')))
    r['a0'] = Rows(c.B, c.Hin, off=o('a0')) if use0 else None
    r['z2'] = Rows(c.B, c.C, off=o('z2')) if c.C else None
    L.head_mlp_fwd(r['x'].v, W1, b1, W2, b2, r['a0'].v if use0 else None, r['z1'].v, r['a1'].v, r['z2'].v if c.C else None, c.p, d['seed'],
                   H.SITES, use0)
    torch.cuda.synchronize()
    return r


def run_backward(c, f, want_dx=True, off=()):
    """The backward of case c behind the forward f (its a0 -- x without a first dropout --, z1, a1 as they stand, NaN rows behind them)."""
    d = H.inputs(c)
    W1, b1, W2, b2 = weights(d)
    use0 = bool(c.first and c.p > 0)
    o = lambda k: int(k in off)
    a0 = f['a0'] if use0 else f['x']
    z1 = f['z1'] if 'z1' not in off else Rows(c.B, c.H1, host(f['z1'].v), 1)
    r = dict(dz2=Rows(c.B, c.C, d['dz2'], o('dz2')), dz1=Rows(c.B, c.H1, off=o('dz1')), dx=Rows(c.B, c.Hin, off=o('dx')) if want_dx else None,
             g=FlatGrads(c.Hin, c.H1, c.C), z1=z1)
    g = r['g'].v
    L.head_mlp_bwd(r['dz2'].v, a0.v, z1.v, f['a1'].v, W1, W2, g['dW1'], g['db1'], g['dW2'], g['db2'], r['dx'].v if want_dx else None, r['dz1'].v,
                   c.p, d['seed'], H.SITES, use0)
    torch.cuda.synchronize()
    return r


def outputs(c, f, b=None):
    """name -> device tensor of every output of a forward (and a backward)."""
    out = {k: f[k].v for k in FWD_OUT if f.get(k) is not None}
    if b is not None:
        out['dz1'] = b['dz1'].v
        out.update(b['g'].v)
        if b['dx'] is not None:
            out['dx'] = b['dx'].v
    return out


def figures(c, got, ref):
    """{quantity: (figure, bar)}: a0 absolute, the rest max-norm relative; NaN when the device value is not finite."""
    fig = {}
    for k, g in got.items():
        if not np.isfinite(g).all():
            fig[k] = (NAN, 0.0)
        elif k == 'a0':
            fig[k] = (float(np.abs(g - ref[k]).max()), H.A0_ATOL)
        else:
            fig[k] = (H.relerr(g, ref[k]), H.ACT_RTOL if k in ('z1', 'a1', 'z2', 'dz1') else H.GRAD_RTOL)
    return fig


def judge(tag, c, got, ref):
    """Print the figures of one pass, then hold each to its bar; a reference that is identically zero is held to exactly zero."""
    fig = figures(c, got, ref)
    print('head-forms %s %s: ' % (tag, H.case_id(c)) + ' '.join('%s %.2e' % (k, v[0]) for k, v in fig.items()))
    w = WORST.setdefault(c.sec, {})
    for k, (e, bar) in fig.items():
        w[k] = e if k not in w or e != e or e > w[k] else w[k]
    for k, (e, bar) in fig.items():
        assert e == e, '%s: not finite' % k
        if not ref[k].any():
            assert not got[k].any(), '%s: the reference is identically zero' % k
        assert e < bar, '%s: %.3e' % (k, e)
    for k in ('a1', 'dz1'):
        if k in got:
            assert ((got[k] == 0) == (ref[k] == 0)).all(), '%s: zero pattern' % k


def check_forward(c, f):
    for k in ('x', 'a0', 'z1', 'a1', 'z2'):
        assert f[k] is None or f[k].guards_intact(), '%s: a guard word was written' % k
    judge('fwd', c, {k: host(v) for k, v in outputs(c, f).items()}, H.reference(c))


def check_backward(c, f, b):
    """Guards and pads, then the backward against the float64 backward of the same a0, z1, a1 (the forward's device outputs)."""
    for k in ('dz2', 'dz1', 'dx'):
        assert b[k] is None or b[k].guards_intact(), '%s: a guard word was written' % k
    assert b['g'].pads_zero(), 'a pad or tail word of the flat gradient buffer was written'
    d = H.inputs(c)
    use0 = bool(c.first and c.p > 0)
    a0, z1, a1 = host((f['a0'] if use0 else f['x']).v), host(b['z1'].v), host(f['a1'].v)
    ref = dict(zip(BWD_OUT, H.head_backward(H.f64(d['dz2']), a0, z1, a1, H.f64(d['W1']), H.f64(d['W2']), d['m0'], d['m1'])))
    got = {k: host(v) for k, v in outputs(c, f, b).items() if k in BWD_OUT}
    judge('bwd', c, got, ref)
    # the device-fed reference is the case's own reference within the forward's bars: the sensitivity figures of the CPU test hold for it
    own = H.reference(c)
    for k in GRADS:
        assert H.relerr(ref[k], own[k]) < 10 * H.ACT_RTOL, k


def run_and_check(c, want_dx=True):
    f = run_forward(c)
    check_forward(c, f)
    if not c.C:
        return f, None
    b = run_backward(c, f, want_dx)
    check_backward(c, f, b)
    return f, b


def test_sites_are_the_librarys():
    assert H.SITES == (L.SITE_FC0, L.SITE_FC1)
    for c in H.CASES:
        assert L.load().dep_head_mlp_supported(c.Hin, c.H1, c.C), c


# ----------------------------------------------------------------------------- A, B
@pytest.mark.parametrize('c', H.section('A'), ids=H.case_id)
def test_a_every_template_instance(c):
    run_and_check(c)
    assert {H.fwd_instance(c.Hin), H.rows_instance(c.H1), H.W_INSTANCE} <= L.instance_log_read()


@pytest.mark.parametrize('c', H.section('B'), ids=H.case_id)
def test_b_batch_edges(c):
    run_and_check(c)


# ----------------------------------------------------------------------------- C
@pytest.mark.parametrize('c', H.section('C'), ids=H.case_id)
def test_c_output_column_edges(c):
    run_and_check(c)


def test_c_zero_columns_is_the_five_column_forward_bit_for_bit():
    """C = 0 returns before the second Linear; x, W1, b1 and the masks of section C do not depend on C (tests/test_head_ref_cpu.py)."""
    c0, c5 = (next(c for c in H.section('C') if c.C == C) for C in (0, 5))
    f0, f5 = run_forward(c0), run_forward(c5)
    assert f0['z2'] is None
    for k in ('a0', 'z1', 'a1'):
        assert same_bits(f0[k].v, f5[k].v), k


@pytest.mark.parametrize('Hin,H1,C', H.REFUSED)
def test_c_refused_shapes_raise_at_both_entry_points(Hin, H1, C):
    assert not L.load().dep_head_mlp_supported(Hin, H1, C) and not L.head_mlp_supported(Hin, H1, C)
    B = 5
    z = lambda *s: torch.zeros(*s, device=DEV)
    outs = [Rows(B, Hin), Rows(B, H1), Rows(B, H1), Rows(B, C)]
    with pytest.raises(L.DepError):
        L.head_mlp_fwd(z(B, Hin), z(H1, Hin), z(H1), z(C, H1), z(C), outs[0].v, outs[1].v, outs[2].v, outs[3].v, 0.5, 1, H.SITES, True)
    g = FlatGrads(Hin, H1, C)
    outs += [Rows(B, Hin), Rows(B, H1)]
    with pytest.raises(L.DepError):
        L.head_mlp_bwd(z(B, C), z(B, Hin), z(B, H1), z(B, H1), z(H1, Hin), z(C, H1), g.v['dW1'], g.v['db1'], g.v['dW2'], g.v['db2'], outs[4].v,
                       outs[5].v, 0.5, 1, H.SITES, True)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs) and g.untouched()
    assert not any('head_mlp' in s for s in L.instance_log_read())


# ----------------------------------------------------------------------------- D
@pytest.mark.parametrize('c', H.section('D'), ids=H.case_id)
def test_d_dx_omitted(c):
    f, b = run_and_check(c)
    b2 = run_backward(c, f, want_dx=False)
    check_backward(c, f, b2)
    assert b2['dx'] is None
    for k in ('dz1',) + GRADS:
        assert same_bits(outputs(c, f, b)[k], outputs(c, f, b2)[k]), k


# ----------------------------------------------------------------------------- E
ALIGN = H.Case('E', 5, 32, 16, 5, 0.5, True)


def test_e_scalar_operands_may_start_one_float_in():
    f, b = run_and_check(ALIGN)
    for k in ('x', 'z1', 'a1', 'z2', 'a0'):
        f1 = run_forward(ALIGN, off=(k,))
        assert f1[k].v.data_ptr() % 16 == 4
        check_forward(ALIGN, f1)
        for n in FWD_OUT:
            assert same_bits(f[n].v, f1[n].v), (k, n)
    for k in ('dz2', 'z1', 'dz1', 'dx'):
        b1 = run_backward(ALIGN, f, off=(k,))
        assert b1[k].v.data_ptr() % 16 == 4
        check_backward(ALIGN, f, b1)
        for n in BWD_OUT:
            assert same_bits(outputs(ALIGN, f, b)[n], outputs(ALIGN, f, b1)[n]), (k, n)


def test_e_vector_operands_one_float_in_are_refused_and_nothing_is_written():
    c = ALIGN
    d = H.inputs(c)
    W1, b1, W2, b2 = weights(d)
    W1o = Rows(c.H1, c.Hin, d['W1'], 1).v
    assert W1o.data_ptr() % 16 == 4
    f = run_forward(c)
    outs = [Rows(c.B, c.Hin), Rows(c.B, c.H1), Rows(c.B, c.H1), Rows(c.B, c.C)]
    with pytest.raises(L.DepError):
        L.head_mlp_fwd(f['x'].v, W1o, b1, W2, b2, outs[0].v, outs[1].v, outs[2].v, outs[3].v, c.p, d['seed'], H.SITES, True)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
    a0o, a1o = Rows(c.B, c.Hin, host(f['a0'].v), 1).v, Rows(c.B, c.H1, host(f['a1'].v), 1).v
    dz2 = Rows(c.B, c.C, d['dz2']).v
    for W1x, a0x, a1x in ((W1o, f['a0'].v, f['a1'].v), (W1, a0o, f['a1'].v), (W1, f['a0'].v, a1o)):
        g, dx, dz1 = FlatGrads(c.Hin, c.H1, c.C), Rows(c.B, c.Hin), Rows(c.B, c.H1)
        with pytest.raises(L.DepError):
            L.head_mlp_bwd(dz2, a0x, f['z1'].v, a1x, W1x, W2, g.v['dW1'], g.v['db1'], g.v['dW2'], g.v['db2'], dx.v, dz1.v, c.p, d['seed'],
                           H.SITES, True)
        torch.cuda.synchronize()
        assert g.untouched() and dx.untouched() and dz1.untouched()


# ----------------------------------------------------------------------------- F
@pytest.mark.parametrize('c', [next(c for c in H.section('B') if c.B == 1025 and c.Hin == 32), next(c for c in H.section('C') if c.C == 5)],
                         ids=H.case_id)
def test_f_a_second_run_gives_the_same_bits(c):
    f1 = run_forward(c); b1 = run_backward(c, f1)
    f2 = run_forward(c); b2 = run_backward(c, f2)
    o1, o2 = outputs(c, f1, b1), outputs(c, f2, b2)
    assert set(o1) == set(FWD_OUT + BWD_OUT)
    for k in o1:
        assert same_bits(o1[k], o2[k]), k


# ----------------------------------------------------------------------------- G
class Owner:
    """What models._MLPHead needs of its module: `_params`, name -> nn.Parameter whose .data and ._grad are views into one flat pair of buffers
    laid out as nn.Module._finalize lays them out (every tensor at a multiple of 4 floats, the gradient buffer zeroed)."""

    def __init__(self, values):
        self._params = {k: nn.Parameter(k, v.shape, self) for k, v in values.items() if v is not None}
        off = 0
        for p in self._params.values():
            p.offset = off
            off += (p.numel + 3) // 4 * 4
        self.flat = torch.zeros(off + 64, device=DEV)
        self.flat_grad = torch.zeros(off + 64, device=DEV)
        self.pad = torch.ones(off + 64, dtype=torch.bool, device=DEV)
        for k, p in self._params.items():
            p.data = self.flat[p.offset:p.offset + p.numel].view(p.shape)
            p._grad = self.flat_grad[p.offset:p.offset + p.numel].view(p.shape)
            p.data.copy_(dev(values[k]))
            p._grad.fill_(NAN)
            self.pad[p.offset:p.offset + p.numel] = False


def run_model_head(c, training, fused, monkeypatch):
    """models._MLPHead forward + backward on case c under DEP_HEAD_FUSED = fused -> outputs (device tensors), the test's launch log so far
    (a set: what a run added to it is the difference to the log before)."""
    monkeypatch.setenv('DEP_HEAD_FUSED', '1' if fused else '0')
    d = H.inputs(c)
    own = Owner({'fc.0.weight': d['W1'], 'fc.0.bias': d['b1'], 'fc.2.weight': d['W2'], 'fc.2.bias': d['b2']})
    head = models._MLPHead(own, 'fc.0', 'fc.2', c.p, c.first, H.SITES)
    x = dev(d['x'])
    z2 = head.forward(x, d['seed'], training)
    a0, z1, a1 = head.saved[:3]
    dx = head.backward(dev(d['dz2']))
    torch.cuda.synchronize()
    assert not bool(bits(own.flat_grad)[own.pad].any()), 'a pad word of the flat gradient buffer was written'
    P = own._params
    out = dict(a0=a0, z1=z1, a1=a1, z2=z2, dW1=P['fc.0.weight']._grad, db1=P['fc.0.bias']._grad, dW2=P['fc.2.weight']._grad,
               db2=P['fc.2.bias']._grad, dx=dx)
    return out, L.instance_log_read()


def is_head(s):
    return s.startswith('head_mlp_')


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('Hin,H1,C,first', [(256, 256, 2, True), (64, 64, 1, False)])
def test_g_model_head_fused_and_composed(Hin, H1, C, first, training, monkeypatch):
    c = H.Case('G', 37, Hin, H1, C, 0.5, first)
    ce = c if training else c._replace(p=0.0)                        # eval: no dropout, the same x and weights
    d = H.inputs(c)
    m0, m1 = (d['m0'], d['m1']) if training else (None, None)
    composed, log0 = run_model_head(c, training, False, monkeypatch)  # first, so that its log cannot hold the other run's launches
    fused, log1 = run_model_head(c, training, True, monkeypatch)
    assert not any(is_head(s) for s in log0) and len(log0) >= 4, sorted(log0)
    assert log1 - log0 == {H.fwd_instance(Hin), H.rows_instance(H1), H.W_INSTANCE}, sorted(log1 - log0)       # the three launches and nothing else
    a0, z1, a1, z2 = H.head_forward(H.f64(d['x']), H.f64(d['W1']), H.f64(d['b1']), H.f64(d['W2']), H.f64(d['b2']), m0, m1)
    ref = dict(a0=a0, z1=z1, a1=a1, z2=z2)
    ref.update(zip(BWD_OUT, H.head_backward(H.f64(d['dz2']), a0, z1, a1, H.f64(d['W1']), H.f64(d['W2']), m0, m1)))
    del ref['dz1']
    hf, hc = ({k: host(v) for k, v in o.items()} for o in (fused, composed))
    judge('model fused %s' % ('train' if training else 'eval'), ce, hf, ref)
    judge('model composed %s' % ('train' if training else 'eval'), ce, hc, ref)
    judge('model fused against composed', ce, hf, hc)
    for k in ('a0', 'a1', 'z2', 'dx'):
        assert ((hf[k] == 0) == (hc[k] == 0)).all(), k
    assert (hf['a0'] == hc['a0']).all()                              # x or x times the mask: one rounding either way


def test_g_model_head_at_a_width_the_kernels_refuse(monkeypatch):
    c = H.Case('G', 37, 96, 64, 2, 0.5, True)
    assert not L.load().dep_head_mlp_supported(96, 64, 2)
    o0, log0 = run_model_head(c, True, False, monkeypatch)
    o1, log1 = run_model_head(c, True, True, monkeypatch)
    assert log0 == log1 and not any(is_head(s) for s in log1)
    for k in o0:
        assert same_bits(o0[k], o1[k]), k
    d = H.inputs(c)
    a0, z1, a1, z2 = H.head_forward(H.f64(d['x']), H.f64(d['W1']), H.f64(d['b1']), H.f64(d['W2']), H.f64(d['b2']), d['m0'], d['m1'])
    ref = dict(a0=a0, z1=z1, a1=a1, z2=z2)
    ref.update(zip(BWD_OUT, H.head_backward(H.f64(d['dz2']), a0, z1, a1, H.f64(d['W1']), H.f64(d['W2']), d['m0'], d['m1'])))
    del ref['dz1']
    judge('model composed Hin=96', c, {k: host(v) for k, v in o1.items()}, ref)


@pytest.mark.parametrize('p', [0.5, 0.0])
@pytest.mark.parametrize('Hin,H1', [(256, 256), (96, 64)])
def test_g_mlp_feature_fused_and_composed(Hin, H1, p, monkeypatch):
    c = H.Case('G', 37, Hin, H1, 0, p, True)
    d = H.inputs(c)
    x, W1, b1 = (dev(d[k]) for k in ('x', 'W1', 'b1'))
    res = []
    for fused in (False, True):
        monkeypatch.setenv('DEP_HEAD_FUSED', '1' if fused else '0')
        a1 = models._mlp_feature(x, W1, b1, p, d['seed'], H.SITES)
        torch.cuda.synchronize()
        res.append((a1, L.instance_log_read()))
    (ac, log0), (af, log1) = res
    assert not any(is_head(s) for s in log0) and log0
    ref = dict(a1=H.reference(c)['a1'])
    judge('feature composed', c, dict(a1=host(ac)), ref)
    judge('feature fused', c, dict(a1=host(af)), ref)
    if H.supported(Hin, H1, 0):
        assert log1 - log0 == {H.fwd_instance(Hin)}
        judge('feature fused against composed', c, dict(a1=host(af)), dict(a1=host(ac)))
    else:
        assert log1 == log0 and same_bits(af, ac)


# ----------------------------------------------------------------------------- H
def test_h_sections_a_to_d_launched_every_instance(request):
    rec = request.config._dep_instances
    for sec, w in sorted(WORST.items()):
        print('head-forms worst %s: ' % sec + ' '.join('%s %.2e' % kv for kv in w.items()))
    seen = set()
    for fn, n in (('test_a_every_template_instance', len(H.section('A'))), ('test_b_batch_edges', len(H.section('B'))),
                  ('test_c_output_column_edges', len(H.section('C'))), ('test_d_dx_omitted', len(H.section('D')))):
        mine = [k for k in rec if 'test_head_forms_gpu' in k and '::' + fn + '[' in k]
        if len(mine) != n:
            pytest.skip('needs sections A to D of this file in one session; %s ran %d of %d cases' % (fn, len(mine), n))
        for k in mine:
            seen |= {s for s in rec[k] if is_head(s)}
    assert seen == H.ALL_INSTANCES, sorted(H.ALL_INSTANCES ^ seen)
