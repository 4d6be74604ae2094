"""Parity of every attention kernel form at its tile, cache and softmax edges, each case proving through the launch-instance log which kernels ran.

Two generations: attention.hip's attn_{fwd,bwd}2_kernel<HQ, CACHE, RAG> for H in {64, 128, 256} (HQ = H / 4; CACHE: h_t = fwd + bwd half of every step
kept in LDS, otherwise `out` is read twice; RAG: ragged batches) -- 12 + 12 instances -- and elementwise.hip's attn_{fwd,bwd}_kernel<RAG> for every other
width and for operands that are not 16-byte aligned.  R rows per pass, R * AU rows per loop trip: H = 64: 32 / 128, H = 128: 16 / 64, H = 256: 8 / 32.

Reference: tests/attention_ref.py's attention_from_pre() in float64, fed the pre-activations THE DEVICE computed, so relu(pre) and the mask pre > 0 are
the same numbers on both sides and the attention kernels are judged alone.  The projection is judged on its own: hsum bit-equal to the float32 sum over
k in order, pre against float64 hsum @ Wa.T + ba, dWa / dba / dh_n against float64 products of the device's dpre (read from the head of the workspace)
at the bounds of the exact GEMM (tests/test_kernels_gpu.py: relerr 2e-6 up to K = 128, 5e-6 above; every projection here is a gemm_small problem, which
the log confirms) and against products of the REFERENCE dpre at the suite's 1e-4.

Scales (attention_ref.make_case): 'flat' -- Wa and ba times 0.02, a nearly uniform softmax in which every step carries weight (at the scale of
test_attention the softmax is one-hot for H >= 128 and a dropped step moves nothing); 'unit' -- test_attention's; 'sat' -- flat with out times 6,
1 - tanh^2 ~ 0 and ctx six times larger; 'zeros' -- flat with exact 0.0 / -0.0 in pre on a quarter of the features, where the unmasked sum is not
zero.  Exact outcomes: the one-hot construction (scores 400 against -400), which also stands for the badly scaled regime no float32 reference follows.
Flat rows of fewer than 80 steps cannot have alpha.max() < 0.05 (a one-step row has alpha = 1): flatness is attention_ref.is_flat().
Ragged twins have B = 4: lengths_mix gives T, 1, 0 and its first interior length at the fourth utterance.

Bounds.  Ceiling (the suite's): ctx 1e-4 abs, alpha 1e-5 abs, dout / dpre / dh_n / dWa / dba relerr 1e-4.  Flat and zeros cases: 16 x the largest
deviation of float32 numpy from float64 over the same cases (tests/test_attention_ref_cpu.py measures it):
                         ctx abs    alpha abs   dout rel   dpre rel
  float32 numpy          3.7e-07    4.6e-08     3.4e-07    1.1e-06
  bound (16 x)           5.9e-06    7.4e-07     5.4e-06    1.8e-05
  MI355X, largest over   4.0e-07    4.5e-08     2.8e-07    5.5e-07      (per form below; the last test prints the table)
  the forms

Every case runs twice from fresh buffers and must repeat bit for bit (the slot-order sums are deterministic); `out` sits between NaN guard rows, every
output between fences of 7.0.  DEP_ATTN_V1 is read once per process into a static: testing it needs a child process and is left out.

Measured on the MI355X, largest figure over the flat and zeros cases of a form (dense .. ragged instance):
  attn_fwd2_kernel<16, true>   ctx 2.4e-07 .. 2.8e-07  alpha 5.2e-09 .. 1.9e-08      attn_bwd2_kernel<16, true>   dout 1.8e-07 .. 3.7e-08  dpre 2.6e-07 .. 2.7e-07
  attn_fwd2_kernel<16, false>  ctx 4.9e-08 .. 1.2e-07  alpha 3.9e-10 .. 8.2e-10      attn_bwd2_kernel<16, false>  dout 2.8e-07 .. 3.0e-09  dpre 2.2e-07 .. 1.5e-07
  attn_fwd2_kernel<32, true>   ctx 2.0e-07 .. 2.8e-07  alpha 2.2e-08 .. 2.0e-08      attn_bwd2_kernel<32, true>   dout 1.7e-07 .. 4.4e-08  dpre 3.4e-07 .. 1.8e-07
  attn_fwd2_kernel<32, false>  ctx 3.2e-08 .. 1.2e-07  alpha 6.4e-10 .. 1.1e-09      attn_bwd2_kernel<32, false>  dout 2.2e-07 .. 3.1e-09  dpre 1.4e-07 .. 1.8e-07
  attn_fwd2_kernel<64, true>   ctx 3.0e-07 .. 3.5e-07  alpha 2.4e-08 .. 4.5e-08      attn_bwd2_kernel<64, true>   dout 1.9e-07 .. 5.3e-08  dpre 2.6e-07 .. 3.2e-07
  attn_fwd2_kernel<64, false>  ctx 6.3e-08 .. 1.2e-07  alpha 1.8e-09 .. 8.4e-09      attn_bwd2_kernel<64, false>  dout 1.3e-07 .. 1.5e-08  dpre 1.4e-07 .. 1.8e-07
  attn_fwd_kernel              ctx 2.4e-07 .. 4.0e-07  alpha 3.3e-08 .. 4.1e-08      attn_bwd_kernel              dout 2.7e-07 .. 8.3e-08  dpre 5.5e-07 .. 5.5e-07
-- no worse than float32 numpy anywhere.  Unit and saturated cases (ceiling 1e-4 / 1e-5): ctx <= 3.1e-06, alpha <= 6.2e-07, dout <= 4.1e-06,
dpre <= 4.2e-06.  One finding on the way: (1, 35, 256) at the unit scale gave dpre relerr 1.6e-4 on attn_bwd2_kernel<64, true>.  Its softmax has
alpha.max() = 0.999, so dalpha - dot cancels to a thousandth and ONE float32 rounding of dot moves dpre by 0.9e-4 (attention_ref.dpre_condition); the
kernel's other figures in that case were 5e-7 .. 3e-6.  The unit cases are therefore chosen by that condition figure (tests/test_attention_ref_cpu.py),
T = 33 in its place; the badly conditioned regime is covered by the exact outcomes.
"""
import re

import numpy as np
import pytest

import attention_ref as A

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

GUARD = 4               # NaN rows of 2H floats before and after `out` (4: an aligned view stays aligned)
FENCE = 64              # floats of 7.0 before and after every output
AU = A.AU

_RAN = set()            # ids of the cases that ran in this session
_SEEN = set()           # attention kernel instances they launched
_FIG = {}               # (kernel form, 'flat' | 'other') -> {figure: largest}


# ----------------------------------------------------------------------------- buffers
def _place_out(x, off):
    B, T, W = x.shape
    buf = np.full(off + (B * T + 2 * GUARD) * W + 3, np.nan, dtype=np.float32)
    buf[off + GUARD * W:off + (GUARD + B * T) * W] = x.ravel()
    t = torch.from_numpy(buf).to(DEV)
    return t, t[off + GUARD * W:off + (GUARD + B * T) * W]


def _place_vec(x, off=0):
    buf = np.full(off + x.size + 8, np.nan, dtype=np.float32)
    buf[off + 4:off + 4 + x.size] = x.ravel()
    t = torch.from_numpy(buf).to(DEV)
    return t, t[off + 4:off + 4 + x.size]


def _fenced(n):
    t = torch.full((n + 2 * FENCE,), 7.0, dtype=torch.float32, device=DEV)
    return t, t[FENCE:FENCE + n]


def _take(t, n, what):
    """The n floats between the fences, after checking that the fences are still 7.0."""
    h = t.cpu().numpy()
    assert (h[:FENCE] == 7.0).all() and (h[FENCE + n:] == 7.0).all(), 'written outside ' + what
    return h[FENCE:FENCE + n]


# ----------------------------------------------------------------------------- which kernel ran
_INST = re.compile(r'^\(?\s*(\w+)\s*(?:<([^>]*)>)?')


def _drain(request):
    """What the library launched since the last call of this function, normalised to `name` or `name<arg, ..>`; the raw entries go to the per-test
    record conftest.py keeps for tests/test_step_coverage_gpu.py."""
    raw = L.instance_log_read(reset=True)
    rec = getattr(request.config, '_dep_instances', None)
    if rec is not None:
        rec.setdefault(request.node.nodeid, set()).update(raw)
    out = set()
    for s in raw:
        m = _INST.match(s)
        assert m, s
        out.add(m.group(1) if m.group(2) is None else '%s<%s>' % (m.group(1), ', '.join(a.strip() for a in m.group(2).split(',') if a.strip())))
    return out


def _v2(d, H, cache, rag):
    return 'attn_%s2_kernel<%d, %s%s>' % (d, H // 4, 'true' if cache else 'false', ', true' if rag else '')


def _v1(d, rag):
    return 'attn_%s_kernel<%s>' % (d, 'true' if rag else '')


def _forms(H, T, rag):
    if H in (64, 128, 256):
        cf, cb = A.cached(H, T)
        return _v2('fwd', H, cf, rag), _v2('bwd', H, cb, rag)
    return _v1('fwd', rag), _v1('bwd', rag)


# ----------------------------------------------------------------------------- one forward and backward through the C ABI
def _call(request, c, off_out=0, off_dctx=0, pre_bits=None):
    lib = L.load()
    B, T, H, K = c['B'], c['T'], c['H'], c['K']
    keep = [_place_out(c['out_in'], off_out), _place_vec(c['hn']), _place_vec(c['Wa']), _place_vec(c['ba']), _place_vec(c['dctx'], off_dctx)]
    out, hn, Wa, ba, dctx = (v for _, v in keep)
    assert (out.data_ptr() % 16 == 0) == (off_out == 0) and (dctx.data_ptr() % 16 == 0) == (off_dctx == 0)
    lens = None if c['lengths'] is None else torch.from_numpy(np.array(c['lengths'], dtype=np.int32)).to(DEV)
    n = dict(ctx=B * H, alpha=B * T, pre=B * H, hsum=B * H, dout=B * T * 2 * H, dhn=K * B * H, dWa=H * H, dba=H,
             ws=(lib.dep_attn_bwd_workspace_bytes(B, T, H) + 3) // 4)
    a = {k: _fenced(v) for k, v in n.items()}
    p = lambda k: a[k][1].data_ptr()
    _drain(request)
    if lens is None:
        L.check(lib.dep_attn_fwd(out.data_ptr(), hn.data_ptr(), K, Wa.data_ptr(), ba.data_ptr(), p('ctx'), p('alpha'), p('pre'), p('hsum'), B, T, H,
                                 L.stream()), 'dep_attn_fwd')
    else:
        L.check(lib.dep_attn_fwd_varlen(out.data_ptr(), lens.data_ptr(), hn.data_ptr(), K, Wa.data_ptr(), ba.data_ptr(), p('ctx'), p('alpha'), p('pre'),
                                        p('hsum'), B, T, H, L.stream()), 'dep_attn_fwd_varlen')
    torch.cuda.synchronize()
    fwd = _drain(request)
    pre_fwd = a['pre'][1].cpu().numpy().copy()
    if pre_bits is not None:                                # the same VALUES with chosen zero signs: what the forward computed is not changed by it
        assert np.array_equal(pre_bits.ravel(), pre_fwd), 'pre is not what the construction says'
        a['pre'][1].copy_(torch.from_numpy(np.array(pre_bits, dtype=np.float32).ravel()))
    if lens is None:
        L.check(lib.dep_attn_bwd(dctx.data_ptr(), out.data_ptr(), Wa.data_ptr(), p('alpha'), p('pre'), p('hsum'), K, p('dout'), p('dhn'), p('dWa'),
                                 p('dba'), B, T, H, p('ws'), n['ws'] * 4, L.stream()), 'dep_attn_bwd')
    else:
        L.check(lib.dep_attn_bwd_varlen(dctx.data_ptr(), out.data_ptr(), lens.data_ptr(), Wa.data_ptr(), p('alpha'), p('pre'), p('hsum'), K, p('dout'),
                                        p('dhn'), p('dWa'), p('dba'), B, T, H, p('ws'), n['ws'] * 4, L.stream()), 'dep_attn_bwd_varlen')
    torch.cuda.synchronize()
    bwd = _drain(request)
    return dict(alloc={k: v[0] for k, v in a.items()}, n=n, fwd=fwd, bwd=bwd)


def _host(r, c):
    B, T, H, K = c['B'], c['T'], c['H'], c['K']
    shape = dict(ctx=(B, H), alpha=(B, T), pre=(B, H), hsum=(B, H), dout=(B, T, 2 * H), dhn=(K, B, H), dWa=(H, H), dba=(H,))
    h = {k: _take(r['alloc'][k], r['n'][k], k).reshape(s) for k, s in shape.items()}
    h['dpre'] = _take(r['alloc']['ws'], r['n']['ws'], 'the workspace')[:B * H].reshape(B, H)        # dep_attn_bwd keeps dpre at the head of its workspace
    return h


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _note(form, kind, figs):
    f = _FIG.setdefault((form, kind), {})
    for k, v in figs.items():
        f[k] = max(f.get(k, 0.0), v)


def _judge(c, r, h, bounds, fwd_form, bwd_form, label):
    B, T, H, K = c['B'], c['T'], c['H'], c['K']
    attn = lambda s: {x for x in s if x.startswith('attn_')}
    gemm = lambda s: {x for x in s if 'gemm' in x or 'splitk' in x}
    assert attn(r['fwd']) == {'attn_hsum_kernel', fwd_form}, (label, r['fwd'])
    assert attn(r['bwd']) == {bwd_form, 'attn_bcast_kernel'}, (label, r['bwd'])
    assert gemm(r['fwd']) == {'gemm_small'} and gemm(r['bwd']) == {'gemm_small'}, (label, r['fwd'], r['bwd'])      # the exact kernel: its bounds below
    _SEEN.update(attn(r['fwd']) | attn(r['bwd']))
    for k, v in h.items():
        assert np.isfinite(v).all(), '%s: NaN / Inf in %s (a guard row or a step behind a length was read, or an element was not written)' % (label, k)
    w = {k: v.astype(np.float64) for k, v in h.items()}
    Wa, ba = c['Wa'].astype(np.float64), c['ba'].astype(np.float64)
    gb = lambda Kc: 2e-6 if Kc <= 128 else 5e-6
    # the projection, forward
    assert np.array_equal(_bits(h['hsum']), _bits(A.hsum_f32(c['hn']))), label + ': hsum is not the float32 sum over k in order'
    e_pre = A.relerr(w['pre'], w['hsum'] @ Wa.T + ba)
    assert e_pre < gb(H), (label, 'pre', e_pre)
    # the attention kernels, on the device's own pre
    ref = A.attention_from_pre(c['out_in'], h['pre'], c['dctx'], c['lengths'])
    if c['scale'] in ('flat', 'zeros'):
        assert A.is_flat(ref[1], c['lengths']), (label, ref[1].max())
        if c['lengths'] is None and T >= 80:
            assert ref[1].max() < 0.05, (label, ref[1].max())
    dev = A.deviations((w['ctx'], w['alpha'], w['dout'], w['dpre']), ref)
    print('%-44s %-34s %-40s ctx %.3g alpha %.3g dout %.3g dpre %.3g pre %.3g' % (label, fwd_form, bwd_form, dev['ctx'], dev['alpha'], dev['dout'], dev['dpre'], e_pre))
    kind = 'flat' if c['scale'] in ('flat', 'zeros') else 'other'
    _note(fwd_form, kind, dict(ctx=dev['ctx'], alpha=dev['alpha'])); _note(bwd_form, kind, dict(dout=dev['dout'], dpre=dev['dpre']))
    for k, v in dev.items():
        assert v < bounds[k], (label, k, v, bounds[k])
    if c['lengths'] is not None:
        pad = np.arange(T)[None, :] >= c['lengths'][:, None]
        assert not _bits(h['alpha'])[pad].any(), label + ': alpha is not exactly 0 behind the utterance'
        assert not _bits(h['dout'])[pad].any(), label + ': dout is not exactly 0 behind the utterance'
        empty = c['lengths'] == 0
        assert not _bits(h['ctx'])[empty].any(), label + ': an empty row must give ctx = 0'
        assert not h['dpre'][empty].any(), label + ': an empty row has no gradient'
    # the projection, backward: the GEMMs on the dpre they were given, then the whole against the reference's dpre
    for k in range(1, K):
        assert np.array_equal(_bits(h['dhn'][k]), _bits(h['dhn'][0])), label + ': the K slices of dh_n differ'
    e = dict(dWa=A.relerr(w['dWa'], w['dpre'].T @ w['hsum']), dhn=A.relerr(w['dhn'][0], w['dpre'] @ Wa))
    assert e['dWa'] < gb(B) and e['dhn'] < gb(H), (label, e)
    assert (np.abs(w['dba'] - w['dpre'].sum(0)) <= 2e-6 * np.abs(w['dpre']).sum(0)).all(), label + ': dba'
    e = dict(dWa=A.relerr(w['dWa'], ref[3].T @ w['hsum']), dhn=A.relerr(w['dhn'][0], ref[3] @ Wa), dba=A.relerr(w['dba'], ref[3].sum(0)))
    for k, v in e.items():
        assert v < 1e-4, (label, k, v)
    return ref


def _run(request, c, bounds, label, off_out=0, off_dctx=0, pre_bits=None, forms=None):
    """The case twice from fresh buffers: bit-identical, fences intact, the expected instances, inside the bounds.  Returns (host arrays, reference)."""
    fwd_form, bwd_form = forms or _forms(c['H'], c['T'], c['lengths'] is not None)
    r0 = _call(request, c, off_out, off_dctx, pre_bits)
    r1 = _call(request, c, off_out, off_dctx, pre_bits)
    h = _host(r0, c)
    ref = _judge(c, r0, h, bounds, fwd_form, bwd_form, label)
    assert r0['fwd'] == r1['fwd'] and r0['bwd'] == r1['bwd']
    for k in r0['alloc']:
        assert torch.equal(r0['alloc'][k], r1['alloc'][k]), '%s: two runs differ in %s' % (label, k)
    return h, ref


def _case(H, T, ragged, scale):
    return A.make_case(H, T, A.RAGGED_B if ragged else A.dense_B(H, T), scale, ragged)


def _label(c):
    return '%s B=%d T=%d H=%d %s' % (c['scale'], c['B'], c['T'], c['H'], 'ragged' if c['lengths'] is not None else 'dense')


RAG = pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])


# ----------------------------------------------------------------------------- attention.hip: tile edges, cache border, softmax stride (flat)
@RAG
@pytest.mark.parametrize('H,T', [(H, T) for H in (64, 128, 256) for T in A.tile_edges(H)])
def test_tile_edges(request, H, T, ragged):
    """T = 1, R - 1, R, R + 1, R AU - 1, R AU, R AU + 1, 2 R AU + 3: the clamped tail loads, the u R + g row map, the R partial rows."""
    _RAN.add(request.node.name)
    c = _case(H, T, ragged, 'flat')
    _run(request, c, A.flat_bounds(), _label(c), forms=(_v2('fwd', H, True, ragged), _v2('bwd', H, True, ragged)))


@RAG
@pytest.mark.parametrize('H,T,cf,cb', A.CACHE_BORDER + A.SOFTMAX_STRIDE)
def test_cache_border_and_softmax_stride(request, H, T, cf, cb, ragged):
    """The last T each direction caches, the band in which only the forward does, the first T both re-read; T = 513: a second trip of the t += AT loops."""
    _RAN.add(request.node.name)
    c = _case(H, T, ragged, 'flat')
    _run(request, c, A.flat_bounds(), _label(c), forms=(_v2('fwd', H, cf, ragged), _v2('bwd', H, cb, ragged)))


# ----------------------------------------------------------------------------- the other scales, one T per form
@RAG
@pytest.mark.parametrize('scale', ['unit', 'sat'])
@pytest.mark.parametrize('H,which', [(H, i) for H in (64, 128, 256) for i in range(3)])
def test_unit_and_saturated_scales(request, H, which, scale, ragged):
    _RAN.add(request.node.name)
    c = _case(H, A.FORM_T[H][which], ragged, scale)
    _run(request, c, A.CEILING, _label(c))


@RAG
@pytest.mark.parametrize('H,T', A.ZEROS)
def test_exact_zeros_in_pre_are_masked(request, H, T, ragged):
    """pre is 0.0 or -0.0 on a quarter of the features (zero rows of Wa, ba = +-0) while the sum over t the mask has to drop is not zero: dpre, the
    rows of dWa and the elements of dba of those features are bit-zero.  The backward is handed both signs of zero whatever the GEMM's epilogue made."""
    _RAN.add(request.node.name)
    c = _case(H, T, ragged, 'zeros')
    z = c['zero_j']
    dev_pre = _host(_call(request, c), c)['pre']
    assert not dev_pre[:, z].any(), 'pre is not an exact zero where Wa has a zero row and ba is +-0'
    pre_bits = dev_pre.copy(); pre_bits[:, z] = c['ba'][z]           # the device's values, the zero signs of ba
    assert np.signbit(pre_bits[:, z]).any() and not np.signbit(pre_bits[:, z]).all()
    h, ref = _run(request, c, A.flat_bounds(), _label(c), pre_bits=pre_bits)
    live = np.ones(c['B'], bool) if c['lengths'] is None else c['lengths'] > 1
    open_pre = h['pre'].astype(np.float64); open_pre[:, z] = 1e-30
    unmasked = A.attention_from_pre(c['out_in'], open_pre, c['dctx'], c['lengths'])[3]
    assert (np.abs(unmasked[live][:, z]) > 1e-3 * np.abs(ref[3]).max()).mean() > 0.9, 'the mask has nothing to drop in this case'
    assert not _bits(h['dpre'])[:, z].any() and not _bits(h['dWa'])[z].any() and not _bits(h['dba'])[z].any()


# ----------------------------------------------------------------------------- exact outcomes
def _exact(request, c, forms=None):
    B, T, H = c['B'], c['T'], c['H']
    h, _ = _run(request, c, A.CEILING, _label(c) + ' t*=%s' % list(c['tstar']), pre_bits=np.broadcast_to(c['ba'], (B, H)), forms=forms)
    hsum = c['out'][..., :H] + c['out'][..., H:]                                   # fl32(out_fwd + out_bwd)
    for b in range(B):
        t = int(c['tstar'][b])
        if t < 0:
            assert not _bits(h['ctx'][b]).any() and not _bits(h['alpha'][b]).any() and not _bits(h['dout'][b]).any()
            continue
        want = np.zeros(T, np.float32); want[t] = 1.0
        assert np.array_equal(h['alpha'][b], want), (b, 'alpha is not exactly one-hot')
        assert np.array_equal(_bits(h['ctx'][b]), _bits(hsum[b, t])), (b, 'ctx is not row t* of fwd + bwd')
        assert np.array_equal(_bits(h['dout'][b, t]), _bits(np.concatenate([c['dctx'][b], c['dctx'][b]]))), (b, 'dout[t*] is not dctx in both halves')
        assert not np.delete(h['dout'][b], t, axis=0).any(), (b, 'dout is not exactly 0 off t*')
    z = c['zero_j']
    assert z.sum() == H - 4
    assert not _bits(h['dba'])[z].any() and not _bits(h['dWa'])[z].any() and not _bits(h['dpre'])[:, z].any()


@pytest.mark.parametrize('which', range(4), ids=['first', 'last', 'RAU-1', 'RAU'])
@pytest.mark.parametrize('reread', [False, True], ids=['cached', 're-read'])
@pytest.mark.parametrize('H', [64, 128, 256])
def test_one_hot_softmax_has_exact_outcomes(request, H, reread, which):
    _RAN.add(request.node.name)
    RA = A.rows_per_pass(H) * AU
    T = A.FORM_T[H][2] if reread else RA + 2
    tstar = [0, T - 1, RA - 1, RA][which]
    assert A.cached(H, T) == (not reread, not reread)
    _exact(request, A.make_exact_case(H, T, 1 + (which + H // 64) % 3, tstar))


@pytest.mark.parametrize('reread', [False, True], ids=['cached', 're-read'])
@pytest.mark.parametrize('H', [64, 128, 256, 96])
def test_one_hot_softmax_has_exact_outcomes_ragged(request, H, reread):
    """t* = len - 1 in every utterance; the empty one gives ctx = 0 bits.  H = 96: the first-generation kernels (one T: they have no second form)."""
    _RAN.add(request.node.name)
    if H == 96:
        T = 257 if reread else 5
    else:
        T = A.FORM_T[H][2] if reread else A.rows_per_pass(H) * AU + 2
    _exact(request, A.make_exact_case(H, T, A.RAGGED_B, 0, ragged=True))


# ----------------------------------------------------------------------------- the first-generation kernels and the alignment fallback
@RAG
@pytest.mark.parametrize('T', A.V1_T)
@pytest.mark.parametrize('H', A.V1_H)
def test_first_generation_kernels(request, H, T, ragged):
    """H = 96, 100: no multiple of the 64-lane stride; 320: above the block's 256 threads; T = 3, 4, 5 around the four waves; 257 above the threads."""
    _RAN.add(request.node.name)
    c = _case(H, T, ragged, 'flat')
    _run(request, c, A.flat_bounds(), _label(c), forms=(_v1('fwd', ragged), _v1('bwd', ragged)))


@RAG
@pytest.mark.parametrize('what', ['out', 'dctx'])
@pytest.mark.parametrize('H,T', [(128, 67), (64, 131)])
def test_alignment_fallback(request, H, T, what, ragged):
    """`out` one float into its allocation: both directions fall back.  `dctx` one float in: the forward stays on attention.hip and only the backward
    falls back, on the alpha the other generation wrote.  The aligned twin of the same data agrees within the bounds."""
    _RAN.add(request.node.name)
    c = _case(H, T, ragged, 'flat')
    bounds = A.flat_bounds()
    forms = (_v1('fwd', ragged) if what == 'out' else _v2('fwd', H, True, ragged), _v1('bwd', ragged))
    h, _ = _run(request, c, bounds, _label(c) + ' %s+4B' % what, off_out=int(what == 'out'), off_dctx=int(what == 'dctx'), forms=forms)
    h2, _ = _run(request, c, bounds, _label(c) + ' aligned', forms=(_v2('fwd', H, True, ragged), _v2('bwd', H, True, ragged)))
    assert np.array_equal(_bits(h['pre']), _bits(h2['pre']))
    if what == 'dctx':
        assert np.array_equal(_bits(h['ctx']), _bits(h2['ctx'])) and np.array_equal(_bits(h['alpha']), _bits(h2['alpha']))     # the same forward kernel
    w = lambda x: x.astype(np.float64)
    twin = A.deviations(tuple(w(h[k]) for k in ('ctx', 'alpha', 'dout', 'dpre')), tuple(w(h2[k]) for k in ('ctx', 'alpha', 'dout', 'dpre')))
    for k, v in twin.items():
        assert v < bounds[k], (k, v)
    for k in ('dWa', 'dba', 'dhn'):
        assert A.relerr(w(h[k]), w(h2[k])) < 1e-4, k


@pytest.mark.parametrize('B,H', [(3, 85), (2, 128), (1, 257)])
@pytest.mark.parametrize('K', [1, 2, 4, 6])
def test_hsum_and_broadcast_over_k(request, K, B, H):
    """attn_hsum_kernel / attn_bcast_kernel at B H = 255, 256, 257 (one block of 256 threads, and one element into the second) for K = 1, 2, 4, 6:
    hsum bit-exact, the K slices of dh_n bit-identical (both asserted by every case of this file; here K and B H vary)."""
    _RAN.add(request.node.name)
    c = A.make_case(H, 5, B, 'flat', False, K=K)
    _run(request, c, A.flat_bounds(), _label(c) + ' K=%d' % K)


# ----------------------------------------------------------------------------- every instance reached
N_CASES = 2 * (24 + len(A.CACHE_BORDER + A.SOFTMAX_STRIDE) + 18 + len(A.ZEROS) + len(A.V1_H) * len(A.V1_T) + 4) + 24 + 8 + 12


def test_every_attention_instance_was_reached():
    """The union of what the cases above launched: all 12 attn_fwd2_kernel and all 12 attn_bwd2_kernel instances, both attn_fwd_kernel and both
    attn_bwd_kernel instances.  Needs the whole file to have run."""
    if len(_RAN) != N_CASES:
        pytest.skip('collects what the other tests of this file launched: run the whole file (%d of its %d cases ran in this session)' % (len(_RAN), N_CASES))
    want = {_v2(d, H, cache, rag) for d in ('fwd', 'bwd') for H in (64, 128, 256) for cache in (True, False) for rag in (True, False)}
    want |= {_v1(d, rag) for d in ('fwd', 'bwd') for rag in (True, False)}
    assert len(want) == 28
    for form, kind in sorted(_FIG):
        print('%-36s %-5s %s' % (form, kind, '  '.join('%s %.3g' % kv for kv in sorted(_FIG[(form, kind)].items()))))
    assert want <= _SEEN, sorted(want - _SEEN)
    assert _SEEN <= want | {'attn_hsum_kernel', 'attn_bcast_kernel'}, sorted(_SEEN - want)
