"""Operator-level parity of every register-staged GEMM form at ragged edges, each case proving through the launch-instance log which kernel it ran.

gemm_plan() (gemm.hip) picks among gemm_small, gemm_mfma<TA, TB, VEC> (+ splitk_reduce) and gemm_bf16x3<TA, TB, VEC, BMT, TERMS> (+ splitk_reduce2);
split_form() (gemm_bf16x3.hip) picks the row tile BMT.  The cases below are the smallest shapes that reach each form with
  * a last M tile / N tile of 4 (vector loaders) or 2 (scalar loaders) rows / columns, a K tail of 4, 1, 5 or 13 behind full 32-wide k-tiles,
  * the scalar loaders for each of their three reasons (contiguous dimension % 4, ld % 4, a view one float into its allocation),
  * bias / beta / ldc > N / an unaligned C in the kernel's vector AND scalar epilogue branches and in both reduce kernels,
  * split-K with the full workspace, with room for two partials only, and with none.
Reference: float64 product of the fp32-rounded inputs, ref = opA @ opB + bias + beta * C0; err = |got - ref| / (|opA| @ |opB| + |bias| + |beta * C0|).
Bounds are those of tests/test_kernels_gpu.py: three-term split err.max < 1.5e-5 and err.mean < 2e-6; single products (mode 2) 2e-5 < err.max < 1e-2;
exact path relerr < 2e-6 (K <= 128) / 5e-6 (above).  K >= 16 everywhere: at K = 4 the IDEAL three-term split already has err.max 1.8e-5.
Operands sit inside NaN: padding columns and four guard rows on either side, so a stray read that enters a product shows.  C sits inside 7.0.

Measured on the MI355X (largest figure over the cases of a form; the last test prints the table):
  gemm_bf16x3<.., 3>   err.max 7.2e-06 .. 7.8e-06 on the ten forms reached at K = 33 / 36, 1.4e-06 / 1.5e-06 on the two NT 256-row forms (K = 548 / 549);
                       err.mean <= 9.2e-07 (2.4e-07 on the NT 256-row forms)
  gemm_bf16x3<.., 1>   err.max 2.8e-03 .. 3.0e-03 on the ten forms reached at K = 33 / 36, 7.2e-04 / 7.6e-04 on the two NT 256-row forms
  gemm_mfma            relerr <= 3.4e-07 at K <= 128 and <= 1.6e-06 above, on each of the six forms (K = 1101 unsplit; 8.8e-07 with two partials, 5.2e-07 with four)
  gemm_small           relerr 1.3e-07 at K = 64, 1.1e-06 at K = 8192
The ideal split (numpy: bf16 round-to-nearest hi and lo, hi*hi + hi*lo + lo*hi in float64) gives the same three-term figures to two digits.
"""
import functools
import re
import zlib

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

GUARD = 4                                       # NaN rows before and after an operand (4: a guard of ld floats keeps an aligned view aligned)
TRANS = [(0, 1), (0, 0), (1, 0)]
TNAME = {(0, 1): 'NT', (0, 0): 'NN', (1, 0): 'TN'}

# name: M, N, K, loader kind of A and B, BMT per transpose form, split-K count the shape asks for (0: none).
# Loader kinds -- 'vec': ld = width, 16-byte aligned.  The scalar ones, by reason:
#   'dim'    the contiguous dimension is no multiple of 4 (ld rounded up to one, aligned view)           S1
#   'ld'     ld % 4 != 0 (aligned view)                                                                  S2 (and V1 in the same-bits test)
#   'off'    the view starts one float into its allocation (ld a multiple of 4)                          S3 (and V1, V4, V5 in the same-bits test)
#   'off+ld' both                                                                                        S4
CASES = {
    'V1': dict(M=1028, N=772, K=36, kind='vec', bmt=dict(NT=128, NN=256, TN=256), want=0),      # 9 x 7 = 63 tiles; 4-row / 4-column last tiles; K = 32 + 4
    'S1': dict(M=1030, N=770, K=33, kind='dim', bmt=dict(NT=128, NN=256, TN=256), want=0),      # 2-wide tails, K tail 1
    'V2': dict(M=260, N=1412, K=36, kind='vec', bmt=dict(NT=128, NN=128, TN=128), want=0),      # 3 x 12 = 36 tiles, M < 512
    'S2': dict(M=258, N=1410, K=33, kind='ld', bmt=dict(NT=128, NN=128, TN=128), want=0),
    'V3': dict(M=1028, N=772, K=548, kind='vec', bmt=dict(NT=256, NN=256, TN=256), want=0),     # NT with K >= 512
    'S3': dict(M=1030, N=770, K=549, kind='off', bmt=dict(NT=256, NN=256, TN=256), want=0),     # K tail 5
    'V4': dict(M=520, N=388, K=1100, kind='vec', bmt=dict(NT=256, NN=256, TN=256), want=4),     # 20 tiles but M*N*K > 2^27; chunks of 288, the last 236
    'S4': dict(M=522, N=386, K=1101, kind='off+ld', bmt=dict(NT=256, NN=256, TN=256), want=4),  # last chunk 237 = 7 x 32 + 13
    'V5': dict(M=260, N=388, K=1500, kind='vec', bmt=dict(NT=128, NN=128, TN=128), want=5),     # chunks of 320, the last 220
}

# Epilogue options.  ldc: 'N' | 'N+3' | 'up4' (the next multiple of 4 above N: an aligned, vector-store C whose last quad of a row may be partial);
# coff: the C view starts one float into its allocation (scalar store branch); ws: 'full' | 'two' (room for exactly two partials) | None.
OPTS = [
    dict(bias=True, beta=0.0, ldc='N', coff=0, ws='full'),
    dict(bias=False, beta=0.5, ldc='N+3', coff=0, ws='two'),
    dict(bias=True, beta=0.5, ldc='N', coff=1, ws=None),
    dict(bias=True, beta=0.5, ldc='up4', coff=0, ws='full'),
]

_RAN = set()            # keys of the form-reaching cases that ran in this session
_SEEN = {}              # case key -> set of launch instances (normalised)
_FIG = {}               # kernel form -> [largest err.max | relerr, largest err.mean, smallest err.max]


# ----------------------------------------------------------------------------- problems and references (computed once, shared, read-only)
def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _make(M, N, K, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    opA, opB, bias, C0 = f(M, K), f(K, N), f(N), f(M, N)
    return dict(M=M, N=N, K=K, opA=opA, opB=opB, bias=bias, C0=C0)


def _with_ref(p, opB_eff=None):
    a = p['opA'].astype(np.float64); b = (p['opB'] if opB_eff is None else opB_eff).astype(np.float64)
    p['P'] = a @ b
    p['S'] = np.abs(a) @ np.abs(b)
    return _freeze(p)


@functools.lru_cache(maxsize=None)
def _problem(name):
    c = CASES[name]
    return _with_ref(_make(c['M'], c['N'], c['K'], zlib.crc32(name.encode())))


@functools.lru_cache(maxsize=None)
def _problem_mnk(M, N, K):
    return _with_ref(_make(M, N, K, M * 7 + N * 3 + K))


@functools.lru_cache(maxsize=None)
def _problem_shift(M, N, K, T, shift):
    """dW_hh-style operand: row r of B is read from row r + shift, zero where (r % T) + shift leaves [0, T) -- built as test_gemm_splitk_and_shift builds it."""
    p = _make(M, N, K, M + N + K)                       # (the same A, B for both shifts)
    Bsz = K // T
    B3 = p['opB'].reshape(Bsz, T, N)
    Bs = np.zeros_like(p['opB'])
    if shift == -1:
        Bs.reshape(Bsz, T, N)[:, 1:] = B3[:, :-1]
    else:
        Bs.reshape(Bsz, T, N)[:, :-1] = B3[:, 1:]
    return _with_ref(p, Bs)


def _reference(p, bias, beta):
    ref = p['P'].copy(); scale = p['S'].copy()
    if bias:
        ref += p['bias'].astype(np.float64); scale += np.abs(p['bias'].astype(np.float64))
    if beta:
        ref += beta * p['C0'].astype(np.float64); scale += np.abs(beta * p['C0'].astype(np.float64))
    return ref, scale


# ----------------------------------------------------------------------------- buffers
def _ld(width, kind):
    if kind == 'vec':
        return width
    if kind in ('dim', 'off'):
        return (width + 3) // 4 * 4
    ld = width + 3
    return ld + (ld % 4 == 0)


def _place(x, kind):
    """x (rows, width) inside a NaN allocation: padding columns up to ld, GUARD NaN rows before and after, the view one float in for the 'off' kinds.
    Returns (allocation, view, ld); the view's data_ptr() is element (0, 0)."""
    rows, width = x.shape
    ld = _ld(width, kind); off = 1 if kind.startswith('off') else 0
    buf = np.full(off + (rows + 2 * GUARD) * ld + 3, np.nan, dtype=np.float32)
    buf[off:off + (rows + 2 * GUARD) * ld].reshape(rows + 2 * GUARD, ld)[GUARD:GUARD + rows, :width] = x
    t = torch.from_numpy(buf).to(DEV)
    return t, t[off + GUARD * ld:], ld


def _is_vector(view, ld, contiguous_dim):
    """The issue's definition of an operand the vector loaders may fetch."""
    return view.data_ptr() % 16 == 0 and ld % 4 == 0 and contiguous_dim % 4 == 0


def _place_bias(bias):
    buf = np.full(bias.size + 8, np.nan, dtype=np.float32)
    buf[4:4 + bias.size] = bias
    t = torch.from_numpy(buf).to(DEV)
    return t, t[4:]


def _ldc(N, how):
    return {'N': N, 'N+3': N + 3, 'up4': N // 4 * 4 + 4}[how]


def _place_c(p, beta, ldc, coff):
    """(M + 2, ldc) of 7.0, `coff` floats into its allocation; the M x N block holds C0 when beta != 0 and NaN when beta == 0 (which must not read C)."""
    M, N = p['M'], p['N']
    buf = np.full(coff + (M + 2) * ldc + 3, 7.0, dtype=np.float32)
    buf[coff:coff + (M + 2) * ldc].reshape(M + 2, ldc)[1:M + 1, :N] = p['C0'] if beta else np.nan
    t = torch.from_numpy(buf).to(DEV)
    return t, t[coff + ldc:]


def _take_c(t, p, ldc, coff):
    """The M x N block as float64, after checking that everything around it is still exactly 7.0."""
    M, N = p['M'], p['N']
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    body = h[coff:coff + (M + 2) * ldc].reshape(M + 2, ldc)
    assert (h[:coff] == 7.0).all() and (h[coff + (M + 2) * ldc:] == 7.0).all(), 'written outside the C allocation view'
    assert (body[0] == 7.0).all() and (body[M + 1] == 7.0).all(), 'written above or below the M x N block'
    assert (body[1:M + 1, N:] == 7.0).all(), 'written into columns N..ldc'
    return body[1:M + 1, :N].astype(np.float64)


# ----------------------------------------------------------------------------- which kernel ran
_INST = re.compile(r'^\(?\s*(\w+)\s*(?:<([^>]*)>)?')


def _drain(request):
    """What the library launched since the last call of this function, normalised to `name` or `name<arg, arg, ..>`.  The log is emptied, so the raw
    entries are handed to the per-test record conftest.py keeps for tests/test_step_coverage_gpu.py."""
    raw = L.instance_log_read(reset=True)
    rec = getattr(request.config, '_dep_instances', None)
    if rec is not None:
        rec.setdefault(request.node.nodeid, set()).update(raw)
    out = set()
    for s in raw:
        m = _INST.match(s)
        assert m, s
        out.add(m.group(1) if m.group(2) is None else '%s<%s>' % (m.group(1), ', '.join(a.strip() for a in m.group(2).split(','))))
    return out


def _b(x):
    return 'true' if x else 'false'


def _x3(tA, tB, vec, bmt, terms):
    return 'gemm_bf16x3<%s, %s, %s, %d, %d>' % (_b(tA), _b(tB), _b(vec), bmt, terms)


def _mfma(tA, tB, vec):
    return 'gemm_mfma<%s, %s, %s>' % (_b(tA), _b(tB), _b(vec))


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _note(form, hi, mean=0.0):
    f = _FIG.setdefault(form, [0.0, 0.0, np.inf])
    f[0] = max(f[0], hi); f[1] = max(f[1], mean); f[2] = min(f[2], hi)


def _judge(form, path, got, ref, scale, K, label):
    """path: 'x3' | 'x1' | 'exact'.  Prints the figures, then asserts the path's bound."""
    assert np.isfinite(got).all(), label + ': NaN / Inf in the result (a guard or padding element entered a product, or an element was not written)'
    if path == 'exact':
        r = _relerr(got, ref)
        print('%-60s %-42s relerr %.3g' % (label, form, r))
        _note(form, r)
        assert r < (2e-6 if K <= 128 else 5e-6), (label, r)
        return
    err = np.abs(got - ref) / scale
    print('%-60s %-42s err.max %.3g err.mean %.3g' % (label, form, err.max(), err.mean()))
    _note(form, err.max(), err.mean())
    if path == 'x3':
        assert err.max() < 1.5e-5, (label, err.max())
        assert err.mean() < 2e-6, (label, err.mean())
    else:
        assert 2e-5 < err.max() < 1e-2, (label, err.max())


# ----------------------------------------------------------------------------- one call, run twice
def _run(request, entry, p, tA, tB, kind_a, kind_b, opt, want, seq_T=0, shiftB=0, key=None):
    """entry(..) on problem p from freshly placed buffers, twice.  Returns (result M x N as float64, C allocation of the first run, launched set,
    vec: whether the operands meet the vector loaders' conditions)."""
    M, N, K = p['M'], p['N'], p['K']
    A = np.ascontiguousarray(p['opA'].T) if tA else p['opA']
    B = np.ascontiguousarray(p['opB'].T) if tB else p['opB']
    a_all, a, lda = _place(A, kind_a)
    b_all, b, ldb = _place(B, kind_b)
    vec = _is_vector(a, lda, M if tA else K) and _is_vector(b, ldb, K if tB else N)
    bi_all, bi = _place_bias(p['bias']) if opt['bias'] else (None, None)
    ldc = _ldc(N, opt['ldc']); coff = opt['coff']
    ws = None
    if opt['ws'] == 'full':
        ws = L.gemm_ws(tA, tB, M, N, K, DEV)
        assert ws.numel() >= want * M * N                 # room for every partial the shape asks for
    elif opt['ws'] == 'two' and want:
        ws = torch.empty(2 * M * N, dtype=torch.float32, device=DEV)
    runs = []
    for _ in range(2):
        c_all, c = _place_c(p, opt['beta'], ldc, coff)
        _drain(request)
        entry(tA, tB, M, N, K, a, lda, b, ldb, c, ldc, bias=bi, beta=opt['beta'], seq_T=seq_T, shiftB=shiftB, ws=ws)
        torch.cuda.synchronize()
        runs.append((c_all, _drain(request)))
        if key is not None:
            _SEEN.setdefault(key, set()).update(runs[-1][1])
    assert runs[0][1] == runs[1][1], runs
    got = _take_c(runs[0][0], p, ldc, coff)
    assert torch.equal(runs[0][0], runs[1][0]), 'two runs of one call differ'
    return got, runs[0][0], runs[0][1], vec


def _label(name, tA, tB, opt, extra=''):
    return '%s %s %sbias=%d beta=%g ldc=%s coff=%d ws=%s' % (name, TNAME[(tA, tB)], extra, opt['bias'], opt['beta'], opt['ldc'], opt['coff'], opt['ws'])


def _reduces(opt, want):
    return bool(want) and opt['ws'] is not None


# ----------------------------------------------------------------------------- the three-term forms
@pytest.mark.parametrize('tA,tB', TRANS)
@pytest.mark.parametrize('name', list(CASES))
def test_three_term_forms(request, name, tA, tB):
    """All 12 gemm_bf16x3<TA, TB, VEC, BMT, 3> forms and splitk_reduce2, every epilogue option on each."""
    key = ('x3', name, tA, tB); _RAN.add(key)
    c = CASES[name]; p = _problem(name)
    for opt in OPTS:
        got, _, launched, vec = _run(request, L.gemm_split, p, tA, tB, c['kind'], c['kind'], opt, c['want'], key=key)
        assert vec == (c['kind'] == 'vec')
        form = _x3(tA, tB, vec, c['bmt'][TNAME[(tA, tB)]], 3)
        expect = {form} | ({'splitk_reduce2'} if _reduces(opt, c['want']) else set())
        assert launched == expect, (_label(name, tA, tB, opt), launched, expect)
        ref, scale = _reference(p, opt['bias'], opt['beta'])
        _judge(form, 'x3', got, ref, scale, p['K'], _label(name, tA, tB, opt))


# ----------------------------------------------------------------------------- the single-product forms (mode 2)
@pytest.mark.parametrize('tA,tB', TRANS)
@pytest.mark.parametrize('name', ['V1', 'S1', 'V2', 'S2', 'V3', 'S3'])
def test_single_product_forms(request, name, tA, tB):
    """All 12 gemm_bf16x3<TA, TB, VEC, BMT, 1> forms through the mode-following entry under dep_set_gemm_mode(2, 0): the error sits in the
    single-product bracket -- above the three-term bound (the mode is in effect), below 1e-2 (tails, bias and beta are right)."""
    key = ('x1', name, tA, tB); _RAN.add(key)
    c = CASES[name]; p = _problem(name)
    L.set_gemm_mode(2, 0)
    try:
        for opt in (OPTS[0], OPTS[2]):
            got, _, launched, vec = _run(request, L.gemm_auto, p, tA, tB, c['kind'], c['kind'], opt, c['want'], key=key)
            form = _x3(tA, tB, vec, c['bmt'][TNAME[(tA, tB)]], 1)
            assert launched == {form}, (_label(name, tA, tB, opt), launched, form)
            ref, scale = _reference(p, opt['bias'], opt['beta'])
            _judge(form, 'x1', got, ref, scale, p['K'], _label(name, tA, tB, opt, 'mode2 '))
    finally:
        L.set_gemm_mode(1, 1 << 28)


# ----------------------------------------------------------------------------- the exact forms
@pytest.mark.parametrize('tA,tB', TRANS)
@pytest.mark.parametrize('name', ['V1', 'S1', 'V4', 'S4'])
def test_exact_forms(request, name, tA, tB):
    """All 6 gemm_mfma<TA, TB, VEC> forms; bias and beta through splitk_reduce (V4, S4), the lowered split count and the dropped split."""
    key = ('f32', name, tA, tB); _RAN.add(key)
    c = CASES[name]; p = _problem(name)
    for opt in OPTS:
        got, _, launched, vec = _run(request, L.gemm, p, tA, tB, c['kind'], c['kind'], opt, c['want'], key=key)
        form = _mfma(tA, tB, vec)
        expect = {form} | ({'splitk_reduce'} if _reduces(opt, c['want']) else set())
        assert launched == expect, (_label(name, tA, tB, opt), launched, expect)
        ref, scale = _reference(p, opt['bias'], opt['beta'])
        _judge(form, 'exact', got, ref, scale, p['K'], _label(name, tA, tB, opt, 'exact '))


# ----------------------------------------------------------------------------- scalar and vector loaders: the same bits
@pytest.mark.parametrize('tA,tB', TRANS)
@pytest.mark.parametrize('name', ['V1', 'V4', 'V5'])
def test_scalar_and_vector_loaders_give_the_same_bits(request, name, tA, tB):
    """The arithmetic of a form does not depend on VEC or on the pointer alignment, only the fetch does: the same M, N, K (so the same plan) from
    operands one float into their allocations (and, V1, with ld % 4 != 0) must equal the vector run bit for bit.  beta = 0: the two epilogue branches
    may contract beta * C differently."""
    c = CASES[name]; p = _problem(name)
    opt = dict(bias=True, beta=0.0, ldc='N', coff=0, ws='full')
    bmt = c['bmt'][TNAME[(tA, tB)]]
    for entry, form_of, red, path in ((L.gemm_split, lambda v: _x3(tA, tB, v, bmt, 3), 'splitk_reduce2', 'x3'),
                                      (L.gemm, lambda v: _mfma(tA, tB, v), 'splitk_reduce', 'exact')):
        extra = {red} if c['want'] else set()
        got_v, c_v, launched, vec = _run(request, entry, p, tA, tB, 'vec', 'vec', opt, c['want'])
        assert vec and launched == {form_of(True)} | extra, launched
        ref, scale = _reference(p, True, 0.0)
        _judge(form_of(True), path, got_v, ref, scale, p['K'], _label(name, tA, tB, opt, 'vector loaders '))
        for ka, kb in [('off', 'off')] + ([('ld', 'vec'), ('vec', 'ld')] if name == 'V1' else []):
            got_s, c_s, launched, vec = _run(request, entry, p, tA, tB, ka, kb, opt, c['want'])
            assert not vec and launched == {form_of(False)} | extra, (ka, kb, launched)
            assert torch.equal(c_s, c_v), (name, TNAME[(tA, tB)], ka, kb, np.abs(got_s - got_v).max())


# ----------------------------------------------------------------------------- shifted sequences with scalar loaders
@pytest.mark.parametrize('shift', [-1, 1])
@pytest.mark.parametrize('tform,M,N,kind_a,kind_b', [('TN', 98, 62, 'ld', 'dim'), ('NN', 1030, 62, 'vec', 'off')])
def test_shifted_sequences_with_scalar_loaders(request, tform, M, N, kind_a, kind_b, shift):
    """dW_hh-style B operand (rows shifted one step inside sequences of 300, zero rows at the sequence ends) through the scalar MN-contiguous loader,
    split-K over K = 9 x 300 (chunks of 288, the last 108), against the float64 reference with the zero rows."""
    T, K = 300, 9 * 300
    tA, tB = (1, 0) if tform == 'TN' else (0, 0)
    p = _problem_shift(M, N, K, T, shift)
    opt = dict(bias=False, beta=0.0, ldc='N', coff=0, ws='full')
    bmt = 256 if M >= 512 else 128
    for entry, form, red, path in ((L.gemm_split, _x3(tA, tB, False, bmt, 3), 'splitk_reduce2', 'x3'), (L.gemm, _mfma(tA, tB, False), 'splitk_reduce', 'exact')):
        got, _, launched, vec = _run(request, entry, p, tA, tB, kind_a, kind_b, opt, 10, seq_T=T, shiftB=shift)
        assert not vec and launched == {form, red}, launched
        _judge(form, path, got, p['P'], p['S'], K, '%s %dx%dx%d seq_T=%d shift=%+d' % (tform, M, N, K, T, shift))


# ----------------------------------------------------------------------------- the planning border
# gemm_plan's first test: seq_T <= 0, fewer than 32 tiles of 128 x 128, K <= 8192, M*N*K <= 2^27 -> gemm_small under every entry.
BORDER = [
    (128, 128, 8192, True, False),          # K = 8192 and M*N*K = 2^27 exactly: still small
    (128, 128, 8224, False, True),          # K past 8192: tiled, split-K (32 wanted: chunks of 288 -> 29)
    (132, 128, 8192, False, True),          # 2 tiles, K = 8192, but M*N*K > 2^27
    (31 * 128, 128, 64, True, False),       # 31 tiles
    (32 * 128, 128, 64, False, False),      # 32 tiles: tiled, K < 1024 so unsplit
]


@pytest.mark.parametrize('tA,tB', TRANS)
@pytest.mark.parametrize('M,N,K,small,splits', BORDER)
def test_planning_border(request, M, N, K, small, splits, tA, tB):
    p = _problem_mnk(M, N, K)
    opt = dict(bias=True, beta=0.5, ldc='N', coff=0, ws='full')
    ref, scale = _reference(p, True, 0.5)
    tf = TNAME[(tA, tB)]
    bmt = 256 if M >= 512 and (tf != 'NT' or K >= 512) else 128
    for entry, form, red, path in ((L.gemm, _mfma(tA, tB, True), 'splitk_reduce', 'exact'), (L.gemm_split, _x3(tA, tB, True, bmt, 3), 'splitk_reduce2', 'x3')):
        key = ('border', M, N, K, tA, tB, path); _RAN.add(key)
        got, _, launched, vec = _run(request, entry, p, tA, tB, 'vec', 'vec', opt, 2 if splits else 0, key=key)
        assert vec
        expect = {'gemm_small'} if small else ({form} | ({red} if splits else set()))
        assert launched == expect, (M, N, K, tf, path, launched, expect)
        if small:
            form, path = 'gemm_small', 'exact'          # the exact kernel, whatever the entry
        _judge(form, path, got, ref, scale, K, 'border %dx%dx%d %s %s' % (M, N, K, tf, entry.__name__))


# ----------------------------------------------------------------------------- every form reached
def _expected_keys():
    keys = {('x3', n, a, b) for n in CASES for a, b in TRANS}
    keys |= {('x1', n, a, b) for n in ('V1', 'S1', 'V2', 'S2', 'V3', 'S3') for a, b in TRANS}
    keys |= {('f32', n, a, b) for n in ('V1', 'S1', 'V4', 'S4') for a, b in TRANS}
    keys |= {('border', M, N, K, a, b, path) for M, N, K, _, _ in BORDER for a, b in TRANS for path in ('exact', 'x3')}
    return keys


def test_every_tiled_and_split_form_was_reached():
    """The union of what the cases above launched: all 12 three-term and all 12 single-product gemm_bf16x3 forms, all 6 gemm_mfma forms, both reduce
    kernels and gemm_small.  Needs the whole file to have run."""
    missing = _expected_keys() - _RAN
    if missing:
        pytest.skip('collects what the other tests of this file launched: run the whole file (%d of its cases did not run in this session)' % len(missing))
    seen = set().union(*_SEEN.values())
    want = {_x3(a, b, v, bmt, t) for a, b in TRANS for v in (True, False) for bmt in (128, 256) for t in (3, 1)}
    want |= {_mfma(a, b, v) for a, b in TRANS for v in (True, False)}
    want |= {'splitk_reduce', 'splitk_reduce2', 'gemm_small'}
    for form in sorted(_FIG):
        hi, mean, lo = _FIG[form]
        print('%-44s largest %.3g  smallest %.3g  largest mean %.3g' % (form, hi, lo, mean))
    assert len(want) == 33
    assert want <= seen, sorted(want - seen)
    assert seen <= want, sorted(seen - want)           # and nothing else ran: no LDS-DMA form, no pre-split form
