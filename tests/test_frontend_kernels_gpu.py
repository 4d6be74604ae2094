"""The five front-end kernels (csrc/frontend.hip) called directly through the C ABI at their edges, against float64 references
(tests/frontend_ref.py), and the log-mel / NetVLAD chains end to end where the log-domain bar of tests/test_frontend_gpu.py
cannot reach (tonal and sparse signals, odd n_fft, other frame sizes).

Every input and output is an interior view of a larger tensor this file owns: inputs have 64 floats of NaN on both sides (a stray
read poisons the result and stays inside the allocation), outputs have canary bands that must come back untouched.  Inputs are
float32 values held in float64.  Every bar is fixed by the float formats or by a float32 emulation of the arithmetic
(tests/test_frontend_kernels_cpu.py shows each bar can be met and is sensitive); none comes from the device's output.

Worst values the device gave on the MI355X when these tests were written (each test prints its own with -s):
  dep_frame_window    0.14 of the bar 2^-20 |y[p]| (n_fft 400); 0.03 .. 0.10 elsewhere
  dep_power_spectrum  0.97 ulp of the 1 ulp (7 x 1025); with both squares rounded before the sum it was 1.06 ulp, hence the fmaf
  dep_log_floor       2.15 ulp of the 4 ulp
  dep_row_softmax     0.25 of the bar, row sums 0.15 of theirs (300 x 2); the float32 emulation of an uncompensated z - m misses
                      the bar 6.3x at (127, 2), hence the TwoSum in the kernel
  dep_vlad_normalize  (F, K): device / emulation E_emu / bar 8 E_emu + 8 * 2^-24, relative to max |ref|, worst of the three scales
                      (1, 1) 0 / 0 / 4.8e-7        (3, 2) 1.5e-7 / 4.1e-8 / 8.0e-7      (80, 16) 3.8e-7 / 3.8e-7 / 3.5e-6
                      (80, 1) 1.0e-7 / 4.8e-8 / 8.6e-7   (5, 64) 2.3e-7 / 1.9e-7 / 2.0e-6  (2, 300) 4.6e-7 / 4.1e-7 / 3.7e-6
                      (1000, 16) 5.8e-7 / 6.4e-7 / 5.6e-6; dead cluster 4.2e-7 / 4.2e-7 / 3.9e-6; epsilon cluster 5.3e-7 / 5.3e-7 / 4.7e-6
                      nowhere more than 8 E_emu is needed (the most is 3.6 E_emu, at (3, 2) and scale 1e5); at (1, 1) and (3, 2) the
                      bar's constant term puts it above the serial-sum ceiling (F K / 2 + F / 2 + 8) 2^-24, the device is under both.
                      (1000, 16), 64068 B of LDS, launches.
  log-mel, power domain: device / emulation / bar 8 x emulation (ceiling 2.4e-4)
                      tone 2.0e-6 / 6.8e-7 / 5.4e-6    tone + noise 4.1e-6 / 1.1e-6 / 8.7e-6    click 2.3e-6 / 1.1e-6 / 9.0e-6
  fallback signal     1.2e-6 in the log (bar 1e-5); NetVLAD 3.1e-7 .. 4.6e-7 (bar 1e-5); n_fft 7 / 400: 1.7e-6 / 9.1e-6 in the log (bar 1e-3)
Run on the MI355X box:  python -m pytest tests/test_frontend_kernels_gpu.py -m gpu -q -s
"""
import numpy as np
import pytest

import frontend_ref as FR
from oracle import ref_frontend as RF

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    from icassp2022_depression_amd import audio_features_whole as m
    DEV = torch.device('cuda:0')

F32 = np.float32
SLACK = 64
CANARY = -7.25


class In:
    """A float32 input as an interior view: [64 NaN | values | 64 NaN]."""

    def __init__(self, a):
        a = np.ascontiguousarray(a, dtype=F32).ravel()
        self.n = a.size
        h = np.full(self.n + 2 * SLACK, np.nan, F32)
        h[SLACK:SLACK + self.n] = a
        self.buf = torch.from_numpy(h).to(DEV)
        self.ptr = self.buf[SLACK:].data_ptr()


class Out:
    """An output as an interior view between two canary bands; `init` preloads the interior (in-place calls)."""

    def __init__(self, n, init=None):
        self.n = n
        h = np.full(n + 2 * SLACK, CANARY, F32)
        if init is not None:
            h[SLACK:SLACK + n] = np.ascontiguousarray(init, dtype=F32).ravel()
        self.buf = torch.from_numpy(h).to(DEV)
        self.ptr = self.buf[SLACK:].data_ptr()

    def read(self):
        """The interior as float32, after checking that both bands still hold the canary."""
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert (h[:SLACK] == F32(CANARY)).all() and (h[SLACK + self.n:] == F32(CANARY)).all(), 'canary band overwritten'
        return h[SLACK:SLACK + self.n].copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf.cpu().numpy() == F32(CANARY)).all())


def refused(rc, what, *outs):
    """rc is a refusal: L.check raises DepError, dep_last_error says why, no output was written."""
    assert rc != 0
    with pytest.raises(L.DepError):
        L.check(rc, what)
    assert len(L.load().dep_last_error()) > 0
    for o in outs:
        assert o.untouched()


def worst(err, bar):
    if err.size == 0:
        return 0.0
    err = np.where(np.isfinite(err), err, np.inf)
    return float((err / np.maximum(bar, 1e-300)).max())


# ----------------------------------------------------------------------------- dep_frame_window
def run_frames(y, n_fft, hop, nfr):
    yi, out = In(y), Out(nfr * n_fft)
    L.check(L.load().dep_frame_window(yi.ptr, len(y), n_fft, hop, nfr, out.ptr, L.stream()), 'dep_frame_window')
    return out.read().astype(np.float64).reshape(nfr, n_fft)


@pytest.mark.parametrize('n_fft,hop,n', FR.FRAME_CASES)
def test_frame_window(n_fft, hop, n):
    y = FR.frame_signal(n, n_fft + hop + n)
    ref, absy = FR.ref_frame_window(y, n_fft, hop)
    got = run_frames(y, n_fft, hop, ref.shape[0])
    err, bar = np.abs(got - ref), FR.frame_bar(absy)
    print('frame_window (%d, %d, %d): %d frames, worst err / bar %.3f' % (n_fft, hop, n, ref.shape[0], worst(err, bar)))
    assert (err <= bar).all(), worst(err, bar)


def test_frame_window_fewer_frames_than_fit():
    n_fft, hop, n = 64, 16, 1007
    y = FR.frame_signal(n, n_fft + hop + n)
    ref, absy = FR.ref_frame_window(y, n_fft, hop, n_frames=5)
    got = run_frames(y, n_fft, hop, 5)
    assert (np.abs(got - ref) <= FR.frame_bar(absy)).all()


@pytest.mark.parametrize('n_fft,hop,n,extra', [
    (8, 4, 4, 0),            # n == n_fft / 2: the reflection would need y[n]
    (8, 4, 8, 1),            # one frame more than the padded signal holds
    (7, 4, 8, 1),            # ... for odd n_fft, where the padding is n_fft - 1 samples, not n_fft
    (8, 0, 8, 0),            # hop 0
    (0, 4, 8, 0),            # n_fft 0
])
def test_frame_window_refusals(n_fft, hop, n, extra):
    nfr = (FR.frame_count(n, n_fft, hop) if hop > 0 and n_fft > 0 else 1) + extra
    y, out = In(FR.frame_signal(n, 1)), Out(max(1, nfr * n_fft))
    refused(L.load().dep_frame_window(y.ptr, n, n_fft, hop, nfr, out.ptr, L.stream()), 'dep_frame_window', out)


def test_frame_window_refuses_null_pointers():
    y, out = In(FR.frame_signal(8, 1)), Out(3 * 8)
    lib = L.load()
    refused(lib.dep_frame_window(None, 8, 8, 4, 3, out.ptr, L.stream()), 'dep_frame_window', out)
    refused(lib.dep_frame_window(y.ptr, 8, 8, 4, 3, None, L.stream()), 'dep_frame_window', out)
    refused(lib.dep_frame_window(y.ptr, 8, 8, 4, 0, out.ptr, L.stream()), 'dep_frame_window', out)


# ----------------------------------------------------------------------------- dep_power_spectrum
@pytest.mark.parametrize('rows,bins,ld', FR.POWER_CASES)
def test_power_spectrum(rows, bins, ld):
    reim = FR.power_input(rows, bins, ld, rows + bins)                   # NaN beyond column 2 * bins
    ref = FR.ref_power(reim, bins)
    ri, out = In(reim), Out(rows * bins)
    L.check(L.load().dep_power_spectrum(ri.ptr, rows, bins, ld, out.ptr, L.stream()), 'dep_power_spectrum')
    got = out.read().astype(np.float64).reshape(rows, bins)
    err, bar = np.abs(got - ref), FR.ulp32(ref)
    print('power_spectrum (%d, %d, %d): worst err %.3f ulp' % (rows, bins, ld, worst(err, bar)))
    assert (err <= bar).all(), worst(err, bar)


def test_power_spectrum_refuses_a_short_row():
    ri, out = In(np.ones((2, 9))), Out(2 * 5)
    refused(L.load().dep_power_spectrum(ri.ptr, 2, 5, 9, out.ptr, L.stream()), 'dep_power_spectrum', out)


# ----------------------------------------------------------------------------- dep_log_floor
@pytest.mark.parametrize('n', FR.LOG_SIZES)
def test_log_floor(n):
    x = FR.log_input(n, n)
    ref = FR.ref_log_floor(x)
    xi, out = In(x), Out(n)
    lib = L.load()
    L.check(lib.dep_log_floor(xi.ptr, out.ptr, n, FR.LOG_FLOOR, L.stream()), 'dep_log_floor')
    got32 = out.read()
    inplace = Out(n, init=x)
    L.check(lib.dep_log_floor(inplace.ptr, inplace.ptr, n, FR.LOG_FLOOR, L.stream()), 'dep_log_floor')
    assert np.array_equal(inplace.read().view(np.uint32), got32.view(np.uint32))          # in place: the same bits
    got = got32.astype(np.float64)
    assert np.isnan(ref).any()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), 'a NaN must stay a NaN (np.maximum), nothing else may become one'
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and not np.isneginf(got).any()
    fin = np.isfinite(ref)
    err, bar = np.abs(got[fin] - ref[fin]), 4 * FR.ulp32(ref[fin])
    print('log_floor %d: worst err %.3f ulp' % (n, 4 * worst(err, bar)))
    assert (err <= bar).all(), worst(err, bar)
    below = ~np.isnan(x) & (x <= FR.LOG_FLOOR)                             # 0, -0, negatives, denormals, -inf, the floor itself:
    assert len(set(got32[below].view(np.uint32).tolist())) <= 1            # one value, logf(floor) (within the bar, above)


def test_log_floor_refusals():
    xi, out = In(np.ones(8)), Out(8)
    lib = L.load()
    for n, floor in [(8, 0.0), (8, -1e-6), (0, 1e-6)]:
        refused(lib.dep_log_floor(xi.ptr, out.ptr, n, floor, L.stream()), 'dep_log_floor', out)
    refused(lib.dep_log_floor(xi.ptr, out.ptr, 8, float('nan'), L.stream()), 'dep_log_floor', out)


# ----------------------------------------------------------------------------- dep_row_softmax
@pytest.mark.parametrize('rows,C', FR.SOFTMAX_CASES)
def test_row_softmax(rows, C):
    z, kinds = FR.softmax_input(rows, C, rows + C)
    ref = FR.ref_softmax(z)
    zi, out = In(z), Out(rows * C)
    lib = L.load()
    L.check(lib.dep_row_softmax(zi.ptr, out.ptr, rows, C, L.stream()), 'dep_row_softmax')
    got32 = out.read()
    inplace = Out(rows * C, init=z)
    L.check(lib.dep_row_softmax(inplace.ptr, inplace.ptr, rows, C, L.stream()), 'dep_row_softmax')
    assert np.array_equal(inplace.read().view(np.uint32), got32.view(np.uint32))          # in place: the same bits
    got = got32.astype(np.float64).reshape(rows, C)
    err, bar = np.abs(got - ref), FR.softmax_bar(ref, C)
    sums = np.abs(got.sum(1) - 1.0)
    print('row_softmax (%d, %d): worst err / bar %.3f, worst |sum - 1| / bar %.3f' % (rows, C, worst(err, bar), sums.max() / ((C + 8) * FR.U)))
    assert (err <= bar).all(), worst(err, bar)
    assert (sums <= (C + 8) * FR.U).all()
    for r, kind in enumerate(kinds):
        if kind == 'const':
            assert (np.abs(got[r] - 1.0 / C) <= FR.ulp32(1.0 / C)).all()
        if kind == 'neginf':
            assert (got[r][np.isneginf(z[r])] == 0.0).all()


@pytest.mark.parametrize('C', [0, 65])
def test_row_softmax_refusals(C):
    zi, out = In(np.zeros(3 * 65)), Out(3 * 65)
    refused(L.load().dep_row_softmax(zi.ptr, out.ptr, 3, C, L.stream()), 'dep_row_softmax', out)


# ----------------------------------------------------------------------------- dep_vlad_normalize
def vlad_cases():
    for F, K in FR.VLAD_CASES:
        for scale in FR.VLAD_SCALES:
            yield F, K, scale, None
    for eng in FR.VLAD_ENGINEERED:
        yield 80, 16, 1.0, eng


@pytest.mark.parametrize('F,K,scale,eng', list(vlad_cases()))
def test_vlad_normalize(F, K, scale, eng):
    vkf, a_sum, w2 = FR.vlad_input(F, K, scale, F * K, eng)
    ref = FR.ref_vlad_normalize(vkf, a_sum, w2)
    E_emu = FR.vlad_error(FR.emu_vlad_normalize(vkf, a_sum, w2), ref)
    bar = FR.vlad_bar(E_emu)
    vi, ai, wi, out = In(vkf), In(a_sum), In(w2), Out(F * K)
    L.check(L.load().dep_vlad_normalize(vi.ptr, ai.ptr, wi.ptr, out.ptr, F, K, L.stream()), 'dep_vlad_normalize')
    got = out.read().astype(np.float64)
    E = FR.vlad_error(got, ref)
    print('vlad_normalize (%d, %d) scale %g %s: device %.3g, emulation %.3g, bar %.3g, ceiling %.3g'
          % (F, K, scale, eng, E, E_emu, bar, FR.vlad_ceiling(F, K)))
    assert np.isfinite(got).all()
    assert E <= bar, (E, bar)
    if eng == 'dead_cluster':
        assert (got.reshape(F, K)[:, 3] == 0.0).all()
    if eng == 'all_zero':
        assert not got.any()


@pytest.mark.parametrize('F,K', [(1023, 16), (65536, 65536), (1 << 30, 4)])
def test_vlad_normalize_refuses_what_does_not_fit_lds(F, K):
    """(1023, 16) needs 65540 B.  The other two wrap a 32-bit product: F*K = 2^32 leaves 65537 floats for F = K = 65536 and 5 floats
    for (2^30, 4) (tests/test_frontend_kernels_cpu.py); the check runs in 64 bits and refuses both before anything is launched."""
    assert FR.vlad_lds_bytes(F, K) > FR.VLAD_LDS_LIMIT
    vi, ai, wi, out = In(np.ones(64)), In(np.ones(64)), In(np.ones(64)), Out(64)
    refused(L.load().dep_vlad_normalize(vi.ptr, ai.ptr, wi.ptr, out.ptr, F, K, L.stream()), 'dep_vlad_normalize', out)


# ----------------------------------------------------------------------------- end to end, power domain
@pytest.mark.parametrize('kind', FR.E2E_KINDS)
def test_log_mel_of_narrow_band_signals_in_the_power_domain(kind):
    sr = 16000
    y = FR.e2e_signal(kind, sr)
    mel_ref = np.exp(RF.log_melspectrogram(y, sr, floor=1e-300))
    E_emu = FR.peak_relative_error(FR.emu_log_mel(y, sr), mel_ref)
    got = m.log_melspectrogram(y, sr).cpu().numpy()
    assert got.shape == mel_ref.shape
    E = FR.peak_relative_error(got, mel_ref)
    print('log-mel %s: device %.3g, emulation %.3g, bar %.3g, ceiling %.3g' % (kind, E, E_emu, 8 * E_emu, FR.POWER_DOMAIN_CEILING))
    assert 8 * E_emu <= FR.POWER_DOMAIN_CEILING
    assert E <= 8 * E_emu, (E, E_emu)


def test_log_mel_of_the_empty_file_fallback():
    sr = 16000
    y = FR.e2e_signal('fallback', sr)
    ref = RF.log_melspectrogram(y, sr)
    got = m.log_melspectrogram(y, sr).cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape == (157, 80)
    print('log-mel fallback: worst |log - ref| %.3g' % np.abs(got - ref).max())
    assert np.abs(got - ref).max() <= 1e-5
    assert np.abs(got[3:-3, 0] - (-11.123)).max() < 1e-3
    assert (ref[:, 1:] == np.log(1e-6)).all() and len(np.unique(got[:, 1:])) == 1        # the floor, one value


def test_front_end_does_not_follow_the_gemm_mode():
    """The front-end runs its contractions on dep_gemm_f32 (exact fp32) whatever dep_set_gemm_mode says: bit-identical results."""
    sr = 16000
    y = FR.e2e_signal('tone_noise', sr)
    rng = np.random.default_rng(8)
    x = torch.from_numpy((rng.standard_normal((63, 80)) * 3.0 + 5.0).astype(F32)).to(DEV)
    layer = m.NetVLAD(80, 63, 16, 256, seed=11)
    res = {}
    try:
        for mode in (0, 1):
            L.set_gemm_mode(mode, 0)
            assert L.get_gemm_mode() == mode
            res[mode] = (m.log_melspectrogram(y, sr).cpu().numpy(), layer(x).cpu().numpy())
    finally:
        L.set_gemm_mode(1, 1 << 28)
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('N', [1, 2, 63, 700])
def test_netvlad_frame_counts(N):
    rng = np.random.default_rng(30 + N)
    F, K, D = 80, 16, 256
    x = (rng.standard_normal((N, F)) * 3.0 + 5.0).astype(F32)
    layer = m.NetVLAD(F, N, K, D, seed=11)
    W = {k: v.cpu().numpy().astype(np.float64) for k, v in layer.weights.items()}
    out = layer(torch.from_numpy(x).to(DEV)).cpu().numpy()
    ref = RF.netvlad(x.astype(np.float64), W)
    assert out.shape == (1, D)
    print('NetVLAD N = %d: worst err %.3g' % (N, np.abs(out - ref).max() / max(1.0, np.abs(ref).max())))
    assert np.abs(out - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize('n_fft,hop,n', [(7, 4, 8), (400, 160, 16000 + 37), (400, 160, 16000)])
def test_log_mel_at_other_frame_sizes(n_fft, hop, n):
    """Odd n_fft with n % hop == 0 (one frame fewer than 1 + n // hop) and a frame size that is no power of two, on a broadband
    signal at the bar of tests/test_frontend_gpu.py."""
    sr = 16000
    rng = np.random.default_rng(n_fft + n)
    y = np.round(rng.standard_normal(n) * 3000.0).clip(-32768, 32767)
    ref = RF.log_melspectrogram(y, sr, n_fft=n_fft, hop=hop)
    got = m.log_melspectrogram(y, sr, n_fft=n_fft, hop=hop).cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape == (m.frame_count(n, n_fft, hop), 80)
    assert (ref > np.log(1e-6)).any()
    print('log-mel (%d, %d, %d): worst |log - ref| %.3g' % (n_fft, hop, n, np.abs(got - ref).max()))
    assert np.abs(got - ref).max() < 1e-3, np.abs(got - ref).max()
