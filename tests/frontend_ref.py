"""References, float32 emulations and case tables for the five front-end kernels of csrc/frontend.hip (dep_frame_window,
dep_power_spectrum, dep_log_floor, dep_row_softmax, dep_vlad_normalize).  CPU only, numpy only: this file does not import the
library, so tests/test_frontend_kernels_cpu.py and tests/test_frontend_kernels_gpu.py walk the same cases against the same
numbers.

* ref_*  : float64, one per kernel, restated here (the end-to-end tests use oracle/ref_frontend.py itself).
* emu_*  : the device's arithmetic in numpy float32 (every operation rounded once, sums serial in the kernel's order).  They
           exist to DERIVE error bars and to show that a correct float32 implementation meets the bars; the `wrong=` switches
           turn them into the deliberately wrong variants the sensitivity tests need.
* *_CASES: the shapes.

Inputs are float32 values held in float64 (`r32`), so reference and kernel see the same numbers.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                       # unit roundoff of float32


def r32(a):
    """float64 holding float32 values: what the kernel is given."""
    return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def ulp32(a):
    """Spacing of float32 at |a| (a float64 array of reference values)."""
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(F32)).astype(np.float64)


# ----------------------------------------------------------------------------- case tables
# (n_fft, hop, n)
FRAME_CASES = [
    (8, 2, 5),               # minimum legal n (n_fft/2 + 1)
    (8, 4, 5),
    (16, 4, 9),
    (16, 24, 100),           # hop > n_fft
    (64, 1, 40),             # hop 1
    (64, 16, 1007),
    (7, 4, 5),               # odd n_fft
    (7, 4, 8),               # odd n_fft, n % hop == 0
    (9, 5, 10),              # odd n_fft, n % hop == 0
    (400, 160, 1763),        # not a power of two
    (2048, 512, 1025),
    (2048, 512, 2048 + 37),
    (2048, 512, 4096),       # n % hop == 0
]
# (rows, bins, ld)
POWER_CASES = [(1, 1, 2), (3, 5, 13), (1, 256, 512), (1, 257, 520), (7, 1025, 2050), (33, 9, 18)]
LOG_SIZES = [1, 255, 256, 257, 1027]
LOG_FLOOR = float(F32(1e-6))         # the floor the kernel receives (a float argument)
# (rows, C): every value of rows {1, 127, 128, 129, 300} and of C {1, 2, 16, 63, 64} at least once
SOFTMAX_CASES = [(1, 1), (1, 64), (127, 2), (128, 16), (129, 63), (300, 64), (300, 1), (129, 16), (300, 2)]
# (F, K)
VLAD_CASES = [(1, 1), (3, 2), (80, 16), (80, 1), (5, 64), (2, 300), (1000, 16)]
VLAD_SCALES = [1e-3, 1.0, 1e5]
VLAD_ENGINEERED = ['dead_cluster', 'epsilon_cluster', 'all_zero']        # at (80, 16)
VLAD_LDS_LIMIT = 64 * 1024


# ----------------------------------------------------------------------------- framing and window
def frame_count(n, n_fft, hop):
    """Frames numpy's reflect padding yields: len(np.pad(y, n_fft // 2)) = n + 2 * (n_fft // 2)."""
    return 1 + (n + 2 * (n_fft // 2) - n_fft) // hop


def frame_signal(n, seed):
    """A seeded permutation of n distinct integers centred on 0: exact in float32, neighbours differ by at least 1, so a wrong
    index moves a value by at least the window weight.  |y| <= 1000 up to n = 2001; the three longer rows of the table cannot
    hold distinct integers inside +-1000 and run to +-n/2 (still exact, and the bar is relative to |y[p]|)."""
    rng = np.random.default_rng(seed)
    return rng.permutation(np.arange(n) - n // 2).astype(np.float64)


def reflect_index(n, n_fft, hop, n_frames=None):
    """(n_frames, n_fft) source index of every frame element: numpy's own reflect padding applied to arange(n)."""
    pad = np.pad(np.arange(n), n_fft // 2, mode='reflect')
    n_frames = 1 + (len(pad) - n_fft) // hop if n_frames is None else n_frames
    return pad[np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]]


def ref_frame_window(y, n_fft, hop, n_frames=None):
    """float64: reflect-padded y framed at hop, times the periodic Hann window.  Returns (frames, |y[p]|)."""
    y = np.asarray(y, np.float64)
    src = y[reflect_index(len(y), n_fft, hop, n_frames)]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    return src * w[None, :], np.abs(src)


def frame_bar(absy):
    """|out - ref| <= 2^-20 |y[p]|: the float32 window (cospif of a rounded quotient: |dw| <= pi 2^-24 + 2^-25 < 2^-22) and one
    product rounding (2^-24)."""
    return 2.0 ** -20 * absy


def kernel_source_index(n, n_fft, hop, n_frames):
    """frame_window_kernel's index arithmetic replayed: p = i*hop + k - n_fft/2, one reflection on each side.  Not clipped: an
    index outside [0, n) is returned as it is."""
    p = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
    p = np.where(p < 0, -p, p)
    return np.where(p >= n, 2 * (n - 1) - p, p)


def emu_window(n_fft, wrong=None):
    """The kernel's window in float32: 0.5f - 0.5f * cospif(2.0f * k / n_fft)."""
    den = n_fft - 1 if wrong == 'symmetric_hann' else n_fft
    x = (F32(2.0) * np.arange(n_fft, dtype=F32)) / F32(den)
    c = np.cos(np.pi * x.astype(np.float64)).astype(F32)
    return F32(0.5) - F32(0.5) * c


def emu_frame_window(y, n_fft, hop, n_frames=None, wrong=None):
    """float32 emulation of dep_frame_window.  wrong: None | 'symmetric_hann' | 'edge_pad' | 'origin'."""
    y = np.asarray(y, F32)
    n = len(y)
    n_frames = frame_count(n, n_fft, hop) if n_frames is None else n_frames
    if wrong == 'edge_pad':
        pad = np.pad(np.arange(n), n_fft // 2, mode='symmetric')
        p = pad[np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]]
    else:
        p = kernel_source_index(n, n_fft, hop, n_frames)
        if wrong == 'origin':
            p = np.clip(p + 1, 0, n - 1)
    return y[p] * emu_window(n_fft, wrong)[None, :]


# ----------------------------------------------------------------------------- power
def power_input(rows, bins, ld, seed):
    """(rows, ld): [re | im] normal values over a few decades; the padding columns hold NaN (they must never be read)."""
    rng = np.random.default_rng(seed)
    a = np.full((rows, ld), np.nan)
    a[:, :2 * bins] = r32(rng.standard_normal((rows, 2 * bins)) * 10.0 ** rng.integers(-3, 4, (rows, 2 * bins)))
    return a


def ref_power(reim, bins):
    return reim[:, :bins] ** 2 + reim[:, bins:2 * bins] ** 2


def emu_power(reim, bins, wrong=None):
    """float32 fmaf(re, re, im * im): a rounded im^2, then one rounding of the sum (the exact re^2 of two float32 fits a float64).
    Half an ulp of im^2 <= result and half an ulp of the result: within 1 ulp.  wrong='three_roundings' is re*re + im*im with
    both squares rounded (up to 1.25 ulp: 1.06 on these cases), wrong='minus' is re^2 - im^2."""
    re, im = reim[:, :bins].astype(F32), reim[:, bins:2 * bins].astype(F32)
    if wrong == 'three_roundings':
        return re * re + im * im
    im2 = (im * im).astype(np.float64)
    re2 = re.astype(np.float64) ** 2
    return (re2 - im2 if wrong == 'minus' else re2 + im2).astype(F32)


# ----------------------------------------------------------------------------- log with a floor
def log_input(n, seed):
    """Positive values over twenty decades with the special values the contract names at the front (as many as fit)."""
    rng = np.random.default_rng(seed)
    fl = F32(LOG_FLOOR)
    special = np.array([np.nan, fl, np.nextafter(fl, F32(0)), np.nextafter(fl, F32(1)), 0.0, -0.0, -1.0, -1e30, 1e-42, -1e-42,
                        1.17549435e-38, 1e30, np.inf, -np.inf, 1e-7, 3.0e-6], dtype=F32)
    x = (10.0 ** rng.uniform(-8, 12, n)).astype(F32)
    if n >= len(special):
        x[:len(special)] = special
        x[-1] = np.nan                                      # the last element of the last block too
    else:
        x[0] = np.nan if seed % 2 else np.inf
    return x.astype(np.float64)


def ref_log_floor(x, floor=LOG_FLOOR):
    with np.errstate(invalid='ignore'):
        return np.log(np.maximum(floor, x))


def emu_log_floor(x, floor=LOG_FLOOR, wrong=None):
    x = np.asarray(x, F32)
    m = np.fmax(F32(floor), x) if wrong == 'fmax' else np.where(x < F32(floor), F32(floor), x)
    return np.log(m.astype(np.float64)).astype(F32)


# ----------------------------------------------------------------------------- row softmax
SOFTMAX_KINDS = ['n1', 'n30', 'n1e4', 'const', 'neginf', 'big+', 'big-', 'mixed']


def softmax_input(rows, C, seed):
    """Row r is of kind SOFTMAX_KINDS[(r + seed) % 8]: normal logits scaled by 1, 30 and 1e4, a constant row, a row with one
    -inf entry (not at C = 1: the row would be empty), rows around +80000 and -80000 and a row of +-80000 entries.
    Returns (z, kinds)."""
    rng = np.random.default_rng(seed)
    z = np.empty((rows, C))
    kinds = []
    for r in range(rows):
        kind = SOFTMAX_KINDS[(r + seed) % len(SOFTMAX_KINDS)]
        g = rng.standard_normal(C)
        if kind == 'neginf' and C == 1:
            kind = 'n1'
        if kind in ('n1', 'n30', 'n1e4'):
            z[r] = g * {'n1': 1.0, 'n30': 30.0, 'n1e4': 1e4}[kind]
        elif kind == 'const':
            z[r] = g[0] * 100.0
        elif kind == 'neginf':
            z[r] = g
            z[r, rng.integers(C)] = -np.inf
        elif kind == 'big+':
            z[r] = 80000.0 + g
        elif kind == 'big-':
            z[r] = -80000.0 + g
        else:
            z[r] = np.where(rng.random(C) < 0.5, 80000.0, -80000.0)
        kinds.append(kind)
    return r32(z), kinds


def ref_softmax(z):
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def softmax_bar(ref, C):
    """expf (a few ulp), a C-term serial sum and the reciprocal: (C + 8) 2^-24 relative, and nothing below 1e-37 is asked for."""
    return (C + 8) * U * ref + 1e-37


def emu_softmax(z, wrong=None):
    """float32: max, expf of the shifted logit, serial sum, one reciprocal.  The kernel recovers the rounding error of z - m
    (TwoSum) and folds it into the exponential, so the shift is exact here (float32 operands subtract exactly in float64).
    wrong='rounded_shift' is the plain expf(z - m): its 2^-24 |z - m| in the exponent alone misses the bar near the underflow
    end (by 6x at C = 2).  wrong='no_shift' leaves the maximum out."""
    z = np.asarray(z, F32)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        if wrong == 'no_shift':
            d = z.astype(np.float64)
        elif wrong == 'rounded_shift':
            d = (z - z.max(1, keepdims=True)).astype(np.float64)
        else:
            d = z.astype(np.float64) - z.max(1, keepdims=True).astype(np.float64)
        e = np.exp(d).astype(F32)
        s = np.cumsum(e, axis=1, dtype=F32)[:, -1:]
        return e * (F32(1.0) / s)


# ----------------------------------------------------------------------------- NetVLAD tail
def vlad_input(F, K, scale, seed, engineered=None):
    """vkf (K, F), a_sum (K,), w2 (F, K): seeded, no engineered cancellation; `engineered` plants the rows of the (80, 16) cases."""
    rng = np.random.default_rng(seed)
    vkf = rng.standard_normal((K, F)) * scale
    a_sum = rng.uniform(0.5, 4.0, K)
    w2 = rng.standard_normal((F, K)) * scale / np.sqrt(F)
    if engineered == 'dead_cluster':                          # nothing assigned to cluster 3: v = 0 - 0 * w2
        a_sum[3] = 0.0
        vkf[3] = 0.0
    elif engineered == 'epsilon_cluster':                     # residual norm of cluster 5 ~ 1e-7 < 1e-6: x * 1e6, not x / |x|
        a_sum[5] = 0.0
        vkf[5] = rng.standard_normal(F) * 1e-8
    elif engineered == 'all_zero':
        vkf[:] = 0.0
        a_sum[:] = 0.0
        w2[:] = 0.0
    return r32(vkf), r32(a_sum), r32(w2)


def ref_vlad_normalize(vkf, a_sum, w2):
    """float64: the lines of oracle.ref_frontend.netvlad from `a = ...` to the global normalisation -> (F*K,), index f*K + k."""
    a = a_sum[None, :] * w2
    vlad = vkf.T - a
    vlad = vlad / np.sqrt(np.maximum((vlad ** 2).sum(0, keepdims=True), 1e-12))
    flat = vlad.reshape(-1)
    return flat / np.sqrt(np.maximum((flat ** 2).sum(), 1e-12))


def emu_vlad_normalize(vkf, a_sum, w2, wrong=None):
    """float32 with serial sums in vlad_normalize_kernel's order (cluster norms over f, the total over f*K + k).
    wrong: None | 'index' (vkf read as (F, K)) | 'axis' (intra normalisation over k) | 'no_eps'."""
    vkf, a_sum, w2 = np.asarray(vkf, F32), np.asarray(a_sum, F32), np.asarray(w2, F32)
    K, F = vkf.shape
    eps = F32(0.0) if wrong == 'no_eps' else F32(1e-12)
    vt = vkf.reshape(-1)[:F * K].reshape(F, K) if wrong == 'index' else vkf.T
    with np.errstate(divide='ignore', invalid='ignore'):
        v = vt - a_sum[None, :] * w2
        if wrong == 'axis':
            s = np.cumsum(v * v, axis=1, dtype=F32)[:, -1:]
        else:
            s = np.cumsum(v * v, axis=0, dtype=F32)[-1:, :]
        v = v * (F32(1.0) / np.sqrt(np.maximum(s, eps)))
        flat = v.reshape(-1)
        tot = np.cumsum(flat * flat, dtype=F32)[-1]
        return flat * (F32(1.0) / np.sqrt(np.maximum(tot, eps)))


def vlad_error(got, ref):
    """max |got - ref| relative to max |ref| (inf for a non-finite result).  An all-zero reference asks for exact zeros."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    top = np.abs(ref).max()
    if top == 0.0:
        return 0.0 if not got.any() else np.inf
    return np.abs(got - ref).max() / top


def vlad_bar(E_emu):
    """8 x the serial float32 emulation's own error (rsqrtf and fma contraction are not in it) + 8 x 2^-24."""
    return 8.0 * E_emu + 8.0 * U


def vlad_ceiling(F, K):
    """Worst-case bound of the two serial sums: (F*K/2 + F/2 + 8) 2^-24."""
    return (F * K / 2.0 + F / 2.0 + 8.0) * U


def vlad_lds_bytes(F, K):
    return (F * K + K + 1) * 4


def wrap_i32(v):
    """Two's-complement wrap of a Python int to 32 bits: what `int` arithmetic leaves on the device's host compiler."""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


# ----------------------------------------------------------------------------- the log-mel chain
def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + 27.0 * np.log(np.maximum(f, 1e-30) / 1000.0) / np.log(6.4), 3.0 * f / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)), 200.0 * m / 3.0)


def mel_table(sr, n_fft, n_mels):
    """Slaney-normalised triangles (n_mels, 1 + n_fft // 2), float64."""
    freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    lo, ce, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    tri = np.maximum(0.0, np.minimum((freqs[None, :] - lo) / (ce - lo), (hi - freqs[None, :]) / (hi - ce)))
    return tri * (2.0 / (hi - lo))


def emu_log_mel(y, sr, n_fft=2048, hop=512, n_mels=80, floor=1e-6):
    """The device's chain in float32: float32 frames, the float32 [cos | -sin] basis and mel table (float64 tables rounded
    once, as the host code builds them), float32 matmuls, re^2 + im^2, log(max(floor, .)).  -> (frames, n_mels) float32."""
    bins = 1 + n_fft // 2
    fr = emu_frame_window(np.asarray(y, F32), n_fft, hop)
    ang = 2.0 * np.pi * np.outer(np.arange(n_fft), np.arange(bins)) / n_fft
    basis = np.concatenate([np.cos(ang), -np.sin(ang)], 1).astype(F32)
    melw = mel_table(sr, n_fft, n_mels).astype(F32)
    reim = fr @ basis
    power = emu_power(reim, bins)
    mel = power @ melw.T
    return emu_log_floor(mel, F32(floor))


def peak_relative_error(log_got, mel_ref):
    """max |exp(log_got) - mel_ref| / (the frame's peak mel_ref): the power-domain measure for narrow-band signals, where the
    bands between the partials hold rounding noise of the peak and the log has no meaning.  mel_ref is the oracle with a
    vanishing floor.  A frame with nothing above the product's floor (the silence around a click) has no peak to measure
    against: there every band must be the floor itself, log(1e-6) to 4 float32 ulp, or the result is inf."""
    log_got = np.asarray(log_got, np.float64)
    loud = mel_ref.max(1) > LOG_FLOOR
    if not loud.any() or (np.abs(log_got[~loud] - np.log(LOG_FLOOR)) > 4 * ulp32(np.log(LOG_FLOOR))).any():
        return np.inf
    return (np.abs(np.exp(log_got[loud]) - mel_ref[loud]) / mel_ref[loud].max(1, keepdims=True)).max()


POWER_DOMAIN_CEILING = 2 * 2048 * U        # worst case of a 2048-term float32 dot product, squared


def e2e_signal(kind, sr=16000):
    """The end-to-end signals: 1 s at `sr`, int16-like scale."""
    t = np.arange(sr) / sr
    rng = np.random.default_rng(17)
    if kind == 'tone':
        return r32(10000.0 * np.sin(2 * np.pi * 1000.0 * t))
    if kind == 'tone_noise':
        return r32(10000.0 * np.sin(2 * np.pi * 1000.0 * t) + rng.standard_normal(sr))
    if kind == 'click':
        y = np.zeros(sr)
        y[sr // 2 + 13] = 20000.0
        return y
    if kind == 'fallback':                  # what extract_features substitutes for an empty file
        return r32(np.array([1e-4] * sr * 5))
    raise ValueError(kind)


E2E_KINDS = ['tone', 'tone_noise', 'click']
