"""The error bars of tests/test_frontend_kernels_gpu.py, checked without a GPU (tests/frontend_ref.py holds references, float32
emulations and the case tables):

* every float32 emulation of the device arithmetic stays within its bar against the float64 reference on every case, so a
  correct kernel can meet the bars;
* every bar is sensitive: a deliberately wrong variant (wrong window, padding, origin, sign, missing max shift, wrong layout,
  wrong axis, missing epsilon, dropped NaN) misses it by at least 100x on at least one case;
* the frame count the product requests is numpy's, odd n_fft included, and the kernel's index arithmetic stays inside the
  signal and equals numpy's reflect index at that count;
* the LDS size check of dep_vlad_normalize in 32-bit and in 64-bit arithmetic.
"""
import numpy as np
import pytest

import frontend_ref as FR
from oracle import ref_frontend as RF

F32 = np.float32


def miss(err, bar):
    """How many times the bar is missed: max err / bar (a NaN or inf counts as infinitely wrong)."""
    err = np.where(np.isfinite(err), err, np.inf)
    return float((err / np.maximum(bar, 1e-300)).max())


# ----------------------------------------------------------------------------- frames
@pytest.mark.parametrize('n_fft,hop,n', FR.FRAME_CASES)
def test_frame_emulation_meets_the_bar(n_fft, hop, n):
    y = FR.frame_signal(n, n_fft + hop + n)
    assert len(np.unique(y)) == n and np.array_equal(FR.r32(y), y)
    ref, absy = FR.ref_frame_window(y, n_fft, hop)
    emu = FR.emu_frame_window(y, n_fft, hop).astype(np.float64)
    assert emu.shape == ref.shape == (FR.frame_count(n, n_fft, hop), n_fft)
    assert (np.abs(emu - ref) <= FR.frame_bar(absy)).all(), miss(np.abs(emu - ref), FR.frame_bar(absy))


@pytest.mark.parametrize('wrong', ['symmetric_hann', 'edge_pad', 'origin'])
def test_frame_bar_is_sensitive(wrong):
    worst = 0.0
    for n_fft, hop, n in FR.FRAME_CASES:
        y = FR.frame_signal(n, n_fft + hop + n)
        ref, absy = FR.ref_frame_window(y, n_fft, hop)
        emu = FR.emu_frame_window(y, n_fft, hop, wrong=wrong).astype(np.float64)
        worst = max(worst, miss(np.abs(emu - ref), FR.frame_bar(absy)))
    assert worst >= 100.0, worst


@pytest.mark.parametrize('n_fft,hop,n', FR.FRAME_CASES)
def test_product_frame_count_is_numpys(n_fft, hop, n):
    from icassp2022_depression_amd import audio_features_whole as m
    want = RF.frames_centered(np.zeros(n), n_fft, hop).shape[0]
    assert m.frame_count(n, n_fft, hop) == want == FR.frame_count(n, n_fft, hop)
    if n_fft % 2 == 0:
        assert want == 1 + n // hop                         # the familiar form holds for even n_fft only


def test_one_plus_n_over_hop_overcounts_odd_n_fft():
    """Why frame_count exists: `1 + n // hop` asks for a frame numpy's padding does not have when n_fft is odd and hop divides n,
    and with n = n_fft/2 + 1 that frame would read y[-1] (n_fft 7, hop 4, n 4: frame 1, k 6)."""
    for n_fft, hop, n in [(7, 4, 8), (9, 5, 10), (7, 4, 4)]:
        assert 1 + n // hop == FR.frame_count(n, n_fft, hop) + 1
    p = FR.kernel_source_index(4, 7, 4, 1 + 4 // 4)
    assert p[1, 6] == -1
    assert FR.kernel_source_index(4, 7, 4, FR.frame_count(4, 7, 4)).min() >= 0


@pytest.mark.parametrize('n_fft,hop,n', FR.FRAME_CASES + [(7, 4, 4), (2048, 512, 1025 + 511)])
def test_kernel_index_replay_stays_inside_and_is_numpys_reflect(n_fft, hop, n):
    from icassp2022_depression_amd import audio_features_whole as m
    nfr = m.frame_count(n, n_fft, hop)
    p = FR.kernel_source_index(n, n_fft, hop, nfr)
    assert p.min() >= 0 and p.max() < n
    assert np.array_equal(p, FR.reflect_index(n, n_fft, hop))
    # and the count is the largest the argument check admits: (nfr - 1) * hop + n_fft <= n + 2 * (n_fft / 2) < nfr * hop + n_fft
    assert (nfr - 1) * hop + n_fft <= n + 2 * (n_fft // 2) < nfr * hop + n_fft


# ----------------------------------------------------------------------------- power
@pytest.mark.parametrize('rows,bins,ld', FR.POWER_CASES)
def test_power_emulation_meets_the_bar(rows, bins, ld):
    reim = FR.power_input(rows, bins, ld, rows + bins)
    ref = FR.ref_power(reim, bins)
    assert np.isfinite(ref).all() and np.isnan(reim[:, 2 * bins:]).all()
    emu = FR.emu_power(reim, bins).astype(np.float64)
    assert (np.abs(emu - ref) <= FR.ulp32(ref)).all(), miss(np.abs(emu - ref), FR.ulp32(ref))


def test_power_bar_needs_the_fma():
    """Both squares rounded and then the sum is three roundings, up to 1.25 ulp: over the bar on three of the six cases (1.06 ulp at
    worst), which is why power_kernel spells the fma out and does not leave it to the compiler's contraction."""
    over = []
    for rows, bins, ld in FR.POWER_CASES:
        reim = FR.power_input(rows, bins, ld, rows + bins)
        ref = FR.ref_power(reim, bins)
        over.append(miss(np.abs(FR.emu_power(reim, bins, wrong='three_roundings') - ref), FR.ulp32(ref)))
    assert 1.0 < max(over) <= 1.25, over


def test_power_bar_is_sensitive():
    worst = 0.0
    for rows, bins, ld in FR.POWER_CASES:
        reim = FR.power_input(rows, bins, ld, rows + bins)
        ref = FR.ref_power(reim, bins)
        worst = max(worst, miss(np.abs(FR.emu_power(reim, bins, wrong='minus') - ref), FR.ulp32(ref)))
    assert worst >= 100.0, worst


# ----------------------------------------------------------------------------- log
@pytest.mark.parametrize('n', FR.LOG_SIZES)
def test_log_floor_emulation_meets_the_bar(n):
    x = FR.log_input(n, n)
    ref = FR.ref_log_floor(x)
    emu = FR.emu_log_floor(x).astype(np.float64)
    assert np.array_equal(np.isnan(emu), np.isnan(ref)) and np.isnan(ref).any()
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isposinf(emu), np.isposinf(ref))
    fin = ok & np.isfinite(ref)
    assert (np.abs(emu[fin] - ref[fin]) <= 4 * FR.ulp32(ref[fin])).all()
    below = ok & (x < FR.LOG_FLOOR)
    assert (ref[below] == np.log(FR.LOG_FLOOR)).all()


def test_log_floor_bar_sees_a_dropped_nan():
    x = FR.log_input(1027, 1027)
    ref = FR.ref_log_floor(x)
    emu = FR.emu_log_floor(x, wrong='fmax').astype(np.float64)
    assert np.isnan(ref).sum() == 2 and not np.isnan(emu).any()          # fmax(floor, NaN) = floor: the NaN is gone
    assert (emu[np.isnan(ref)] == np.log(FR.LOG_FLOOR).astype(F32)).all()


# ----------------------------------------------------------------------------- softmax
@pytest.mark.parametrize('rows,C', FR.SOFTMAX_CASES)
def test_softmax_emulation_meets_the_bar(rows, C):
    z, kinds = FR.softmax_input(rows, C, rows + C)
    ref = FR.ref_softmax(z)
    emu = FR.emu_softmax(z).astype(np.float64)
    err, bar = np.abs(emu - ref), FR.softmax_bar(ref, C)
    print('softmax emulation (%d, %d): worst err / bar %.3f' % (rows, C, miss(err, bar)))
    assert (err <= bar).all(), miss(err, bar)
    assert (np.abs(emu.sum(1) - 1.0) <= (C + 8) * FR.U).all()
    for r, kind in enumerate(kinds):
        if kind == 'const':
            assert (np.abs(emu[r] - 1.0 / C) <= FR.ulp32(1.0 / C)).all()
        if kind == 'neginf':
            assert (emu[r][np.isneginf(z[r])] == 0.0).all() and np.isneginf(z[r]).sum() == 1


def test_softmax_cases_reach_every_kind():
    seen = set()
    for rows, C in FR.SOFTMAX_CASES:
        seen.update(FR.softmax_input(rows, C, rows + C)[1])
    assert seen == set(FR.SOFTMAX_KINDS)
    assert {r for r, _ in FR.SOFTMAX_CASES} == {1, 127, 128, 129, 300} and {c for _, c in FR.SOFTMAX_CASES} == {1, 2, 16, 63, 64}


def test_softmax_bar_is_sensitive():
    """Without the max shift the rows at +80000 overflow (inf / inf) and the rows at -80000 underflow (0 / 0)."""
    worst = 0.0
    for rows, C in FR.SOFTMAX_CASES:
        z, kinds = FR.softmax_input(rows, C, rows + C)
        big = [r for r, k in enumerate(kinds) if k in ('big+', 'big-', 'mixed', 'n1e4')]
        if big:
            ref = FR.ref_softmax(z[big])
            worst = max(worst, miss(np.abs(FR.emu_softmax(z[big], wrong='no_shift') - ref), FR.softmax_bar(ref, C)))
    assert worst >= 100.0, worst


def test_softmax_bar_needs_the_exact_shift():
    """A float32 z - m rounds by up to 2^-24 |z - m|, and that is the relative error of the exponential: on the logits scaled by 30
    a probability of 1e-29 is then off by several times the bar.  This is why row_softmax_kernel compensates the subtraction."""
    rows, C = 127, 2
    z, _ = FR.softmax_input(rows, C, rows + C)
    ref = FR.ref_softmax(z)
    m_plain = miss(np.abs(FR.emu_softmax(z, wrong='rounded_shift') - ref), FR.softmax_bar(ref, C))
    assert 1.0 < m_plain < 100.0, m_plain


# ----------------------------------------------------------------------------- NetVLAD tail
def vlad_cases():
    for F, K in FR.VLAD_CASES:
        for scale in FR.VLAD_SCALES:
            yield F, K, scale, None
    for eng in FR.VLAD_ENGINEERED:
        yield 80, 16, 1.0, eng


@pytest.mark.parametrize('F,K,scale,eng', list(vlad_cases()))
def test_vlad_emulation_is_inside_the_ceiling(F, K, scale, eng):
    """The bar of the GPU test is 8 E_emu + 8 * 2^-24: E_emu itself must be finite, small, and the bar below the worst-case bound
    of the serial sums wherever that bound is the larger statement (from F*K = 160 on)."""
    vkf, a_sum, w2 = FR.vlad_input(F, K, scale, F * K, eng)
    ref = FR.ref_vlad_normalize(vkf, a_sum, w2)
    emu = FR.emu_vlad_normalize(vkf, a_sum, w2)
    assert np.isfinite(ref).all() and np.isfinite(emu).all()
    E = FR.vlad_error(emu, ref)
    print('vlad emulation (%d, %d) scale %g %s: E_emu %.3g' % (F, K, scale, eng, E))
    assert E <= FR.vlad_ceiling(F, K)
    assert E <= 2e-6
    if F * K >= 160:
        assert FR.vlad_bar(E) <= FR.vlad_ceiling(F, K)
    if eng == 'dead_cluster':
        assert (ref.reshape(F, K)[:, 3] == 0).all() and (emu.reshape(F, K)[:, 3] == 0).all()
    if eng == 'epsilon_cluster':                            # scaled by 1e6 (then globally), not normalised to 1
        col = ref.reshape(F, K)[:, 5] / np.sqrt(1.0 / (K - 1 + (vkf[5] ** 2).sum() * 1e12))
        assert np.allclose(col, vkf[5] * 1e6, rtol=1e-9, atol=0) and 0 < (vkf[5] ** 2).sum() < 1e-12
    if eng == 'all_zero':
        assert not ref.any() and not emu.any()


@pytest.mark.parametrize('wrong', ['index', 'axis', 'no_eps'])
def test_vlad_bar_is_sensitive(wrong):
    worst = 0.0
    for F, K, scale, eng in vlad_cases():
        vkf, a_sum, w2 = FR.vlad_input(F, K, scale, F * K, eng)
        ref = FR.ref_vlad_normalize(vkf, a_sum, w2)
        bar = FR.vlad_bar(FR.vlad_error(FR.emu_vlad_normalize(vkf, a_sum, w2), ref))
        got = FR.vlad_error(FR.emu_vlad_normalize(vkf, a_sum, w2, wrong=wrong), ref)
        worst = max(worst, got / bar)
    assert worst >= 100.0, worst


def test_vlad_lds_check_needs_64_bits():
    """The size check of dep_vlad_normalize: (F*K + K + 1) * 4 bytes <= 64 KiB.  Done in `int`, F*K wraps: F = K = 65536 leaves 65537
    floats (refused only by luck), F = 2^30 with K = 4 leaves 5 floats and would pass.  In 64 bits both are refused, and the
    table's cases are on the side the issue names."""
    def admitted_i32(F, K):
        return FR.wrap_i32(FR.wrap_i32(F * K) + K + 1) * 4 <= FR.VLAD_LDS_LIMIT
    assert FR.wrap_i32(65536 * 65536) == 0 and not admitted_i32(65536, 65536)
    assert admitted_i32(1 << 30, 4)                                            # the defect
    for F, K in [(65536, 65536), (1 << 30, 4), (1023, 16)]:
        assert FR.vlad_lds_bytes(F, K) > FR.VLAD_LDS_LIMIT
    assert FR.vlad_lds_bytes(1023, 16) == 65540 and FR.vlad_lds_bytes(1000, 16) == 64068
    for F, K in FR.VLAD_CASES:
        assert FR.vlad_lds_bytes(F, K) <= FR.VLAD_LDS_LIMIT


# ----------------------------------------------------------------------------- the log-mel chain
@pytest.fixture(scope='module')
def mel_refs():
    """kind -> (float64 mel power with a vanishing floor, float32 emulation of the log-mel), computed once."""
    out = {}
    for kind in FR.E2E_KINDS:
        y = FR.e2e_signal(kind)
        out[kind] = (np.exp(RF.log_melspectrogram(y, 16000, floor=1e-300)), FR.emu_log_mel(y, 16000))
    return out


@pytest.mark.parametrize('kind', FR.E2E_KINDS)
def test_log_mel_emulation_in_the_power_domain(kind, mel_refs):
    mel_ref, emu = mel_refs[kind]
    assert emu.dtype == F32 and emu.shape == mel_ref.shape == (32, 80)
    E = FR.peak_relative_error(emu, mel_ref)
    print('log-mel emulation, %s: peak-relative error %.3g' % (kind, E))
    assert 8 * E <= FR.POWER_DOMAIN_CEILING
    # the log-domain bar of tests/test_frontend_gpu.py cannot be asked of these signals: between the partials the float32 chain
    # holds rounding noise of the peak
    if kind == 'tone':
        assert np.abs(emu - np.log(np.maximum(1e-6, mel_ref))).max() > 1.0


def test_fallback_signal_is_one_band_over_the_floor():
    y = FR.e2e_signal('fallback')
    ref = RF.log_melspectrogram(y, 16000)
    emu = FR.emu_log_mel(y, 16000).astype(np.float64)
    assert ref.shape == emu.shape == (157, 80)
    inner = ref[3:-3]                                       # frames clear of the reflect padding see a constant
    assert np.abs(inner[:, 0] - (-11.123)).max() < 1e-3
    assert (ref[:, 1:] == np.log(1e-6)).all()
    assert np.abs(emu - ref).max() <= 1e-5
