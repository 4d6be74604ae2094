"""Reference, tile geometry and case lists of the attention parity tests (tests/test_attention_forms_gpu.py, tests/test_attention_ref_cpu.py).

attention_from_pre() is oracle/ref_numpy.py's attention_fwd / attention_bwd behind the projection: it takes `pre` as an INPUT, so a test can hand it
the pre-activations the device computed.  relu(pre) and the mask pre > 0 are then the same numbers on both sides and the attention kernels are judged
alone; the projection (hsum, pre, dWa, dba, dh_n) is judged separately against its own float64 products.
"""
import zlib

import numpy as np

from varlen_ref import lengths_mix

AT, AU = 512, 4                                     # attention.hip: threads per workgroup, rows in flight per thread
LDS_MAX = 160 * 1024


def rows_per_pass(H):
    """R of attn_{fwd,bwd}2_kernel: 8 waves x 64 / (H / 4) rows.  H = 64: 32, 128: 16, 256: 8; a loop trip covers R * AU rows."""
    return (AT // 64) * (64 // (H // 4))


# ----------------------------------------------------------------------------- reference
def attention_from_pre(out, pre, dctx, lengths=None, dtype=np.float64):
    """out (B, T, 2H), pre (B, H), dctx (B, H) -> ctx (B, H), alpha (B, T), dout (B, T, 2H), dpre (B, H), all computed in `dtype`.
    q = max(pre, 0), mask pre > 0; the formulas of R.attention_fwd / R.attention_bwd.  With `lengths` row b is the dense result of its first
    lengths[b] steps alone, alpha and dout are 0 behind them, an empty row gives ctx = 0 and no gradient (out behind a length is never read)."""
    B, T, H2 = out.shape
    H = H2 // 2
    pre = np.asarray(pre, dtype=dtype); dctx = np.asarray(dctx, dtype=dtype)
    ctx = np.zeros((B, H), dtype); alpha = np.zeros((B, T), dtype); dout = np.zeros((B, T, H2), dtype); dpre = np.zeros((B, H), dtype)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        if n == 0:
            continue
        o = np.asarray(out[b, :n], dtype=dtype)
        h = o[:, :H] + o[:, H:]
        q = np.maximum(pre[b], dtype(0.0))
        m = np.tanh(h)
        sc = np.einsum('j,tj->t', q, m)
        e = np.exp(sc - sc.max())
        al = e / e.sum()
        ctx[b] = np.einsum('t,tj->j', al, h)
        alpha[b, :n] = al
        dal = np.einsum('j,tj->t', dctx[b], h)
        dsc = al * (dal - (al * dal).sum())
        dq = np.einsum('t,tj->j', dsc, m)
        dh = al[:, None] * dctx[b][None, :] + dsc[:, None] * q[None, :] * (1 - m * m)
        dout[b, :n, :H] = dh; dout[b, :n, H:] = dh
        dpre[b] = dq * (pre[b] > 0)
    return ctx, alpha, dout, dpre


def dpre_condition(c, pre):
    """What ONE float32 rounding of dot = sum_t alpha_t dalpha_t does to dpre, relative to dpre's largest element: dsc_t = alpha_t (dalpha_t - dot), so
    an error e in dot moves dq_j by e sum_t alpha_t m_tj, and e is half an ulp of sum_t |alpha_t dalpha_t|.  When the softmax is nearly one-hot
    dalpha_t* - dot cancels and this grows like 1 / (1 - alpha.max()): no float32 summation order is then held to a bound near it."""
    H = c['H']
    ref = attention_from_pre(c['out_in'], pre, c['dctx'], c['lengths'])
    worst = 0.0
    for b in range(c['B']):
        n = c['T'] if c['lengths'] is None else int(c['lengths'][b])
        if n == 0:
            continue
        o = c['out'][b, :n].astype(np.float64)
        h = o[:, :H] + o[:, H:]
        al = ref[1][b, :n]
        e = 2.0 ** -24 * np.abs(al * (h @ c['dctx'][b].astype(np.float64))).sum()
        worst = max(worst, e * np.abs((al[:, None] * np.tanh(h)).sum(0) * (np.asarray(pre[b]) > 0)).max())
    return float(worst / max(np.abs(ref[3]).max(), 1e-300))


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def deviations(got, ref):
    """The four figures a result is judged by: ctx and alpha as largest absolute difference, dout and dpre relative to the reference's largest element."""
    return dict(ctx=float(np.abs(got[0] - ref[0]).max()), alpha=float(np.abs(got[1] - ref[1]).max()), dout=relerr(got[2], ref[2]), dpre=relerr(got[3], ref[3]))


def hsum_f32(hn):
    """sum over k of hn (K, B, H) in float32, in order -- what attn_hsum_kernel computes, bit for bit."""
    s = np.zeros(hn.shape[1:], np.float32)
    for k in range(hn.shape[0]):
        s = s + hn[k].astype(np.float32)
    return s


def is_flat(alpha, lengths=None):
    """Every step carries weight: each row's weights lie within a factor 8 of uniform -- the lightest of 630 steps still moves ctx by 1e-4, twenty
    times the flat bound -- and no step of a row of 80 or more steps holds 5 % (the 1 / n of a shorter row is above that whatever the scores are: a
    one-step row has alpha = 1)."""
    for b in range(alpha.shape[0]):
        n = alpha.shape[1] if lengths is None else int(lengths[b])
        if n == 0:
            continue
        a = alpha[b, :n]
        if not (a.max() * n < 8.0 and a.min() * n > 0.125 and (n < 80 or a.max() < 0.05)):
            return False
    return True


# ----------------------------------------------------------------------------- inputs
SCALES = ('flat', 'unit', 'sat', 'zeros')
RAGGED_B = 4                                        # lengths_mix: T, 1, 0, then its first interior length


def make_case(H, T, B, scale='flat', ragged=False, K=4):
    """float32 inputs of one case, read-only.  'unit': the distribution of test_attention.  'flat': Wa and ba times 0.02, so pre ~ 0.02 x and the
    softmax is nearly uniform.  'sat': flat with out times 6: tanh saturated, 1 - m^2 ~ 0, ctx six times larger (with the unit projection on top the
    scores spread over hundreds and float32 itself, numpy's included, misses 1e-4 on ctx and dpre: no reference to hold a kernel to).  'zeros': flat,
    and every fourth feature (j % 4 == 1) has a zero row of Wa and ba = 0.0 or -0.0, so pre is an exact zero there while the sum the mask must drop
    is not.
    ragged: lengths from lengths_mix(B, T); `out_in` holds NaN behind each length."""
    assert scale in SCALES
    rng = np.random.default_rng(zlib.crc32(('%d %d %d %s %d %d' % (H, T, B, scale, ragged, K)).encode()))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    out, hn, Wa, ba, dctx = f(B, T, 2 * H), f(K, B, H), (f(H, H) / np.float32(np.sqrt(H))).astype(np.float32), f(H), f(B, H)
    if scale in ('flat', 'zeros', 'sat'):
        Wa = Wa * np.float32(0.02); ba = ba * np.float32(0.02)
    if scale == 'sat':
        out = out * np.float32(6.0)
    zero_j = np.zeros(H, bool)
    if scale == 'zeros':
        zero_j[1::4] = True
        if H == 1:
            zero_j[0] = True
        Wa[zero_j] = 0.0
        ba[zero_j] = np.where(np.arange(zero_j.sum()) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    lengths = lengths_mix(B, T, rng) if ragged else None
    out_in = out.copy()
    if ragged:
        out_in[np.arange(T)[None, :] >= lengths[:, None]] = np.nan
    c = dict(H=H, T=T, B=B, K=K, scale=scale, out=out, out_in=out_in, hn=hn, Wa=Wa, ba=ba, dctx=dctx, lengths=lengths, zero_j=zero_j)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def pre_f32(c):
    """The projection in float32 numpy (the CPU stand-in of the device's pre)."""
    return (hsum_f32(c['hn']) @ c['Wa'].T + c['ba']).astype(np.float32)


def make_exact_case(H, T, B, tstar, ragged=False, K=4):
    """The one-hot construction.  Wa = 0, ba = 100 on four features and 0.0 / -0.0 / negatives elsewhere, so pre = ba exactly and q is 100 on the four.
    Row t* of each utterance has h = out_fwd + out_bwd = +20 on the four features, every other row -20: scores 400 and -400, exp(-800) = 0 in float32.
    tstar: the dense row; a ragged utterance takes its last step, lengths[b] - 1."""
    rng = np.random.default_rng(zlib.crc32(('exact %d %d %d %d %d' % (H, T, B, tstar, ragged)).encode()))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    out, hn, dctx = f(B, T, 2 * H), f(K, B, H), f(B, H)
    Wa = np.zeros((H, H), np.float32)
    hot = np.array([0, H // 4 + 1, H // 2 + 2, H - 1])
    ba = np.where(np.arange(H) % 3 == 0, np.float32(0.0), np.where(np.arange(H) % 3 == 1, np.float32(-0.0), -np.abs(f(H)) - np.float32(0.5))).astype(np.float32)
    ba[hot] = 100.0
    lengths = lengths_mix(B, T, rng) if ragged else None
    ts = np.full(B, tstar) if not ragged else lengths.astype(np.int64) - 1            # (-1: an empty utterance)
    for b in range(B):
        fw = out[b][:, hot]
        out[b][:, H + hot] = np.float32(-20.0) - fw
        if ts[b] >= 0:
            out[b, ts[b], H + hot] = np.float32(20.0) - fw[ts[b]]
    out_in = out.copy()
    if ragged:
        out_in[np.arange(T)[None, :] >= lengths[:, None]] = np.nan
    c = dict(H=H, T=T, B=B, K=K, scale='exact', out=out, out_in=out_in, hn=hn, Wa=Wa, ba=ba, dctx=dctx, lengths=lengths, tstar=ts, hot=hot,
             zero_j=(ba <= 0))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ----------------------------------------------------------------------------- case lists
# attention.hip keeps h_t for the whole utterance in LDS (CACHE) while  fixed + max(T, R) H 4 <= LDS_MAX  with  fixed = (Tp + 32) 4  in the forward and
# (2 Tp + 32) 4  in the backward, Tp = T rounded up to 4.  Last cached T:   H     forward  backward
#                                                                          64       629      620
#                                                                         128       317      314
#                                                                         256       159      158
# (H, T, forward cached, backward cached)
CACHE_BORDER = [(128, 314, True, True), (128, 315, True, False), (128, 317, True, False), (128, 318, False, False),
                (256, 158, True, True), (256, 159, True, False), (256, 160, False, False),
                (64, 620, True, True), (64, 621, True, False), (64, 629, True, False), (64, 630, False, False)]
SOFTMAX_STRIDE = [(64, AT + 1, True, True), (128, AT + 1, False, False)]      # the t += AT loops take a second trip of one element


def tile_edges(H):
    R = rows_per_pass(H)
    return [1, R - 1, R, R + 1, R * AU - 1, R * AU, R * AU + 1, 2 * R * AU + 3]


def cached(H, T):
    """(forward cached, backward cached) -- the launcher's own arithmetic, for the lists above and for the CPU test that checks them against it."""
    R = rows_per_pass(H); Tp = (T + 3) & ~3
    body = max(T, R) * H * 4
    return (Tp + 32) * 4 + body <= LDS_MAX, (2 * Tp + 32) * 4 + body <= LDS_MAX


def dense_B(H, T):
    """1 - 3 utterances; B = 1 at every third case."""
    return 1 + (H // 64 + T) % 3


# one T per kernel form and H for the scales that do not run the whole lists: both cached / forward cached, backward re-reading / both re-reading
FORM_T = {64: (131, 625, 630), 128: (67, 317, 318), 256: (33, 159, 160)}
V1_H = (1, 8, 96, 100, 320)
V1_T = (1, 3, 4, 5, 257)


ZEROS = [(64, 131), (64, 630), (128, 67), (128, 317), (256, 35), (256, 160), (100, 5), (320, 257)]      # (H, T) of the 'zeros' cases


def flat_family():
    """Every (H, T, B, ragged, scale) the GPU file runs against the tightened bounds."""
    seen = []
    for H in (64, 128, 256):
        for T in tile_edges(H) + [t for h, t, _, _ in CACHE_BORDER + SOFTMAX_STRIDE if h == H]:
            seen.append((H, T, dense_B(H, T), False, 'flat')); seen.append((H, T, RAGGED_B, True, 'flat'))
    for H in V1_H:
        for T in V1_T:
            seen.append((H, T, dense_B(H, T), False, 'flat')); seen.append((H, T, RAGGED_B, True, 'flat'))
    for H, T in ZEROS:
        seen.append((H, T, dense_B(H, T), False, 'zeros')); seen.append((H, T, RAGGED_B, True, 'zeros'))
    return seen


# Largest deviation of attention_from_pre(dtype=float32) from float64 over flat_family() (tests/test_attention_ref_cpu.py measures it again); the
# device is allowed 16 times this for its fma contraction, summation order and tanhf / expf, under the suite's older bounds as a ceiling.
FLAT_F32 = dict(ctx=3.7e-7, alpha=4.6e-8, dout=3.4e-7, dpre=1.1e-6)
CEILING = dict(ctx=1e-4, alpha=1e-5, dout=1e-4, dpre=1e-4)


def flat_bounds():
    return {k: min(16 * FLAT_F32[k], CEILING[k]) for k in FLAT_F32}
