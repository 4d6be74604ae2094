"""Reference, masks, inputs and case table of the MLP head parity tests (tests/test_head_forms_gpu.py, tests/test_head_ref_cpu.py).

The head of csrc/head.hip is  [Dropout(p)] -> Linear(Hin, H1) -> ReLU -> Dropout(p) -> [Linear(H1, C)].  head_forward / head_backward are its plain
float64 formulas (pinned against stock torch in the CPU test); masks() draws both dropout masks from oracle/ref_numpy.py's own Philox, never from
the device.  The rest restates the geometry of the three kernels -- which template instance a width selects, where the weight pass splits the batch
over its waves and rounds -- so that the case table can be checked for what it reaches without a GPU.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import ref_numpy as R

HR = 4                                              # head.hip: batch rows per workgroup of the two row passes
JR, WAVES, BCH = 4, 8, 1024                         # weight pass: output rows per workgroup, waves that split the batch, batch rows per round
STAGE_ROWS = 512 * 4 // JR                          # batch rows one staging iteration of a round covers (HT * 4 values, JR per row)
HC = 16                                             # most output columns
WIDTHS = (8, 16, 32, 64, 128, 256)                  # dep_head_mlp_supported: Hin and H1
SITES = (1, 2)                                      # _lib.SITE_FC0, _lib.SITE_FC1
GUARD = 8                                           # NaN rows behind every row buffer of the GPU test

# the bars of tests/test_kernels_gpu.py::test_fused_mlp_head_against_float64_with_the_same_masks, unchanged
A0_ATOL = 1e-6
ACT_RTOL = 2e-6                                     # z1, a1, z2, dz1: max-norm relative error
GRAD_RTOL = 5e-6                                    # dW1, db1, dW2, db2, dx


def f64(a):
    """float32-rounded float64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


# ----------------------------------------------------------------------------- reference
def head_forward(x, W1, b1, W2, b2, m0, m1):
    """x (B, Hin), W1 (H1, Hin), b1 (H1), W2 (C, H1) or None, b2 (C), masks (B, Hin) / (B, H1) or None for ones -> a0, z1, a1, z2 (None without W2)."""
    a0 = x if m0 is None else x * m0
    z1 = a0 @ W1.T + b1
    a1 = np.maximum(z1, 0.0)
    if m1 is not None:
        a1 = a1 * m1
    z2 = None if W2 is None else a1 @ W2.T + b2
    return a0, z1, a1, z2


def head_backward(dz2, a0, z1, a1, W1, W2, m0, m1):
    """-> dz1, dW1, db1, dW2, db2, dx  with  dz1 = (dz2 W2) * (z1 > 0) * m1  and  dx = (dz1 W1) * m0."""
    dz1 = (dz2 @ W2) * (z1 > 0)
    if m1 is not None:
        dz1 = dz1 * m1
    dx = dz1 @ W1
    if m0 is not None:
        dx = dx * m0
    return dz1, dz1.T @ a0, dz1.sum(0), dz2.T @ a1, dz2.sum(0), dx


def masks(B, Hin, H1, p, seed, sites, first):
    """(m0, m1) as float64, None where the head draws nothing: element (row, column) of a site is draw row * width + column."""
    if not p > 0:
        return None, None
    m0 = R.dropout_mask(B * Hin, p, seed, sites[0]).astype(np.float64).reshape(B, Hin) if first else None
    return m0, R.dropout_mask(B * H1, p, seed, sites[1]).astype(np.float64).reshape(B, H1)


# ----------------------------------------------------------------------------- geometry of the kernels
def fwd_instance(Hin):
    return 'head_mlp_fwd_kernel<%d>' % (Hin // 8)


def rows_instance(H1):
    return 'head_mlp_bwd_rows_kernel<%d>' % (H1 // 8)


W_INSTANCE = 'head_mlp_bwd_w_kernel'
ALL_INSTANCES = frozenset([fwd_instance(h) for h in WIDTHS] + [rows_instance(h) for h in WIDTHS] + [W_INSTANCE])


def supported(Hin, H1, C):
    ok = lambda h: 8 <= h <= 256 and h & (h - 1) == 0
    return ok(Hin) and ok(H1) and 0 <= C <= HC


def wave_rows(B):
    """Per wave of a weight-pass workgroup, the batch rows it sums, in its order: [lo, hi) of every 1024-row round, one round after the other."""
    rows = [[] for _ in range(WAVES)]
    for b0 in range(0, B, BCH):
        nb = min(B - b0, BCH)
        per = (nb + WAVES - 1) // WAVES
        for w in range(WAVES):
            rows[w] += range(b0 + min(w * per, nb), b0 + min(w * per + per, nb))
    return rows


def probe_rows(B):
    """The batch rows whose loss a gradient must show: row 0, the last, and the rows on each side of every boundary B crosses -- 3|4 (row groups
    of the row passes), the wave boundaries of every round of the weight pass, 511|512 (staging iterations) and 1023|1024, 2047|2048 (rounds)."""
    edges = {HR} | {b0 + STAGE_ROWS for b0 in range(0, B, BCH)}
    for rows in wave_rows(B):
        start = 0
        for k in range(1, len(rows) + 1):                     # each contiguous run of a wave starts at a boundary
            if k == len(rows) or rows[k] != rows[k - 1] + 1:
                edges.add(rows[start]); start = k
    out = {0, B - 1}
    for e in edges:
        out |= {e - 1, e}
    return sorted(r for r in out if 0 <= r < B)


# ----------------------------------------------------------------------------- cases
Case = namedtuple('Case', 'sec B Hin H1 C p first')

INSTANCE_SHAPES = [(8, 256), (16, 128), (32, 64), (64, 32), (128, 16), (256, 8), (8, 8), (256, 256)]
P_FIRST = [(0.0, False), (0.5, True), (0.3, False)]
BATCH_EDGES = [1, 3, 4, 5, 8, 9, 15, 16, 17, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2049]
WIDE_B = [513, 1025, 2049]
C_EDGES = [0, 1, 3, 4, 5, 15, 16]
REFUSED = [(64, 64, 17), (4, 64, 2), (64, 4, 2), (24, 64, 2), (64, 24, 2), (512, 64, 2), (64, 512, 2)]       # (Hin, H1, C)

CASES = ([Case('A', 5, hin, h1, 2, p, f) for hin, h1 in INSTANCE_SHAPES for p, f in P_FIRST] +
         [Case('B', b, 32, 16, 5, 0.5, True) for b in BATCH_EDGES] +
         [Case('B', b, 256, 256, 16, 0.0, False) for b in WIDE_B] +
         [Case('C', 37, 64, 64, c, 0.5, True) for c in C_EDGES] +
         [Case('D', b, hin, h1, c, 0.5, True) for hin, h1, c in ((32, 16, 5), (256, 256, 2)) for b in (5, 1025)])


def case_id(c):
    return '%s-B%d-%dx%d-C%d-p%g-%s' % (c.sec, c.B, c.Hin, c.H1, c.C, c.p, 'first' if c.first else 'nofirst')


def section(sec):
    return [c for c in CASES if c.sec == sec]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(' '.join(str(k) for k in key).encode()))


@functools.lru_cache(maxsize=None)
def _trunk(B, Hin, H1, p, first):
    """x, W1, b1, the dropout seed and both masks of a case: everything up to a1, which does not depend on C.  A batch row whose hidden units are
    all off (ReLU or mask: about one row in ten at H1 = 8, p = 0.5) adds nothing to dW1, db1 and dW2, so no gradient can show its loss; the draw
    is repeated under the next salt until every row of probe_rows(B) has a live unit.  The rule reads the inputs alone."""
    for salt in range(64):
        rng = _rng('head', B, Hin, H1, p, first, salt)
        x = rng.standard_normal((B, Hin)).astype(np.float32)
        W1 = (rng.standard_normal((H1, Hin)) / np.sqrt(Hin)).astype(np.float32)
        b1 = (rng.standard_normal(H1) * 0.5).astype(np.float32)
        seed = int(rng.integers(1, 2 ** 63))
        m0, m1 = masks(B, Hin, H1, p, seed, SITES, first)
        a1 = head_forward(f64(x), f64(W1), f64(b1), None, None, m0, m1)[2]
        if all(a1[r].any() for r in probe_rows(B)):
            break
    else:
        raise AssertionError('no draw with live probe rows')
    for a in (x, W1, b1):
        a.setflags(write=False)
    return dict(x=x, W1=W1, b1=b1, seed=seed, m0=m0, m1=m1)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """float32 inputs of a case, read-only: x, W1, b1 (shared by every C at the same shape), W2, b2, dz2 (None at C = 0), seed, m0, m1."""
    d = dict(_trunk(c.B, c.Hin, c.H1, c.p, c.first))
    rng = _rng('tail', c.B, c.H1, c.C)
    if c.C:
        d['W2'] = (rng.standard_normal((c.C, c.H1)) / np.sqrt(c.H1)).astype(np.float32)
        d['b2'] = rng.standard_normal(c.C).astype(np.float32)
        d['dz2'] = rng.standard_normal((c.B, c.C)).astype(np.float32)
        for k in ('W2', 'b2', 'dz2'):
            d[k].setflags(write=False)
    else:
        d['W2'] = d['b2'] = d['dz2'] = None
    return d


@functools.lru_cache(maxsize=None)
def reference(c):
    """The float64 forward and backward of a case from its own inputs: dict a0, z1, a1, z2, dz1, dW1, db1, dW2, db2, dx (read-only)."""
    d = inputs(c)
    opt = lambda a: None if a is None else f64(a)
    a0, z1, a1, z2 = head_forward(f64(d['x']), f64(d['W1']), f64(d['b1']), opt(d['W2']), opt(d['b2']), d['m0'], d['m1'])
    out = dict(a0=a0, z1=z1, a1=a1, z2=z2)
    if c.C:
        out.update(zip(('dz1', 'dW1', 'db1', 'dW2', 'db2', 'dx'), head_backward(f64(d['dz2']), a0, z1, a1, f64(d['W1']), f64(d['W2']), d['m0'], d['m1'])))
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


# ----------------------------------------------------------------------------- the weight pass in float32
def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, so one float64 add and one rounding to float32 follow (the double
    rounding differs from a true fma in about one result in 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def weight_rows_f32(D, A):
    """out = D^T A and bias = column sums of D in float32, in weight_rows' own order: per wave one fma chain (one add chain for the bias) over its
    rows that carries across the 1024-row rounds, then the eight wave partials added in wave order from 0.  D (B, J), A (B, I), float32."""
    D = np.asarray(D, np.float32); A = np.asarray(A, np.float32)
    out = np.zeros((D.shape[1], A.shape[1]), np.float32); bias = np.zeros(D.shape[1], np.float32)
    for rows in wave_rows(D.shape[0]):
        acc = np.zeros_like(out); sb = np.zeros_like(bias)
        for b in rows:
            acc = fma32(D[b][:, None], A[b][None, :], acc)
            sb = sb + D[b]
        out = out + acc; bias = bias + sb
    return out, bias


def weight_bound(D, A):
    """The a-priori bound of that walk per element of D^T A:  (chain length + 8) 2^-24 sum_b |D[b, j] A[b, i]|,  the chain being the longest
    wave's (every fma and every one of the eight final adds rounds once, each by at most 2^-24 of a partial sum that sum_b |d a| bounds)."""
    chain = max(len(r) for r in wave_rows(D.shape[0]))
    return (chain + WAVES) * 2.0 ** -24 * (np.abs(f64(D)).T @ np.abs(f64(A)))
