"""The small kernels every training step runs through (csrc/elementwise.hip), at the sizes where their indexing changes and
against references that do not come from the library: the dropout draw against the oracle's own Philox (bit for bit), the
loss heads and the loss reduction, colsum, LayerNorm's capped parameter reduction, Adam, and the helper entry points.
Every expected value and tolerance here is fixed in advance: exact where the arithmetic is exact, otherwise the tolerance
of the existing one-shape test of the same kernel (tests/test_kernels_gpu.py).
Run on the MI355X box:  python -m pytest tests/test_small_kernels_gpu.py -m gpu -q"""
import numpy as np
import pytest

from oracle import ref_numpy as R

torch = pytest.importorskip('torch')
pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

if torch.cuda.is_available():
    from icassp2022_depression_amd import _lib as L
    DEV = torch.device('cuda:0')

F32 = np.float32
HI_SEED, MAX_SEED = (7 << 32) | 99, 2 ** 64 - 1


def r32(a):
    """float64 holding float32 values: what the kernel is given."""
    return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def bits(t):
    """The tensor's own values on the host, dtype kept: for equality comparisons."""
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


# ----------------------------------------------------------------------------- B. the dropout draw
# Every value of every axis occurs (n: 1 3 4 5 255 256 257 1027 70001; p: 0 0.3 0.5 0.999; four seeds; five sites); the seeds with a
# high word run at n = 70001.
DRAW_CASES = [
    (1, 0.3, 0, 0), (3, 0.5, 99, 1), (4, 0.999, HI_SEED, 16), (5, 0.0, MAX_SEED, 17), (255, 0.5, 0, 0xFFFFFFFF),
    (256, 0.3, 99, 17), (257, 0.5, HI_SEED, 0), (1027, 0.999, MAX_SEED, 1), (1027, 0.3, 99, 16), (1027, 0.0, 0, 1),
    (70001, 0.3, HI_SEED, 17), (70001, 0.5, MAX_SEED, 0xFFFFFFFF), (70001, 0.5, HI_SEED, 16), (70001, 0.999, MAX_SEED, 0),
]


@pytest.mark.parametrize('n,p,seed,site', DRAW_CASES)
def test_device_draw_equals_the_independent_philox(n, p, seed, site):
    """dep_dropout_mask against oracle.dropout_mask, bit for bit: the multipliers, the round count, the key schedule, the counter
    layout (group index, site, the constant word), the >> 8 conversion, the keep rule and the scale.
    NOT verified: the counter's second word, g4 >> 32.  It is non-zero only from element 2**34 on, and no buffer of that size
    (64 GiB of mask) can be allocated for a test; through this entry point it is always 0."""
    got = bits(L.dropout_mask(n, p, seed, site, DEV))
    want = R.dropout_mask(n, p, seed, site)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_a_uniform_equal_to_p_is_kept():
    """Seed 985, site 17: element 238's uniform is exactly 0.5 (its word >> 8 is 2**23), so at p = 0.5 the keep rule u >= p is on
    its edge: the element is kept."""
    seed, site, e, n = 985, 17, 238, 257
    w = int(R.philox4x32_10((e // 4, 0, site, 0x2545F491), (seed, 0))[e % 4])
    assert w >> 8 == 1 << 23                                   # the premise, from the oracle's Philox alone
    want = R.dropout_mask(n, 0.5, seed, site)
    assert want[e] == 2.0
    got = bits(L.dropout_mask(n, 0.5, seed, site, DEV))
    assert got[e] == 2.0
    assert np.array_equal(got, want)


def zero_some_kept(z, mask):
    """+0.0 and -0.0 at the first two kept positions (where a wrong gradient would show), when there are two."""
    kept = np.flatnonzero(mask)
    if kept.size >= 2:
        z[kept[0]] = 0.0
        z[kept[1]] = -0.0
    return kept[:2] if kept.size >= 2 else kept[:0]


@pytest.mark.parametrize('n', [1, 5, 257, 1027])
@pytest.mark.parametrize('p,seed,site', [(0.3, 99, 2), (0.5, HI_SEED, 17)])
def test_dropout_kernels_apply_the_oracle_mask_exactly(n, p, seed, site):
    """y = x * mask, a = max(z, 0) * mask, dz = da * (z > 0) * mask with the ORACLE's mask.  A float32 times a float32 mask value
    rounds once on both sides, so the comparison is equality with numpy's float32 product."""
    rng = np.random.default_rng(1000 + n)
    mask = R.dropout_mask(n, p, seed, site)
    x = rng.standard_normal(n).astype(F32)
    z = rng.standard_normal(n).astype(F32)
    zeros = zero_some_kept(z, mask)
    da = rng.standard_normal(n).astype(F32)
    xd, zd, dad = dev(x), dev(z), dev(da)
    # out of place, inside a poisoned buffer: nothing before or after the n elements is written
    buf = torch.full((n + 8,), 7.0, device=DEV)
    L.dropout(xd, buf[4:4 + n], p, seed, site)
    got = bits(buf)
    assert np.array_equal(got[4:4 + n], x * mask)
    assert np.all(got[:4] == 7.0) and np.all(got[4 + n:] == 7.0)
    # in place
    xi = xd.clone()
    L.dropout(xi, xi, p, seed, site)
    assert np.array_equal(bits(xi), x * mask)
    a = torch.full((n,), 7.0, device=DEV); dz = torch.full((n,), 7.0, device=DEV)
    L.relu_dropout_fwd(zd, a, p, seed, site)
    L.relu_dropout_bwd(dad, zd, dz, p, seed, site)
    a, dz = bits(a), bits(dz)
    assert np.array_equal(a, np.maximum(z, F32(0)) * mask)
    assert np.array_equal(dz, da * (z > 0).astype(F32) * mask)
    assert np.all(a[zeros] == 0.0) and np.all(dz[zeros] == 0.0)


@pytest.mark.parametrize('n', [1, 5, 257, 1027])
def test_dropout_kernels_at_p0(n):
    """p = 0: dep_dropout is an exact copy out of place and touches nothing in place; the relu pair is plain relu and its gradient."""
    rng = np.random.default_rng(2000 + n)
    x = rng.standard_normal(n).astype(F32)
    z = rng.standard_normal(n).astype(F32)
    zeros = zero_some_kept(z, np.ones(n, F32))
    da = rng.standard_normal(n).astype(F32)
    xd, zd, dad = dev(x), dev(z), dev(da)
    buf = torch.full((n + 8,), 7.0, device=DEV)
    L.dropout(xd, buf[4:4 + n], 0.0, 99, 2)
    got = bits(buf)
    assert np.array_equal(got[4:4 + n], x)
    assert np.all(got[:4] == 7.0) and np.all(got[4 + n:] == 7.0)
    xi = xd.clone()
    L.dropout(xi, xi, 0.0, 99, 2)
    assert np.array_equal(bits(xi), x)
    a = torch.full((n,), 7.0, device=DEV); dz = torch.full((n,), 7.0, device=DEV)
    L.relu_dropout_fwd(zd, a, 0.0, 99, 2)
    L.relu_dropout_bwd(dad, zd, dz, 0.0, 99, 2)
    a, dz = bits(a), bits(dz)
    assert np.array_equal(a, np.maximum(z, F32(0)))
    assert np.array_equal(dz, da * (z > 0).astype(F32))
    assert np.all(a[zeros] == 0.0) and np.all(dz[zeros] == 0.0)


# ----------------------------------------------------------------------------- C. loss heads and the reduction
# The head kernel's block is 128 rows and its per-row arrays hold 16 classes.  Every B of {1, 127, 128, 129, 513} and every C of
# {1, 2, 3, 7, 16} occurs.
CE_CASES = [(1, 1), (1, 3), (127, 2), (127, 16), (128, 1), (128, 7), (129, 3), (129, 16), (513, 2), (513, 7), (513, 16)]


def labels_with_both_ends(rng, B, C):
    y = rng.integers(0, C, B)
    y[-1] = C - 1
    if B > 1:
        y[0] = 0
    return y


@pytest.mark.parametrize('B,C', CE_CASES)
def test_ce_heads_over_block_and_class_edges(B, C):
    rng = np.random.default_rng(100 * B + C)
    z = r32(rng.standard_normal((B, C)) * 2)
    y = labels_with_both_ends(rng, B, C)
    zd = dev(z)
    y32 = torch.from_numpy(y.astype(np.int32)).to(DEV); y64 = torch.from_numpy(y.astype(np.int64)).to(DEV)
    p = R.softmax(z)
    ls_soft, dp = R.ce_on_probs(p, y)
    refs = {L.LOSS_CE_ON_SOFTMAX: (ls_soft, R.softmax_bwd(p, dp)), L.LOSS_CE_LOGITS: R.ce_logits(z, y)}
    for kind, (loss_ref, dz_ref) in refs.items():
        out = torch.full((B, C), 7.0, device=DEV); rows = torch.full((B,), 7.0, device=DEV); dz = torch.full((B, C), 7.0, device=DEV)
        loss = torch.full((1,), float('nan'), device=DEV)
        L.head_loss(kind, zd, y32, out, rows, dz, B)
        L.reduce_loss(rows, B, loss)
        assert np.abs(host(out) - p).max() < 1e-6
        assert relerr(host(dz), dz_ref) < 1e-5
        assert abs(host(loss)[0] - loss_ref) < 1e-6 * max(1.0, abs(loss_ref))
        # torch.long labels read in place: bit-identical
        out64 = torch.full((B, C), 7.0, device=DEV); rows64 = torch.full((B,), 7.0, device=DEV); dz64 = torch.full((B, C), 7.0, device=DEV)
        L.head_loss(kind | L.LOSS_LABELS_I64, zd, y64, out64, rows64, dz64, B)
        assert torch.equal(out64, out) and torch.equal(rows64, rows) and torch.equal(dz64, dz)


REG_KINDS = [('LOSS_L1_RELU', 'l1_loss', True), ('LOSS_SMOOTHL1_RELU', 'smooth_l1_loss', True), ('LOSS_SMOOTHL1', 'smooth_l1_loss', False)]


def reg_reference(fn, relu, z, t):
    o = np.maximum(z, 0.0) if relu else z
    loss, g = getattr(R, fn)(o, t)
    return o, loss, (g * (z > 0) if relu else g)


@pytest.mark.parametrize('B,C', [(1, 1), (127, 3), (128, 1), (129, 3), (513, 1), (513, 3)])
@pytest.mark.parametrize('kind,fn,relu', REG_KINDS)
def test_regression_heads_over_block_edges(kind, fn, relu, B, C):
    """norm = B * C on both calls: the oracle's mean runs over every element."""
    rng = np.random.default_rng(100 * B + C)
    z = r32(rng.standard_normal((B, C)) * 3 + 1)
    t = r32(rng.uniform(-1, 3, (B, C)))
    o, loss_ref, g = reg_reference(fn, relu, z, t)
    out = torch.full((B, C), 7.0, device=DEV); rows = torch.full((B,), 7.0, device=DEV); dz = torch.full((B, C), 7.0, device=DEV)
    loss = torch.full((1,), float('nan'), device=DEV)
    L.head_loss(getattr(L, kind), dev(z), dev(t), out, rows, dz, B * C)
    L.reduce_loss(rows, B * C, loss)
    assert np.abs(host(out) - o).max() < 1e-6
    assert np.abs(host(dz) - g).max() < 1e-6
    assert abs(host(loss)[0] - loss_ref) < 1e-6 * max(1.0, abs(loss_ref))


def test_saturated_logits_have_exact_outcomes():
    """Logits 120 apart: exp(-120) is 0 in float32, so the softmax is exactly (1, 0); the log-sum-exp is 0, so a CE_LOGITS row
    loss is 0 for the right class and z_max - z_y for a wrong one; nothing overflows on the way."""
    for zs, ys in (([(60, -60), (60, -60), (-60, 60), (-60, 60)], [0, 1, 1, 0]),
                   ([(-60, 60, -60), (-60, 60, -60), (-60, 60, -60), (60, -60, -60), (-60, -60, 60)], [1, 0, 2, 0, 1])):
        z = np.array(zs, dtype=np.float64); y = np.array(ys)
        B, C = z.shape
        zd = dev(z); yd = torch.from_numpy(y.astype(np.int32)).to(DEV)
        onehot_max = (z == z.max(1, keepdims=True)).astype(np.float64)
        for kind in (L.LOSS_CE_LOGITS, L.LOSS_CE_ON_SOFTMAX):
            out = torch.full((B, C), 7.0, device=DEV); rows = torch.full((B,), 7.0, device=DEV); dz = torch.full((B, C), 7.0, device=DEV)
            L.head_loss(kind, zd, yd, out, rows, dz, B)
            assert np.array_equal(host(out), onehot_max)
            assert np.isfinite(host(rows)).all() and np.isfinite(host(dz)).all()
            if kind == L.LOSS_CE_LOGITS:
                want = z.max(1) - z[np.arange(B), y]
                got = host(rows)
                assert np.all(got[want == 0] == 0.0)
                assert np.all(np.abs(got - want)[want > 0] <= 1e-6 * want[want > 0])
                assert relerr(host(dz), R.ce_logits(z, y)[1]) < 1e-5
            else:
                p = R.softmax(z)
                ls, dp = R.ce_on_probs(p, y)
                assert np.abs(host(rows).mean() - ls) < 1e-6 * max(1.0, abs(ls))
                assert relerr(host(dz), R.softmax_bwd(p, dp)) < 1e-5


@pytest.mark.parametrize('kind,fn,relu', REG_KINDS)
def test_regression_heads_at_their_kinks(kind, fn, relu):
    """d = out - target exactly 0, +1 and -1 (SmoothL1's switch between its branches, L1's corner), and z exactly +0.0 / -0.0 under
    the ReLU kinds.  Where the reference's gradient is 0 the kernel's must be 0 exactly."""
    z = np.array([[2.5, 2.5, 2.5], [0.0, -0.0, 0.0], [-0.0, 4.0, 0.25], [0.75, 1.0, 3.0]], dtype=np.float64)
    t = np.array([[2.5, 1.5, 3.5], [1.0, 1.0, 0.0], [0.0, 4.0, 1.25], [0.75, 0.0, 3.0]], dtype=np.float64)
    B, C = z.shape
    o, loss_ref, g = reg_reference(fn, relu, z, t)
    out = torch.full((B, C), 7.0, device=DEV); rows = torch.full((B,), 7.0, device=DEV); dz = torch.full((B, C), 7.0, device=DEV)
    loss = torch.full((1,), float('nan'), device=DEV)
    L.head_loss(getattr(L, kind), dev(z), dev(t), out, rows, dz, B * C)
    L.reduce_loss(rows, B * C, loss)
    assert np.abs(host(out) - o).max() < 1e-6
    got = host(dz)
    assert np.abs(got - g).max() < 1e-6
    assert abs(host(loss)[0] - loss_ref) < 1e-6 * max(1.0, abs(loss_ref))
    if relu:
        assert np.all(got[z == 0] == 0.0)                      # +0.0 and -0.0 alike
    if fn == 'l1_loss':
        assert np.all(got[(o - t) == 0] == 0.0)
    assert np.all(got[g == 0] == 0.0)


def test_head_loss_optional_outputs_and_refusals():
    rng = np.random.default_rng(31)
    B, C = 129, 3
    z = r32(rng.standard_normal((B, C)) * 2)
    y = labels_with_both_ends(rng, B, C)
    zd = dev(z); yd = torch.from_numpy(y.astype(np.int32)).to(DEV)
    p = R.softmax(z)
    loss_ref, dz_ref = R.ce_logits(z, y)
    rows_ref = -R.log_softmax(z)[np.arange(B), y]
    # inference: no target, out alone
    out = torch.full((B, C), 7.0, device=DEV)
    L.head_loss(L.LOSS_CE_ON_SOFTMAX, zd, None, out, None, None, B)
    assert np.abs(host(out) - p).max() < 1e-6
    t = r32(rng.uniform(-1, 3, (B, C)))
    out = torch.full((B, C), 7.0, device=DEV)
    L.head_loss(L.LOSS_L1_RELU, zd, None, out, None, None, B * C)
    assert np.abs(host(out) - np.maximum(z, 0)).max() < 1e-6
    # no out: rows and dz as before
    rows = torch.full((B,), 7.0, device=DEV); dz = torch.full((B, C), 7.0, device=DEV)
    L.head_loss(L.LOSS_CE_LOGITS, zd, yd, None, rows, dz, B)
    assert np.abs(host(rows) - rows_ref).max() < 1e-6 * max(1.0, np.abs(rows_ref).max())
    assert relerr(host(dz), dz_ref) < 1e-5
    o, lref, g = reg_reference('smooth_l1_loss', True, z, t)
    rows2 = torch.full((B,), 7.0, device=DEV); dz2 = torch.full((B, C), 7.0, device=DEV); loss = torch.zeros(1, device=DEV)
    L.head_loss(L.LOSS_SMOOTHL1_RELU, zd, dev(t), None, rows2, dz2, B * C)
    L.reduce_loss(rows2, B * C, loss)
    assert np.abs(host(dz2) - g).max() < 1e-6 and abs(host(loss)[0] - lref) < 1e-6 * max(1.0, abs(lref))
    # no dz: the call succeeds and the rows are the same bits
    rows3 = torch.full((B,), 7.0, device=DEV)
    L.head_loss(L.LOSS_CE_LOGITS, zd, yd, None, rows3, None, B)
    assert torch.equal(rows3, rows)
    # refusals: more classes than the kernel's per-row arrays hold; a gradient without a target
    z17 = torch.zeros(4, 17, device=DEV); y17 = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(L.DepError):
        L.head_loss(L.LOSS_CE_LOGITS, z17, y17, torch.empty(4, 17, device=DEV), torch.empty(4, device=DEV), torch.empty(4, 17, device=DEV), 4)
    with pytest.raises(L.DepError):
        L.head_loss(L.LOSS_CE_LOGITS, zd, None, out, None, dz, B)
    with pytest.raises(L.DepError):
        L.head_loss(L.LOSS_CE_LOGITS, zd, None, out, rows, None, B)


@pytest.mark.parametrize('B,norm', [(1, 1), (255, 255), (256, 256), (257, 3 * 257), (1000, 7)])
def test_reduce_loss_over_its_stride_and_its_accumulate_flag(B, norm):
    """One block of 256 threads strides over the rows.  Rows are O(1), so 1e-6 relative is some 16 float32 roundings of the result."""
    rng = np.random.default_rng(B)
    rows = rng.uniform(0.25, 1.75, B).astype(F32)
    s = rows.astype(np.float64).sum() / norm
    rd = dev(rows)
    out = torch.full((3,), float('nan'), device=DEV)             # poisoned: accumulate = 0 overwrites, and only word 0
    out[1:] = 7.0
    L.reduce_loss(rd, norm, out[0:1])
    got = host(out)
    assert abs(got[0] - s) < 1e-6 * max(1.0, abs(s))
    assert np.all(got[1:] == 7.0)
    preset = 0.375
    acc = torch.full((1,), preset, device=DEV)
    L.reduce_loss(rd, norm, acc, accumulate=True)
    L.reduce_loss(rd, norm, acc, accumulate=True)
    ref = preset + 2 * s
    assert abs(host(acc)[0] - ref) < 1e-6 * max(1.0, abs(ref))
    L.reduce_loss(rd, norm, acc, accumulate=False)
    assert abs(host(acc)[0] - s) < 1e-6 * max(1.0, abs(s))


def test_loss_accumulate_sums_in_float64_and_keeps_running_maxima():
    losses = [F32(0.1), F32(3.7e-8), F32(1234.5677)]
    status = [0, 5, 2]
    soft = [1, 0, 3]
    acc = torch.tensor([0.25, 0.0, 0.0], dtype=torch.float64, device=DEV)
    total, smax, fmax = 0.25, 0.0, 0.0
    for l, st, so in zip(losses, status, soft):
        ld = torch.tensor([float(l)], dtype=torch.float32, device=DEV)
        sd = torch.tensor([st], dtype=torch.int32, device=DEV); fd = torch.tensor([so], dtype=torch.int32, device=DEV)
        L.loss_accumulate(ld, sd, fd, acc)
        total = total + float(l); smax = max(smax, float(st)); fmax = max(fmax, float(so))      # Python floats are float64
        assert bits(acc).tolist() == [total, smax, fmax]
    # 0.25 + 0.1f + 3.7e-8f is not representable in float32 next to 1234.57: a float32 accumulator would have lost it
    assert total != float(F32(total))
    L.loss_accumulate(None, torch.tensor([7], dtype=torch.int32, device=DEV), None, acc)
    assert bits(acc).tolist() == [total, 7.0, fmax]
    L.loss_accumulate(torch.tensor([2.0], dtype=torch.float32, device=DEV), None, None, acc)
    assert bits(acc).tolist() == [total + 2.0, 7.0, fmax]


# ----------------------------------------------------------------------------- D. colsum, LayerNorm's capped reduction, Adam, helpers
SENTINEL = 1.0e6


@pytest.mark.parametrize('M,N,ld', [(1, 1, 1), (3, 5, 5), (4, 64, 64), (29, 65, 70), (32, 64, 64), (33, 130, 256), (61, 7, 9), (1000, 3, 3)])
def test_colsum_over_row_tails_column_blocks_and_strides(M, N, ld):
    """The kernel sums 32 rows per pass of its main loop (8 loads in each of 4 row groups), the rest 4 at a time, in blocks of 64
    columns.  The M x N operand is the top-left corner of a wider and taller array whose other elements are 1e6: reading a
    column >= N, ignoring ld, or reading a row >= M moves a sum by 1e6."""
    rng = np.random.default_rng(1000 * M + N)
    full = np.full((M + 4, ld), SENTINEL, dtype=F32)
    full[:M, :N] = rng.standard_normal((M, N)).astype(F32)
    fd = dev(full)
    x = fd[:M, :N]
    assert x.stride(0) == ld and x.data_ptr() == fd.data_ptr()
    out = torch.full((N + 8,), 7.0, device=DEV)
    L.colsum(x, out[:N])
    got = host(out)
    assert np.abs(got[:N] - full[:M, :N].astype(np.float64).sum(0)).max() < 1e-4
    assert np.all(got[N:] == 7.0)


def ln_case(rows, F, seed):
    rng = np.random.default_rng(seed)
    x = r32(rng.standard_normal((rows, F)) * 2 + 0.3)
    g = r32(rng.standard_normal(F)); b = r32(rng.standard_normal(F))
    dy = r32(rng.standard_normal((rows, F)))
    return x, g, b, dy


def check_layernorm(xd, gd, bd, dyd, x, g, b, dy):
    """test_layernorm's calls and tolerances (tests/test_kernels_gpu.py); returns the device outputs for further comparisons."""
    F = x.shape[1]
    y, mr = L.layernorm_fwd(xd, gd, bd)
    yr, cache = R.layernorm_fwd(x, g, b)
    assert np.abs(host(y) - yr).max() < 2e-5
    dg = torch.full((F + 8,), 7.0, device=DEV); db = torch.full((F + 8,), 7.0, device=DEV)
    dx = L.layernorm_bwd(dyd, xd, gd, mr, dg[:F], db[:F], want_dx=True)
    dxr, dgr, dbr = R.layernorm_bwd(dy, g, cache)
    assert relerr(host(dx), dxr) < 2e-5
    assert relerr(host(dg)[:F], dgr) < 2e-5
    assert relerr(host(db)[:F], dbr) < 2e-5
    assert np.all(host(dg)[F:] == 7.0) and np.all(host(db)[F:] == 7.0)
    return y, mr, dx, dg[:F], db[:F]


@pytest.mark.parametrize('rows,F', [(32768, 5), (32805, 39), (40000, 7)])
def test_layernorm_param_gradient_at_the_block_cap(rows, F):
    """The parameter gradient runs over min(ceil(rows / 64), 512) blocks: 32768 rows are the last count with 64 rows per block,
    32805 and 40000 rows share 512 blocks at 65 and 79 rows each (40000: the last blocks are empty).  Every full-size call is capped."""
    x, g, b, dy = ln_case(rows, F, rows + F)
    check_layernorm(dev(x), dev(g), dev(b), dev(dy), x, g, b, dy)


def off1(a):
    """A device copy of `a` that starts one float into its buffer: 4-byte aligned, not 16."""
    buf = torch.empty(a.size + 5, dtype=torch.float32, device=DEV)
    v = buf[1:1 + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=F32)))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def drain(request):
    """What the library launched since the last call (the log is emptied, so the entries go to the per-test record conftest.py keeps)."""
    raw = L.instance_log_read(reset=True)
    rec = getattr(request.config, '_dep_instances', None)
    if rec is not None:
        rec.setdefault(request.node.nodeid, set()).update(raw)
    return raw


def test_layernorm_scalar_kernel_at_a_vector_width(request):
    """F = 256 with operands one float off 16-byte alignment: the 16-byte kernel must stand aside for the scalar one.  Against the
    oracle, and against the aligned call (the two kernels sum a row in different orders: the tolerance, not equality)."""
    rows, F = 37, 256
    x, g, b, dy = ln_case(rows, F, 77)
    drain(request)
    ya, _, dxa, dga, dba = check_layernorm(dev(x), dev(g), dev(b), dev(dy), x, g, b, dy)
    launched = drain(request)
    assert any('ln_fwd_vec_kernel' in k for k in launched), launched
    yu, _, dxu, dgu, dbu = check_layernorm(off1(x), off1(g), off1(b), off1(dy), x, g, b, dy)
    launched = drain(request)
    assert any('ln_fwd_kernel' in k for k in launched) and not any('ln_fwd_vec_kernel' in k for k in launched), launched
    assert np.abs(host(yu) - host(ya)).max() < 2e-5
    assert relerr(host(dxu), host(dxa)) < 2e-5 and relerr(host(dgu), host(dga)) < 2e-5 and relerr(host(dbu), host(dba)) < 2e-5


def test_layernorm_of_constant_rows_is_beta():
    """Every x of a row 0.5, F = 39: the row sum 19.5 and the mean 0.5 are exact, x - mean is 0, and 0 * rstd * gamma + beta is beta."""
    rows, F = 130, 39
    rng = np.random.default_rng(5)
    g = rng.standard_normal(F).astype(F32); b = rng.standard_normal(F).astype(F32)
    y, mr = L.layernorm_fwd(torch.full((rows, F), 0.5, device=DEV), dev(g), dev(b))
    assert np.array_equal(bits(y), np.broadcast_to(b, (rows, F)))
    mr = bits(mr)
    assert np.all(mr[:, 0] == 0.5)
    assert np.abs(mr[:, 1].astype(np.float64) - 1e-5 ** -0.5).max() < 1e-6 * 1e-5 ** -0.5


LR, B1, B2, EPS = (float(F32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))        # as the kernel receives them


def adam_run(n, decoupled, wd, first_step, steps, seed, zero_moments=True):
    """Device and float64 oracle side by side.  p starts inside (-0.4, 0.4) and moves at most 3.2 lr per step (|m_hat| / sqrt(v_hat)
    <= (1 - b1) / sqrt(1 - b2)), so it stays below 0.5 where a float32 rounding is at most 2**-26 = 1.5e-8: the kernel rounds p at most
    twice per step (the decoupled decay, the update), at most 6e-7 over 20 steps, inside the existing test's 1e-6."""
    rng = np.random.default_rng(seed)
    wd = float(F32(wd))
    p = r32(rng.uniform(-0.4, 0.4, n))
    m = np.zeros(n) if zero_moments else r32(rng.standard_normal(n) * 0.1)
    v = np.zeros(n) if zero_moments else r32(rng.uniform(0.5, 1.5, n))
    pd, md, vd = dev(p), dev(m), dev(v)
    for step in range(first_step, first_step + steps):
        g = r32(rng.standard_normal(n))
        L.adam_step(pd, dev(g), md, vd, LR, B1, B2, EPS, wd, decoupled, step)
        p, m, v = R.adam_step(p, g, m, v, step, LR, wd=wd, decoupled=decoupled, b1=B1, b2=B2, eps=EPS)
    assert np.abs(p).max() < 0.5
    assert np.abs(host(pd) - p).max() < 1e-6
    assert relerr(host(md), m) < 1e-6
    assert relerr(host(vd), v) < 1e-6


@pytest.mark.parametrize('n', [1, 255, 256, 257, 100003])
@pytest.mark.parametrize('decoupled,wd', [(True, 1e-2), (False, 0.0), (False, 1e-3)])
def test_adam_twenty_steps_with_moments(n, decoupled, wd):
    """p, and the moments m and v the existing test never reads, after 20 consecutive steps.  The hyper-parameters are rounded to
    float32 on both sides: 1 - float32(0.999) is 1.3e-5 away from 0.001, which the moments' 1e-6 would see."""
    adam_run(n, decoupled, wd, 1, 20, 10 * n + int(decoupled))


@pytest.mark.parametrize('decoupled,wd', [(True, 1e-2), (False, 1e-3)])
def test_adam_late_steps(decoupled, wd):
    """Step counter from 100000 on (both bias corrections 1 to float64's last bit), from non-zero moments."""
    adam_run(257, decoupled, wd, 100000, 20, 4, zero_moments=False)


@pytest.mark.parametrize('n', [1, 257, 100003])
def test_adam_with_zero_gradient_from_zero_moments(n):
    rng = np.random.default_rng(n)
    p = rng.uniform(-2, 2, n).astype(F32)
    zero = np.zeros(n, F32)
    # no decay: 0 / (0 + eps) is 0, p keeps its bits
    pd, md, vd = dev(p), dev(zero), dev(zero)
    L.adam_step(pd, dev(zero), md, vd, LR, B1, B2, EPS, 0.0, False, 1)
    assert np.array_equal(bits(pd), p) and np.array_equal(bits(md), zero) and np.array_equal(bits(vd), zero)
    # decoupled decay alone: p (1 - lr wd), one float32 rounding of the factor and one of the product: within one ulp of p
    wd = float(F32(1e-2))
    pd, md, vd = dev(p), dev(zero), dev(zero)
    L.adam_step(pd, dev(zero), md, vd, LR, B1, B2, EPS, wd, True, 1)
    want = p.astype(np.float64) * (1.0 - LR * wd)
    assert np.all(np.abs(host(pd) - want) <= np.abs(want) * 2.0 ** -23)
    assert np.any(bits(pd) != p)
    assert np.array_equal(bits(md), zero) and np.array_equal(bits(vd), zero)


HELPER_N = [1, 255, 257, 5000]


def in_poison(n, value=7.0):
    """n elements inside a longer poisoned buffer; returns (buffer, the view)."""
    buf = torch.full((n + 8,), value, device=DEV)
    return buf, buf[4:4 + n]


def fence_ok(buf, n, value=7.0):
    b = bits(buf)
    return bool(np.all(b[:4] == value) and np.all(b[4 + n:] == value))


@pytest.mark.parametrize('n', HELPER_N)
def test_fill_is_exact(n):
    buf, v = in_poison(n)
    L.fill(v, -1.25)
    assert np.all(bits(v) == F32(-1.25)) and fence_ok(buf, n)
    L.fill(v, 0.1)
    assert np.all(bits(v) == F32(0.1)) and fence_ok(buf, n)


@pytest.mark.parametrize('n', HELPER_N)
def test_axpby(n):
    rng = np.random.default_rng(n)
    x = r32(rng.standard_normal(n)); y = r32(rng.standard_normal(n))
    a, b = float(F32(1.7)), float(F32(-0.3))
    buf, yd = in_poison(n)
    yd.copy_(dev(y))
    L.axpby(dev(x), yd, a, b)
    assert relerr(host(yd), a * x + b * y) < 1e-6 and fence_ok(buf, n)
    # b == 0 must not read y: NaN in, a * x rounded to float32 out
    buf, yd = in_poison(n)
    yd.fill_(float('nan'))
    L.axpby(dev(x), yd, a, 0.0)
    got = bits(yd)
    assert np.isfinite(got).all()
    assert np.array_equal(got, (F32(a) * x.astype(F32)))
    assert fence_ok(buf, n)


@pytest.mark.parametrize('n', HELPER_N)
def test_sigmoid_gate(n):
    rng = np.random.default_rng(n)
    g = r32(rng.standard_normal(n) * 4); x = r32(rng.standard_normal(n))
    buf, yd = in_poison(n)
    L.sigmoid_gate(dev(g), dev(x), yd)
    assert relerr(host(yd), R.sigmoid(g) * x) < 2e-6 and fence_ok(buf, n)


def test_sigmoid_gate_saturates_without_overflow():
    """exp(90) overflows float32: the gate at -90 is 1 / inf = 0, at +90 it is 1 / (1 + 0) = 1."""
    g = np.array([90.0, -90.0, 90.0, -90.0, 0.0], dtype=np.float64)
    x = np.array([1.5, 1.5, -3.25e5, -3.25e5, 2.0], dtype=np.float64)
    yd = torch.full((5,), 7.0, device=DEV)
    L.sigmoid_gate(dev(g), dev(x), yd)
    got = host(yd)
    assert np.isfinite(got).all()
    assert got[0] == 1.5 and got[2] == -3.25e5
    assert abs(got[1]) <= 1e-30 and abs(got[3]) <= 1e-30
    assert got[4] == 1.0
    assert relerr(got, R.sigmoid(g) * x) < 2e-6


@pytest.mark.parametrize('rows,cols', [(1, 1), (7, 5), (300, 33)])
def test_copy2d_between_padded_arrays(rows, cols):
    rng = np.random.default_rng(rows)
    lds, ldd = cols + 3, cols + 2
    src = rng.standard_normal((rows, lds)).astype(F32)
    sd = dev(src); dd = torch.full((rows + 1, ldd), 7.0, device=DEV)
    L.check(L.load().dep_copy2d(sd.data_ptr(), lds, dd.data_ptr(), ldd, rows, cols, L.stream()), 'dep_copy2d')
    got = bits(dd)
    assert np.array_equal(got[:rows, :cols], src[:, :cols])
    assert np.all(got[:rows, cols:] == 7.0) and np.all(got[rows:] == 7.0)
    assert np.array_equal(bits(sd), src)
