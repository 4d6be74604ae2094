"""The oracle's own Philox4x32-10 and dropout mask (oracle/ref_numpy.py), pinned without a GPU: the published known-answer
vectors, and the properties a keep mask has whatever the generator.  tests/test_small_kernels_gpu.py then holds the device
draw (csrc/dep_common.h) to this oracle bit for bit."""
import numpy as np
import pytest

from oracle import ref_numpy as R

# Known-answer vectors of Philox4x32-10 (the Random123 distribution's kat_vectors): counter, key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SEED, SITE = (7 << 32) | 99, 17


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [hex(int(w)) for w in got] == [hex(w) for w in want]


def test_philox_is_vectorised_over_counters_and_keys():
    """All three vectors in one call (every word an array) give the rows the scalar calls give."""
    ctr = [np.array([k[0][i] for k in KAT]) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT]) for i in range(2)]
    got = R.philox4x32_10(ctr, key)
    assert got.shape == (3, 4)
    assert np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint32))
    # a scalar key broadcasts against an array of counters
    one = R.philox4x32_10((np.arange(5), 0, 3, 9), (11, 12))
    for g in range(5):
        assert np.array_equal(one[g], R.philox4x32_10((g, 0, 3, 9), (11, 12)))


def test_dropout_mask_follows_the_stated_convention():
    """Element 4g + i is word i of the block with counter (g, 0, site, 0x2545F491) under key (seed lo, seed hi)."""
    p = np.float32(0.3)
    m = R.dropout_mask(11, 0.3, SEED, SITE)
    scale = np.float32(1) / (np.float32(1) - p)
    for e in range(11):
        w = int(R.philox4x32_10((e // 4, 0, SITE, 0x2545F491), (99, 7))[e % 4])
        u = np.float32(w >> 8) * np.float32(2.0 ** -24)
        assert 0.0 <= u < 1.0
        assert m[e] == (scale if u >= p else np.float32(0)), e


@pytest.mark.parametrize('p', [0.3, 0.5, 0.999])
def test_dropout_mask_values_are_zero_or_the_scale(p):
    m = R.dropout_mask(4099, p, SEED, SITE)
    assert m.dtype == np.float32 and m.shape == (4099,)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    assert set(np.unique(m).tolist()) == {0.0, float(scale)}


def test_dropout_mask_p0_keeps_everything():
    assert np.array_equal(R.dropout_mask(1027, 0.0, SEED, SITE), np.ones(1027, np.float32))


def test_dropout_mask_sites_and_seeds_are_separate_streams():
    base = R.dropout_mask(4096, 0.5, SEED, SITE)
    for seed, site in ((SEED, SITE + 1), (SEED, 0), (SEED + 1, SITE), (99, SITE), ((8 << 32) | 99, SITE)):
        other = R.dropout_mask(4096, 0.5, seed, site)
        # independent fair masks agree on about half the elements (sd 32 of 4096): far from equal, far from complementary
        agree = int((other == base).sum())
        assert 2048 - 6 * 32 < agree < 2048 + 6 * 32, (seed, site, agree)


def test_dropout_mask_prefix_does_not_depend_on_n():
    full = R.dropout_mask(70001, 0.3, SEED, SITE)
    for n in (1, 3, 4, 5, 255, 256, 257, 1027):
        assert np.array_equal(R.dropout_mask(n, 0.3, SEED, SITE), full[:n]), n
    assert R.dropout_mask(0, 0.3, SEED, SITE).shape == (0,)


@pytest.mark.parametrize('p', [0.3, 0.5])
def test_dropout_mask_kept_fraction(p):
    n = 70001
    kept = float((R.dropout_mask(n, p, SEED, SITE) != 0).mean())
    assert abs(kept - (1 - p)) < 4 * np.sqrt(p * (1 - p) / n), kept
