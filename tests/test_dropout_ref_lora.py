"""CPU: the numpy twin of the LoRA dropped-flag generator (oracle/dropout_ref.py: lora_words / lora_keep) is consistent with itself --
the bit-sliced words equal a plain per-element evaluation of the same 15-bit comparison, the threshold follows the documented rounding,
row0 shifts the rows, planes and seeds are independent streams, and the dropped rate is binomial around thr15 / 2^15.  The GPU half
(tests/test_gpu_lora_f64.py) compares these words with ur_lora_dropout_bits byte for byte."""
import numpy as np
import pytest

from oracle import dropout_ref as D

PS = [0.1, 0.25, 0.3, 0.5, 2.0 ** -15, 0.99999]


@pytest.mark.parametrize("p", PS + [0.0])
@pytest.mark.parametrize("W", [8, 40, 136])
def test_bit_sliced_words_equal_the_per_element_comparison(p, W):
    M, nad, seed, row0 = 37, 3, (0xABCD << 32) | 17, 5
    keep = D.lora_keep(seed, p, M, W, nad, row0)
    plain = D.lora_dropped_plain(seed, p, M, W, nad, row0)
    assert keep.shape == plain.shape == (nad, M, W) and keep.dtype == np.uint8
    assert np.array_equal(keep, 1 - plain)
    words = D.lora_words(seed, p, M, W, nad, row0)
    assert words.dtype == np.uint32 and words.shape == (nad, M, D.lora_bits_ld(W) // 4)
    assert not words[:, :, (W + 31) // 32:].any()                       # the padding words are zero


def test_p_zero_keeps_everything():
    assert D.lora_keep(3, 0.0, 9, 136, 2).all()
    assert not D.lora_words(3, 0.0, 9, 136, 2).any()


def test_threshold_rounding_and_clamp():
    assert D.lora_thr15(0.0) == 0
    assert D.lora_thr15(2.0 ** -15) == 1
    assert D.lora_thr15(0.5) == 16384 and D.lora_thr15(0.25) == 8192
    assert D.lora_thr15(0.1) == int(float(np.float32(0.1)) * 32768.0 + 0.5) == 3277
    assert D.lora_thr15(0.3) == 9830                                    # 9830.4 + 0.5 truncates
    assert D.lora_thr15(0.99999) == 32767 and D.lora_thr15(0.999999) == 32767
    assert D.lora_thr15(3277 / 32768.0 - 1e-5) == 3277                   # within half a step below: rounds up


@pytest.mark.parametrize("r", [1, 33, 2 ** 33])
def test_row0_shifts_the_rows(r):
    seed, p, W, nad, M = 99, 0.3, 136, 2, 7
    part = D.lora_keep(seed, p, M, W, nad, row0=r)
    if r < 1000:
        assert np.array_equal(part, D.lora_keep(seed, p, M + r, W, nad)[:, r:r + M])
    else:                                                               # too many rows to generate: the shift composes
        assert np.array_equal(part[:, 3:], D.lora_keep(seed, p, M - 3, W, nad, row0=r + 3))
        assert not np.array_equal(part, D.lora_keep(seed, p, M, W, nad))


def test_planes_and_seeds_are_different_streams():
    M, W, p = 64, 256, 0.3
    k = D.lora_keep(10, p, M, W, 4)
    for a in range(4):
        for b in range(a + 1, 4):
            assert 0.3 < (k[a] != k[b]).mean() < 0.55                    # independent: 2 p (1 - p) = 0.42
    for other in (11, 10 ^ 2, 10 | (1 << 32)):
        assert 0.3 < (k != D.lora_keep(other, p, M, W, 4)).mean() < 0.55


@pytest.mark.parametrize("p", PS)
def test_dropped_rate_is_binomial(p):
    M, W, nad = 512, 1024, 2
    n = M * W * nad
    q = D.lora_thr15(p) / 32768.0
    dropped = n - int(D.lora_keep(0x1234_5678_9ABC, p, M, W, nad).sum())
    assert abs(dropped - n * q) <= 5.0 * np.sqrt(n * q * (1.0 - q)), (dropped, n * q)


def test_token_packed_repack():
    seed, p, M, W, nad = 5, 0.3, 64, 40, 2
    words = D.lora_words(seed, p, M, W, nad)
    bt = D.lora_words_transposed(words, W)
    assert bt.shape == (nad, 2, 40) and bt.dtype == np.uint32
    keep = D.lora_keep(seed, p, M, W, nad)
    for (a, m, c) in [(0, 0, 0), (1, 37, 39), (0, 63, 9), (1, 8, 1)]:
        t = m % 32
        bit = 8 * (t // 8) + (t % 8) // 2 + 4 * (t % 2)
        assert (int(bt[a, m // 32, c]) >> bit) & 1 == 1 - int(keep[a, m, c])
