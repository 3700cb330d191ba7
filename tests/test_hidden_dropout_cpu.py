"""The numpy statement of the hidden-state dropout generator (oracle/hidden_dropout.py) on its own, no GPU: its drop rate and the
p = 0 case.  tests/test_glue_ops_gpu.py pins kzv_debug_dropout_mask and every kernel that draws these masks against it."""
import numpy as np
import pytest

from oracle import hidden_dropout as HD
from oracle.attn_dropout import thr16_of


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("key,ld_extra", [(0, 0), (0xdeadbeef, 0), (12345, 4)])
def test_drop_rate_matches_the_threshold(p, key, ld_extra):
    """2^20 elements: the fraction dropped is within 4 sigma of thr16 / 65536 (binomial), and the kept multiplier is 1 / P(keep)."""
    rows, cols = 1024, 1024
    m = HD.multiplier(key, p, rows, cols, cols + ld_extra)
    assert m.dtype == np.float32 and m.shape == (rows, cols)
    q = thr16_of(p) / 65536.0
    n = rows * cols
    sigma = (q * (1 - q) / n) ** 0.5
    frac = float((m == 0).mean())
    assert abs(frac - q) <= 4 * sigma, (frac, q, sigma)
    kept = np.unique(m[m != 0])
    assert kept.size == 1 and kept[0] == np.float32(65536.0) / np.float32(65536 - thr16_of(p))


def test_p_zero_keeps_everything():
    assert np.array_equal(HD.multiplier(77, 0.0, 33, 20, 20), np.ones((33, 20), dtype=np.float32))


def test_the_index_is_row_times_ld_plus_col():
    """A [rows, cols] window of a wider index space is the same window of the full mask (what `ld_index` means), and two elements of
    one pair take the two halves of one hash."""
    full = HD.bits16(9, 6, 20, 20)
    assert np.array_equal(HD.bits16(9, 6, 12, 20), full[:, :12])
    x = HD.hash32((np.arange(60, dtype=np.uint32) * np.uint32(0x9E3779B9)) + np.uint32(9))
    assert np.array_equal(full.reshape(-1)[0::2], x & 0xffff) and np.array_equal(full.reshape(-1)[1::2], x >> 16)
