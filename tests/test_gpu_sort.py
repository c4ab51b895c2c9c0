"""sa_sort_u64 (the device-wide radix sort under sa_call_scores_finish) equals np.sort exactly: around the tile size, on inputs that
run every pass or none, on the bit patterns of scores."""
import numpy as np
import pytest

import signalalign_amd as sa

pytestmark = pytest.mark.gpu

T = sa.SORT_TILE


def _check(keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    before = keys.copy()
    got = sa.sort_u64(keys)
    assert keys.tobytes() == before.tobytes()                    # the input is only read
    assert got.dtype == np.uint64 and got.tobytes() == np.sort(before).tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1])
def test_sizes_around_the_tile(n):
    rng = np.random.default_rng(n)
    _check(rng.integers(0, 2**64, n, dtype=np.uint64))


def test_two_hundred_thousand_keys():
    rng = np.random.default_rng(7)
    st = {}
    keys = rng.integers(0, 2**64, 200003, dtype=np.uint64)
    assert sa.sort_u64(keys, stats=st).tobytes() == np.sort(keys).tobytes()
    assert st["kernel_ms"] > 0


def test_all_keys_equal():
    _check(np.full(2 * T + 5, 0x3FE0000000000000, dtype=np.uint64))   # no pass runs


@pytest.mark.parametrize("byte", [0, 3, 7])
def test_keys_that_differ_in_one_byte_only(byte):
    rng = np.random.default_rng(byte)
    v = rng.integers(0, 256, 3 * T + 17, dtype=np.uint64)
    _check(np.uint64(0x0123456789ABCDEF & ~(0xFF << (8 * byte))) | (v << np.uint64(8 * byte)))


def test_each_pass_must_keep_the_order_of_the_pass_before():
    """two digits only: the upper one has few values, so long runs of equal upper digits must stay in lower-digit order"""
    rng = np.random.default_rng(11)
    n = 5 * T + 3
    _check((rng.integers(0, 3, n, dtype=np.uint64) << np.uint64(8)) | rng.integers(0, 256, n, dtype=np.uint64))


def test_ascending_and_descending_input():
    rng = np.random.default_rng(13)
    s = np.sort(rng.integers(0, 2**64, 2 * T + 100, dtype=np.uint64))
    _check(s)
    _check(s[::-1])


def test_bit_patterns_of_scores():
    rng = np.random.default_rng(17)
    v = rng.random(3 * T + 9)
    v[:6] = [0.0, 5e-324, 1.0, 1.0, 0.0, 2.2250738585072014e-308]
    _check(v.view(np.uint64))
    got = sa.sort_u64(v.view(np.uint64)).view(np.float64)
    assert got.tobytes() == np.sort(v).tobytes()                 # non-negative doubles order as their bit patterns
    six = np.round(rng.random(4 * T + 1), 6)                     # six decimals: ties abound
    assert len(np.unique(six)) < len(six)
    _check(six.view(np.uint64))


def test_arguments():
    L = sa.lib()
    k = np.arange(4, dtype=np.uint64)
    assert L.sa_sort_u64(k.ctypes.data, -1, k.ctypes.data, 0, None) == -1      # SA_EINVAL
    assert L.sa_sort_u64(None, 4, k.ctypes.data, 0, None) == -1
    assert L.sa_sort_u64(k.ctypes.data, 4, k.ctypes.data, 99, None) == -1      # no such device
    assert L.sa_sort_u64(None, 0, None, 0, None) == 0
