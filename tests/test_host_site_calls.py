"""Host side of the per-site calls (sa_batch_site_calls, signalMachine --site-calls-aggregate): the float formatter of the
over-reads table and the ABI's record layout.  No GPU needed."""
import ctypes as C

import numpy as np

import signalalign_amd as sa
from signalalign_amd import _capi


def _fmt(v):
    buf = C.create_string_buffer(64)
    n = sa.lib().sa_format_py_round6(buf, float(v))
    s = buf.value.decode()
    assert n == len(s)
    return s


def _pandas_like(v):
    """what AggregateOverReadsFull.write_data prints for a value of _normalize_all_data (src/signalalign/variantCaller.py:404-410):
    pandas writes a float column through repr"""
    return repr(float(np.round(v, 6)))


def test_round6_formatter_on_every_grid_value():
    for k in range(0, 1_000_001):
        v = k / 1e6
        assert _fmt(v) == _pandas_like(v), k


def test_round6_formatter_off_the_grid():
    rng = np.random.default_rng(5)
    vals = list(rng.random(200_000)) + list(rng.random(20_000) * 1e-4) + [0.0, 1.0, 0.5, 1e-7, 4.99999e-7, 5e-7, 5.000001e-7,
                                                                          0.9999995, 0.99999949, 0.0001, 0.00009999951, 1 / 3, 2 / 3]
    # sums of per-read probabilities divided by their total, as the table forms them
    for n in (2, 3, 7, 10, 49):
        vals += list(rng.integers(0, 1_000_001, (2000, n)).sum(axis=1) / 1e6 / n)
    for v in vals:
        assert _fmt(v) == _pandas_like(v), repr(v)


def test_site_call_abi():
    L = sa.lib()
    for name in ("sa_batch_site_calls", "sa_format_py_round6"):
        assert hasattr(L, name)
    assert sa.FLAG_SITE_CALLS == 128 and _capi.SITE_MAX_LETTERS == 8
    S = _capi.SiteCall
    assert C.sizeof(S) == 4 + 4 + 8 + 64 + 64
    assert (S.x.offset, S.n_letters.offset, S.letters.offset, S.units.offset, S.prob.offset) == (0, 4, 8, 16, 80)
    assert _capi.SITE_CALL_DTYPE.itemsize == C.sizeof(S)
    assert [_capi.SITE_CALL_DTYPE.fields[f][1] for f in ("x", "n_letters", "letters", "units", "prob")] == [0, 4, 8, 16, 80]


def test_site_calls_on_a_null_batch_is_einval():
    """A batch cannot be created here (no GPU), but the entry point answers a NULL batch with SA_EINVAL rather than crashing."""
    L = sa.lib()
    cnt = C.c_int64()
    ptr = C.POINTER(_capi.SiteCall)()
    assert L.sa_batch_site_calls(None, 0, C.byref(ptr), C.byref(cnt), None) == -1
