"""SA_FLAG_TWO_DIST_ALL_KERNELS and sa_batch_create_noise_scaled: what can be said about them without a GPU."""
import os
import re

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth, _capi

import sa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_constants_of_the_header_and_the_python_mirror_agree():
    hdr = open(os.path.join(ROOT, "include", "signalalign_hip.h")).read()
    flags = {name: int(value) for name, value in re.findall(r"#define\s+SA_FLAG_([A-Z0-9_]+)\s+(\d+)u", hdr)}
    assert flags["TWO_DIST_ALL_KERNELS"] == 512
    assert len(set(flags.values())) == len(flags)                      # one bit each
    assert all(v & (v - 1) == 0 for v in flags.values())
    mirrored = {name[5:]: getattr(_capi, name) for name in dir(_capi) if name.startswith("FLAG_")}
    assert "TWO_DIST_ALL_KERNELS" in mirrored and sa.FLAG_TWO_DIST_ALL_KERNELS == 512
    for name, value in mirrored.items():
        assert flags[name] == value, name
    assert set(flags) - set(mirrored) <= {"RNA"}                       # (event alignment's flag: passed by number there)


def test_noise_scaled_batches_are_exported_and_refuse_without_a_device():
    assert "sa_batch_create_noise_scaled" in _capi.EXPORTS and hasattr(sa.lib(), "sa_batch_create_noise_scaled")
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_5MER)
    m = sa.Model.create(alpha, k, t10, tab)
    m.set_emission(1)
    ev = np.array([[60.0, 1.0, 0.01, 0.0], [61.0, 1.1, 0.01, 0.01]])
    job = dict(ref="ACGTACGTACGT", events=ev, ax=[], ay=[], scale=1.0, shift=0.0, var=1.0)
    with pytest.raises(sa.SaError) as ei:
        # (on a machine with a GPU the call gets as far as its arguments: no flag, SA_EINVAL)
        sa.Batch(m, sa.default_params(), [job], flags=0, noise=[(1.0, 1.0)])
    assert ei.value.code == (-3 if sa.device_count() == 0 else -1)
    with pytest.raises(ValueError):
        sa.Batch(m, sa.default_params(), [job], flags=sa.FLAG_TWO_DIST_ALL_KERNELS, noise=[(1.0, 1.0), (1.0, 1.0)])
    # the Python wrapper of sa_model_clone_with_table: the same model with another table
    t2 = np.array(tab, dtype=np.float64).copy()
    t2[2::5] *= 1.25
    c = m.clone_with_table(t2)
    assert c.alphabet() == m.alphabet() and np.array_equal(c.table5(), t2) and np.array_equal(m.table5(), tab)
    c.close(); m.close()
