"""Host side of the Gaussian emission training: Python's repr (the model writer's number format), the "%f" rounding the
table's units come from, sa_model_write_trained against a restatement of train_normal_emmissions + HmmModel.write, and the
reference's own assignments file through the restated top-N selection."""
import gzip
import math
import os
import struct

import numpy as np
import pytest

import signalalign_amd as sa

import kmer_training_ref as ref
import sa_cases as cases

FIXTURE = os.path.join(cases.GOLDEN, "hdp", "d6160b0b-a35e-43b5-947f-adaa1abade28.sm.assignments.tsv.gz")


def _doubles(n, seed):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2**63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    v = [float(x) for x in bits.view(np.float64)]
    v += [float(x) for x in rng.standard_normal(n) * 10.0 ** rng.integers(-12, 20, n)]
    return [x for x in v if not math.isnan(x)]


def test_repr_formatter_equals_python_repr():
    vals = _doubles(450000, 7)
    vals += [2.0**e for e in range(-1074, 1024)] + [-(2.0**e) for e in range(-60, 60)]
    vals += [float(i) for i in range(-2000, 2000)] + [i / 1000 for i in range(-5000, 5000)]
    vals += [5e-324, 1.7976931348623157e308, 1e16, 1e15, 9999999999999998.0, 1e-4, 1e-5, 0.0001, 0.00001, 1e22, 1e23, 0.1, 0.2,
             0.3, 2.0 / 3, -0.0, 0.0, float("inf"), float("-inf"), 86.9596, 1e-09, 123456789012345680.0]
    assert len(vals) > 900000
    bad = [v for v in vals if sa.format_py_repr(v) != repr(v)]
    assert not bad, [(v, sa.format_py_repr(v), repr(v)) for v in bad[:5]]


def test_host_f6_units_equal_printf():
    rng = np.random.default_rng(3)
    vals = list(rng.uniform(-300, 300, 100000)) + [(2 * i + 1) / 128 for i in range(-2000, 2000)]   # odd multiples of 1/128: ties
    vals += [0.0, -0.0, -1e-9, 1e-9, -4e-7, 5e-7, -5e-7, 2147483647.5, -2147483647.9]
    for v in vals:
        u, nz, rc = sa.f6_units(float(v))
        assert rc == 0
        assert (u, nz) == ref.units("%f" % v), v
    assert sa.f6_units(2.0**31)[2] == -8 and sa.f6_units(float("nan"))[2] == -8


def _random_stats(nk, seed, with_median):
    rng = np.random.default_rng(seed)
    st = np.zeros(nk, dtype=sa.KMER_STAT_DTYPE)
    for km in range(nk):
        if rng.random() < 0.4:
            continue
        vals = list(rng.integers(60_000_000, 130_000_000, int(rng.integers(1, 40))))
        st[km] = ref.stats(vals, with_median)
    return st


@pytest.mark.parametrize("use_median", [False, True])
@pytest.mark.parametrize("variant", ["plain", "mod_only", "kmer_list", "min_sd"])
def test_model_writer_equals_the_restatement(tmp_path, use_median, variant):
    prior = cases.MODEL_CPG if variant == "mod_only" else cases.MODEL_6MER
    head, _, params = ref.read_model(prior)
    alphabet, k = head[2], int(head[3])
    nk = len(params) // 5
    st = _random_stats(nk, 11 + (variant == "mod_only"), use_median)
    kw = dict(weight=100.0, min_sd=0.0, mod_only=False)
    mask, names = None, None
    if variant == "mod_only":
        kw["mod_only"] = True
    elif variant == "kmer_list":
        rng = np.random.default_rng(5)
        mask = (rng.random(nk) < 0.3).astype(np.uint8)
        names = {ref.kmer_name(i, alphabet, k) for i in np.nonzero(mask)[0]}
    elif variant == "min_sd":
        kw["min_sd"], kw["weight"] = 1.6, 7.5
    out, exp = tmp_path / "got.model", tmp_path / "exp.model"
    sa.model_write_trained(prior, st, str(out), kmer_mask=mask, **kw)
    ref.write_trained(prior, {i: tuple(st[i]) for i in range(nk)}, str(exp), kmers=names, **kw)
    got_b, exp_b = out.read_bytes(), exp.read_bytes()
    assert got_b == exp_b
    # untouched k-mers print their prior's tokens as str(float(token))
    with open(prior) as f:
        f.readline(), f.readline()
        toks = f.readline().split()
    got_toks = got_b.decode().split("\n")[2].split("\t")
    untouched = [i for i in range(nk) if st[i]["n"] == 0]
    assert untouched
    for i in untouched[:50]:
        assert got_toks[5 * i:5 * i + 5] == [str(float(t)) for t in toks[5 * i:5 * i + 5]]
    if variant == "mod_only":   # only k-mers holding E changed
        changed = [i for i in range(nk) if got_toks[5 * i] != str(float(toks[5 * i]))]
        assert changed and all("E" in ref.kmer_name(i, alphabet, k) for i in changed)


def fixture_rows():
    with gzip.open(FIXTURE, "rt") as f:
        return [ln.split() for ln in f if ln.strip()]


def test_reference_assignments_through_the_host_steps(tmp_path):
    """The reference's test file read twice, N = 1, min_prob 0 (test_trainModels.py:181-203): the restated selection keeps 3182
    rows, and the library's host steps on those real rows -- the "%f" units of every printed value, the k-mer ids, the model
    writer on their statistics (mean / sd and median / MAD) -- agree with the restatement byte for byte."""
    m = sa.Model.load(cases.MODEL_6MER)
    raw = fixture_rows()
    assert len(raw) == 17350 and {r[1] for r in raw} == {"t"}
    for r in raw:
        for text in (r[2], r[3]):
            u, nz, rc = sa.f6_units(float(text))
            assert rc == 0 and (u, nz) == ref.units(text), text
    kid = {r[0]: m.kmer_id(r[0]) for r in raw}
    assert all(ref.kmer_name(v, "ACGT", 6) == name for name, v in kid.items())
    rows = [(r[1], kid[r[0]], r[2], r[3]) for r in raw] * 2
    kept = ref.top_n(rows, 1, 0.0)
    assert sum(len(v) for v in kept.values()) == 3182
    kept10 = ref.top_n(rows, 10, 0.0)
    for v in kept10.values():   # within each k-mer the posteriors do not increase (test_trainModels.py:108-115, :132-142)
        p = [float(r[3]) for r in v]
        assert p == sorted(p, reverse=True)
    for med in (False, True):
        st = np.zeros(4096, dtype=sa.KMER_STAT_DTYPE)
        for (_, km), v in kept10.items():
            st[km] = ref.stats([ref.units(r[2])[0] for r in v], med)
        got, want = tmp_path / "got.model", tmp_path / "want.model"
        sa.model_write_trained(cases.MODEL_6MER, st, str(got))
        ref.write_trained(cases.MODEL_6MER, {i: tuple(st[i]) for i in range(4096)}, str(want))
        assert got.read_bytes() == want.read_bytes()
