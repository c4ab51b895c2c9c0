"""The shapes at which the event <-> k-mer pre-alignment is checked, one list for the CPU tests (oracle against the plain
reference, tests/test_oracle_event_align.py) and the GPU tests (kernel against the oracle, tests/test_gpu_event_align.py).

Every 6-mer case is cut from ONE synthetic read, synth.make_read(7, 6000, ...): its sequence, its event means and its
base-to-event map.  make_read's n_events is a target, so exact sizes are set by slicing.  A case is
(label, sequence, event_mean, scale, shift, var); scale and shift are the method-of-moments scalings unless the case
says otherwise.  The numbers are those at which k_event_align (signalalign_amd/csrc/sa_ea.hip) changes what it does:
  * the band is 100 offsets on 64 lanes: rep 0 holds k-mers 0..12 and the initial load k-mers 0..48 of band 1;
  * the k-mer stream starts at k-mer 49 and refills at 113 and 177; the event stream starts at event 51 and refills at
    115 and 179;
  * the traceback stages 64 bands at a time and starts near band n_events + n_kmers;
  * the status bits flip at 50 / 51 skipped k-mers in a row and at 5 events per k-mer.
"""
import functools

import numpy as np

from signalalign_amd import synth
from oracle import sa_oracle_py as oracle

import sa_cases

MATCHED_KMERS = (1, 2, 3, 12, 13, 14, 48, 49, 50, 51, 63, 64, 65, 99, 100, 101, 112, 113, 114, 176, 177, 178)
EXACT_EVENTS = (1, 2, 3, 49, 50, 51, 52, 63, 64, 65, 99, 100, 101, 114, 115, 116, 178, 179, 180)
BLOCK_SUMS = tuple(range(61, 67)) + tuple(range(125, 131))
ONE_EVENT_KMERS = (2, 51, 52, 53, 295)
RNA_KMERS = (1, 2, 49, 50, 113, 114)
MAX_REF_CELLS = 150000    # the plain reference fills the whole matrix: cases above this are checked on the GPU only


@functools.lru_cache(maxsize=None)
def oracle_model(model_path):
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    return oracle.Model(alpha, k, t10, tab), tab


def _mom(om, seq, ev, rna=False):
    sh, sc = oracle.scalings_mom(om, ev, oracle.kmer_ids_of(om, seq, rna=rna))
    return sc, sh


@functools.lru_cache(maxsize=None)
def cases_6mer():
    alpha, k, t10, tab = synth.parse_model_table(sa_cases.MODEL_6MER)
    om = oracle.Model(alpha, k, t10, tab)
    r = synth.make_read(7, 6000, alpha, k, tab)
    ref = r["ref"]
    means = np.ascontiguousarray(np.asarray(r["events4"])[:, 0])
    emap = np.asarray(r["event_map"])
    out = []

    def seq_of(n_kmers, first=0):
        return ref[first:first + n_kmers + k - 1]

    def add(label, seq, ev, scale=None, shift=None, var=1.0):
        ev = np.ascontiguousarray(ev, dtype=np.float64)
        if scale is None:
            scale, shift = _mom(om, seq, ev)
        out.append((label, seq, ev, float(scale), float(shift), float(var)))

    def matched(n_kmers):
        return seq_of(n_kmers), means[:max(int(emap[n_kmers]), 1)]

    def own_events(i, count):   # `count` events of k-mer i: its own events, repeated
        a, b = int(emap[i]), int(emap[i + 1])
        assert b > a, "k-mer %d of the read has no event of its own" % i
        return np.resize(means[a:b], count)

    for n in MATCHED_KMERS:
        add("matched_%dk" % n, *matched(n))
    for n in EXACT_EVENTS:
        add("events_%d" % n, seq_of(max(int(n / 1.6), 1)), means[:n])
    for s in BLOCK_SUMS:
        for n_kmers in (s // 3, s // 2):
            add("block_%d_%dk" % (s, n_kmers), seq_of(n_kmers), means[:s - n_kmers])
    add("one_by_one", seq_of(1), means[:1])
    for n in ONE_EVENT_KMERS:
        add("one_event_%dk" % n, seq_of(n), means[:1], scale=1.0, shift=0.0)
    for n in (5, 6, 400):
        add("per_kmer_%dx1" % n, seq_of(1), own_events(0, n))
    for n_kmers in (2, 7):
        # k-mers with events of their own (a skipped k-mer has none to repeat): the first n_kmers consecutive ones
        first = next(i for i in range(len(emap) - n_kmers - k) if all(emap[j + 1] > emap[j] for j in range(i, i + n_kmers)))
        five = np.concatenate([own_events(first + i, 5) for i in range(n_kmers)])
        add("per_kmer_%dx%d" % (5 * n_kmers, n_kmers), seq_of(n_kmers, first), five)
        add("per_kmer_%dx%d" % (5 * n_kmers + 1, n_kmers), seq_of(n_kmers, first),
            np.concatenate([five, own_events(first + n_kmers - 1, 1)]))
    # reads that do not fit their sequence
    rng = np.random.default_rng(5)
    seq, ev = matched(479)
    sc, sh = _mom(om, seq, ev)
    add("noise_800x479", seq, rng.uniform(40, 140, 800), scale=sc, shift=sh)
    add("short_300x1824", seq_of(1824), means[:300])
    add("long_2983x195", seq_of(195), means[:2983])
    add("long_600x55", seq_of(55), means[:600])
    for n_ev, n_kmers in ((300, 187), (500, 312), (300, 50), (800, 150)):
        half = n_ev // 2
        noise = np.random.default_rng(5).uniform(40, 140, n_ev - half)
        add("half_noise_%dx%d" % (n_ev, n_kmers), seq_of(n_kmers), np.concatenate([means[:half], noise]))
    # one absurd (finite) event in the middle of a matched read, scalings of the read without it: from that row on the
    # float scores are near -1e11 and the transition terms round away (rejected by the average emission: word 1)
    for n in (48, 100, 177):
        seq, ev = matched(n)
        sc, sh = _mom(om, seq, ev)
        ev = ev.copy()
        ev[len(ev) // 2] = 1e6
        add("outlier_%dk" % n, seq, ev, scale=sc, shift=sh)
    for n, var in ((100, 1.3), (177, 0.8)):
        seq, ev = matched(n)
        add("matched_%dk_var%g" % (n, var), seq, ev, var=var)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases_rna():
    """The 5-mer model with SA_FLAG_RNA (U reads as T, every k-mer reversed), events drawn for the reversed k-mers as
    test_rna_kmer_list draws them; cut from one read by k-mer count."""
    alpha, k, t10, tab = synth.parse_model_table(sa_cases.MODEL_5MER)
    om = oracle.Model(alpha, k, t10, tab)
    r = synth.make_read(4242, 700, alpha, k, tab)
    seq = r["ref"].replace("T", "U")
    ids = oracle.kmer_ids_of(om, seq, rna=True)
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 3, size=len(ids))
    owner = np.repeat(np.arange(len(ids)), counts)
    ev = rng.normal(tab[5 * ids[owner]], tab[5 * ids[owner] + 1])
    first = np.cumsum(counts) - counts
    out = []
    for n in RNA_KMERS:
        s, e = seq[:n + k - 1], np.ascontiguousarray(ev[:first[n]])
        sc, sh = _mom(om, s, e, rna=True)
        out.append(("rna_%dk" % n, s, e, float(sc), float(sh), 1.0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(which):
    """event_align_ex of every case of cases_6mer() ("6mer") or cases_rna() ("rna"): (k-mer idx, event idx, status, fills,
    walk flags) per case, computed once and shared."""
    rna = which == "rna"
    om, _ = oracle_model(sa_cases.MODEL_5MER if rna else sa_cases.MODEL_6MER)
    out = []
    for label, seq, ev, scale, shift, var in (cases_rna() if rna else cases_6mer()):
        om.set_read_params(scale, shift, var)
        res = oracle.event_align_ex(om, ev, oracle.kmer_ids_of(om, seq, rna=rna))
        for a in res[:2]:
            a.setflags(write=False)
        out.append(res)
    return tuple(out)
