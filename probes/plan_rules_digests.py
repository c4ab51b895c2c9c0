#!/usr/bin/env python3
"""Digests (sa.plan_digest: every array of a host plan, no GPU needed) of a fixed, seeded set of batches, one line per case.
Run it on two checkouts and compare the lines: a planner refactor must leave every one of them equal.
    python probes/plan_rules_digests.py > digests.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import signalalign_amd as sa  # noqa: E402
from signalalign_amd import synth  # noqa: E402
import sa_cases as cases  # noqa: E402
import test_gpu_dplan  # noqa: E402  (for _mixed_jobs: importing it runs nothing on a GPU)

FLAG_EXPECT_INTERNAL = 0x10000


def line(name, model, params, jobs, **kw):
    jobs = jobs * -(-16 // len(jobs))          # (the planner takes a thread per four reads: 16 reads for four threads)
    for threads in (1, 4):
        try:
            info, dig = sa.plan_digest(model, params, jobs, threads=threads, **kw)
            print("%-58s threads=%d %016x regions=%d fast=%d ring=%d segs=%d cks=%d" % (
                name, threads, dig, info.n_regions, info.n_fast_regions, info.n_ring_regions, info.n_segments, info.n_checkpoints))
        except sa.SaError as e:
            print("%-58s threads=%d error %s" % (name, threads, e))


def main():
    sa.build()
    pm = sa.Model.load(cases.MODEL_6MER)
    mixed = test_gpu_dplan._mixed_jobs()
    psets = (("default", sa.default_params()), ("e20_tb40", sa.default_params(expansion=20, trace_back=40)),
             ("thr0.5_e4", sa.default_params(threshold=0.5, expansion=4)))
    for pn, p in psets:
        line("mixed/" + pn, pm, p, mixed)
    p = sa.default_params()
    for var in ("SA_RING", "SA_RING_WIDE"):
        os.environ[var] = "0"
        line("mixed/%s=0" % var, pm, p, mixed)
        del os.environ[var]
    for fn, fl in (("EXACT", sa.FLAG_EXACT), ("FORCE_GENERIC", sa.FLAG_FORCE_GENERIC), ("EXPECT_INTERNAL", FLAG_EXPECT_INTERNAL)):
        line("mixed/flag_" + fn, pm, p, mixed, flags=fl)
    line("mixed/threshold0", pm, sa.default_params(threshold=0.0), mixed)

    # the ambiguity test's jobs: CpG X -> C/E, R7.3 L / P, with and without the HDP model
    pmc = sa.Model.load(cases.MODEL_CPG)
    amb = sa.default_ambig({"X": "CE"})
    cpg = cases.synthetic_jobs(cases.MODEL_CPG, 6, 1400, 20, cpg_ambiguous=True) + cases.synthetic_jobs(cases.MODEL_CPG, 2, 900, 3)
    sparse = cases.realistic_anchor_jobs(cases.MODEL_CPG, 2, 1200, 77)
    cpg += [dict(j, ref=j["ref"].replace("CG", "XG")) for j in sparse]
    line("cpg_X_CE", pmc, p, cpg, ambig=amb)
    line("cpg_X_CE/flag_EXPECT_INTERNAL", pmc, p, cpg, ambig=amb, flags=FLAG_EXPECT_INTERNAL)
    line("cpg_X_CC (options repeat)", pmc, p, cpg, ambig=sa.default_ambig({"X": "CC"}))
    os.environ["SA_RING"] = "0"
    line("cpg_X_CE/SA_RING=0", pmc, p, cpg, ambig=amb)
    del os.environ["SA_RING"]
    pm7 = sa.Model.load(cases.MODEL_R73)
    lp = []
    for j, job in enumerate(cases.synthetic_jobs(cases.MODEL_R73, 3, 600, 50)):
        ref = list(job["ref"])
        for i in range(7 + j, len(ref) - 6, 23):
            ref[i] = "L" if (i // 23) % 2 == 0 else "P"
        for i in (200, 201, 202):
            ref[i] = "L"
        lp.append(dict(job, ref="".join(ref)))
    line("r73_LP", pm7, p, lp)
    hd = sa.Model.load(cases.MODEL_R73, cases.NHDP)
    hd.set_to_hdp_expected_values()
    line("r73_LP/hdp", hd, p, lp)
    line("r73_LP/hdp/flag_EXPECT_INTERNAL", hd, sa.default_params(threshold=0.1), lp, flags=FLAG_EXPECT_INTERNAL)
    thin = cases.realistic_anchor_jobs(cases.MODEL_R73, 3, 1500, 7)
    thin_l = thin + [dict(thin[0], ref=thin[0]["ref"].replace("CG", "LG"))]
    line("r73_thin+LG", pm7, p, thin_l)
    line("r73_thin+LG/hdp", hd, p, thin_l)
    line("r73_dense/hdp", hd, p, cases.synthetic_jobs(cases.MODEL_R73, 3, 900, 5))

    # a two-distribution model, with and without its ring / strip instances
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_6MER)
    wide = cases.realistic_anchor_jobs(cases.MODEL_6MER, 1, 1500, 31)[0]
    ambj = dict(cases.synthetic_jobs(cases.MODEL_6MER, 1, 600, 32)[0])
    ambj["ref"] = ambj["ref"][:100] + "X" + ambj["ref"][101:]
    many = dict(cases.synthetic_jobs(cases.MODEL_6MER, 1, 600, 33)[0])
    many["ref"] = many["ref"].replace("CG", "XG")          # rows of more than SA_RING_MAX_ROWPATHS cell-paths, if any
    two = [wide, ambj, many] + cases.synthetic_jobs(cases.MODEL_6MER, 2, 900, 34)
    for emission in (1, 2):
        m = sa.Model.create(alpha, k, t10, tab)
        m.set_emission(emission)
        for fn, fl in (("flags0", 0), ("TWO_DIST_ALL_KERNELS", sa.FLAG_TWO_DIST_ALL_KERNELS)):
            line("two_dist%d/%s" % (emission, fn), m, p, two, ambig=sa.default_ambig({"X": "CT"}), flags=fl)
            line("two_dist%d/%s/X_ACGT" % (emission, fn), m, p, [many], flags=fl)
        m.close()

    # a gap that splits the matrix
    big = synth.make_read(7, 14000, alpha, k, tab)
    hole = (big["ax"] > 1500) & (big["ax"] < 6500)
    big["ax"], big["ay"] = big["ax"][~hole], big["ay"][~hole]
    dense = cases.synthetic_jobs(cases.MODEL_6MER, 3, 900, 5)
    line("split_gap", pm, p, dense + [big])
    line("split_gap/not_ragged", pm, p, [dict(big, ragged=(1, 1))] + dense)

    # jobs the planner rejects: the error must stay what it is, whatever the thread count
    bad_var = dict(dense[0], var=0.0)
    line("reject/var0", pm, p, dense * 2 + [bad_var] + dense * 2)
    out = dict(dense[0], ax=np.array([5, 3], dtype=np.int64), ay=np.array([5, 9], dtype=np.int64))
    line("reject/anchors", pm, p, dense * 2 + [out] + dense * 2)
    line("reject/var0_then_anchors", pm, p, dense * 2 + [bad_var, out] + dense * 2)
    line("reject/anchors_then_var0", pm, p, dense * 2 + [out, bad_var] + dense * 2)
    line("reject/letter", pm, p, dense * 2 + [dict(dense[0], ref=dense[0]["ref"][:50] + "N" + dense[0]["ref"][51:])] + dense * 2)


if __name__ == "__main__":
    main()
