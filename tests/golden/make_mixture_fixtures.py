"""Writes tests/golden/mixture/: sklearn's fits of the CPU cases of tests/kmer_mixture_ref.py (sklearn_fits.npz) and the k-mer
pairs the reference's own get_motif_kmer_pairs gives (motif_pairs.json).

    python tests/golden/make_mixture_fixtures.py <root of a signalAlign checkout>

Needs scikit-learn and, for the pairs, the reference's Python sources (src/signalalign/mixture_model.py and
utils/sequenceTools.py).  The two modules import plotting and helper packages that need not be installed, so the five
functions used are compiled from the files' text on their own; the one helper they take from py3helpers
(all_string_permutations: every string of a length over an alphabet) is supplied here.  Run on a CPU machine, by hand, when
the cases change; the tests only read what it wrote."""
import ast
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmer_mixture_ref as ref   # noqa: E402

MOTIF_CASES = [(5, "CCAGG", "CEAGG", "ATGC"), (6, "CCAGG", "CEAGG", "ATGC"), (5, "CCTGG", "CETGG", "ATGC"),
               (6, "CCTGG", "CETGG", "ATGC"), (5, "GATCCAGGTA", "GATCEAGGTA", "ATGC"), (3, "CCAGG", "CEAGG", "ATGC"),
               (6, "CCAGG", "CEAGG", "ACEGT"), (4, "AC", "EC", "ACGT")]


def functions_of(path, names):
    tree = ast.parse(open(path).read())
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in picked) == sorted(names), path
    return ast.Module(body=picked, type_ignores=[])


def reference_pairs(root):
    ns = {"all_string_permutations": lambda alphabet, length: ("".join(p) for p in itertools.product(alphabet, repeat=length))}
    src = os.path.join(root, "src", "signalalign")
    for path, names in ((os.path.join(src, "utils", "sequenceTools.py"),
                         ["find_different_char_index", "find_modification_index_and_character", "get_front_back_kmer_overlap",
                          "get_motif_kmers"]),
                        (os.path.join(src, "mixture_model.py"), ["get_motif_kmer_pairs"])):
        exec(compile(functions_of(path, names), path, "exec"), ns)
    out = []
    for k, can, mod, alphabet in MOTIF_CASES:
        pairs = sorted(set(tuple(p) for p in ns["get_motif_kmer_pairs"]([can, mod], k, alphabet=alphabet)))
        out.append(dict(k=k, canonical=can, modified=mod, alphabet=alphabet, pairs=[list(p) for p in pairs]))
    return out


def main():
    out_dir = os.path.join(HERE, "mixture")
    os.makedirs(out_dir, exist_ok=True)
    z = {}
    for name, x, K, max_iter, tol in ref.host_cases():
        w, m, s, n_iter, conv, lb = ref.sklearn_fit(x, K, max_iter, tol)
        z[name + "_weight"], z[name + "_mean"], z[name + "_sd"] = w, m, s
        z[name + "_iter"] = np.array([n_iter, conv], dtype=np.int64)
        z[name + "_lb"] = np.array([lb])
    np.savez_compressed(os.path.join(out_dir, "sklearn_fits.npz"), **z)
    if len(sys.argv) > 1:
        with open(os.path.join(out_dir, "motif_pairs.json"), "w") as f:
            json.dump(reference_pairs(sys.argv[1]), f, indent=0)
            f.write("\n")


if __name__ == "__main__":
    main()
