"""Writes tests/golden/call_quality/reference_cases.json: the outputs of signalAlign's own get_distance_from_guide_alignment
(src/signalalign/alignedsignal.py) and find_gaps_in_alignment_data (src/signalalign/visualization/plot_breaks_in_alignments.py) on
seeded small cases, both strands.  Run by hand against a signalAlign checkout (needs numpy and pandas):

    python tests/golden/make_call_quality_fixtures.py /path/to/signalAlign

The two functions are compiled on their own from the checkout's text with ast (the modules around them import what is not needed
here); only the cases' inputs and the recorded results are written.  A case is kept when the script's walk wraps to no row and
leaves no call without a delta; `own_row` says whether every call also has a guide row of its own, that is whether the script's
one-row-per-call walk and the rule "the row at the position, else the row before it" name the same rows."""
import ast
import json
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import call_quality_ref as ref     # noqa: E402

N_DRAWS = 800


def function_from(path, name, namespace):
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(node) == 1, (path, name)
    code = compile(ast.Module(body=node, type_ignores=[]), path, "exec")
    exec(code, namespace)
    return namespace[name]


def draw(rng):
    n_events = int(rng.integers(8, 22))
    lengths = rng.integers(1, 10, size=n_events)
    holes = np.where(rng.random(n_events) < 0.25, rng.integers(1, 45, size=n_events), 0)
    raw_start = np.cumsum(np.concatenate([[int(rng.integers(0, 50))], (lengths + holes)[:-1]]))
    x_sign = int(rng.choice([1, -1]))
    x0 = int(rng.integers(100, 1000))
    n_anchors = int(rng.integers(2, 7))
    ay = np.sort(rng.choice(n_events, size=n_anchors, replace=False))
    ax = np.cumsum(rng.integers(0, 4, size=n_anchors)) + int(rng.integers(0, 3))
    n_sites = int(rng.integers(1, 5))
    around = np.arange(max(int(ax[0]) - 1, 0), int(ax[-1]) + 2)      # mostly within the guide, now and then just outside it
    site_x = np.sort(rng.choice(around, size=min(n_sites, len(around)), replace=False))
    bands = []
    for _ in site_x:
        a = int(rng.integers(0, n_events))
        bands.append((a, min(n_events - 1, a + int(rng.integers(0, 4)))))
    n_path = int(rng.integers(1, n_events + 1))
    path_y = np.sort(rng.choice(n_events, size=n_path, replace=False))
    return dict(x_sign=x_sign, x0=x0, raw_start=[int(v) for v in raw_start], raw_length=[int(v) for v in lengths],
                ax=[int(v) for v in ax], ay=[int(v) for v in ay], site_x=[int(v) for v in site_x],
                band_y=[[a, b] for a, b in bands], path_y=[int(v) for v in path_y], min_gap=int(rng.choice([0, 3, 30])))


def main(checkout):
    ns = {"np": np, "pd": pd}
    distance = function_from(os.path.join(checkout, "src", "signalalign", "alignedsignal.py"), "get_distance_from_guide_alignment", ns)
    find_gaps = function_from(os.path.join(checkout, "src", "signalalign", "visualization", "plot_breaks_in_alignments.py"),
                              "find_gaps_in_alignment_data", ns)
    rng = np.random.default_rng(20261021)
    cases = []
    for _ in range(N_DRAWS):
        c = draw(rng)
        rs, rl, sign = c["raw_start"], c["raw_length"], c["x_sign"]
        # the calls in ascending reference_index, as the script sorts them, with their bands
        order = sorted(range(len(c["site_x"])), key=lambda q: sign * c["site_x"][q])
        xs = [c["site_x"][q] for q in order]
        walked = ref.script_walk_rows(c["ax"], xs, sign)
        if any(r is None or r < 0 for r in walked):
            continue
        rows = []
        for q in order:
            y0, y1 = c["band_y"][q]
            rows.append((c["x0"] + sign * c["site_x"][q], rs[y0], rs[y1] - rs[y0] + rl[y1]))
        data = pd.DataFrame(rows, columns=["position", "raw_start", "raw_length"])
        # the guide in event order: ascending reference_index on the plus strand, descending on the minus strand (the script
        # reverses it)
        guide = pd.DataFrame([(c["x0"] + sign * x, rs[y], rl[y]) for x, y in zip(c["ax"], c["ay"])],
                             columns=["reference_index", "raw_start", "raw_length"])
        out = distance(data, guide, reference_index_key="position", minus_strand=sign < 0)
        deltas = [float(v) for v in out["guide_delta"]]
        assert len(deltas) == len(xs) and not any(np.isnan(deltas))
        c["call_x"] = xs
        c["guide_delta"] = deltas
        c["own_row"] = walked == [ref.guide_row(c["ax"], x, sign) for x in xs]
        c["gaps"] = [int(g) for g in find_gaps([dict(raw_start=rs[y], raw_length=rl[y]) for y in c["path_y"]], min_gap=c["min_gap"])]
        cases.append(c)
    n_own = sum(1 for c in cases if c["own_row"])
    print("%d draws, %d kept, %d with a guide row of its own per call" % (N_DRAWS, len(cases), n_own))
    assert n_own >= 200
    out_dir = os.path.join(HERE, "call_quality")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "reference_cases.json"), "w") as fh:
        json.dump(dict(source="get_distance_from_guide_alignment, find_gaps_in_alignment_data", n_draws=N_DRAWS, cases=cases), fh,
                  separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
