"""Restatement, in plain Python, of the marginalisation of single-nucleotide probabilities over reads
(call_sites_with_marginal_probs / scan_for_proposals of scripts/variantCallingLib.py and group_sites_in_window of
scripts/jamison.py), written fresh for the tests of sa_snp_marginals_*.  Two deliberate differences from those scripts, both
stated in include/signalalign_hip.h: sites are grouped by (contig, position), and rows are taken in run order."""

LETTERS = "ACGT"


def in_order(call):
    """the rows of one add call -- (contig, pos, run, strand, direction, (pA, pC, pG, pT)) -- in the order they are summed:
    ascending run, within a run strand t (0) before c (1), otherwise as given (sorted() is stable)"""
    return sorted(call, key=lambda r: (r[2], r[3]))


def accumulate(calls, acc=None, reverse=False):
    """acc[(contig, pos)] = [fwd, bwd, depth] after the calls, one after the other; reverse: every call's rows backwards (only
    to show that the order matters)"""
    acc = {} if acc is None else acc
    for call in calls:
        rows = in_order(call)
        if reverse:
            rows.reverse()
        for contig, pos, _run, _strand, direction, p in rows:
            e = acc.setdefault((contig, pos), [[0, 0, 0, 0], [0, 0, 0, 0], 0])
            side = e[0] if direction else e[1]
            for l in range(4):
                side[l] += p[l]
            e[2] += 1
    return acc


def finish(acc, min_depth=1, ref_by_contig=None):
    """the reported sites in (contig, position) order: dicts with contig, pos, depth, fwd, bwd, prob, called, ref, is_proposal,
    delta"""
    out = []
    for (contig, pos) in sorted(acc):
        fwd, bwd, depth = acc[(contig, pos)]
        if depth < max(min_depth, 1):
            continue
        m = [fwd[0] + bwd[3], fwd[1] + bwd[2], fwd[2] + bwd[1], fwd[3] + bwd[0]]
        total = 0
        for v in m:
            total += v
        ref = ref_by_contig[contig][pos].upper() if ref_by_contig is not None else "N"
        site = dict(contig=contig, pos=pos, depth=depth, fwd=[float(v) for v in fwd], bwd=[float(v) for v in bwd], ref=ref)
        if total == 0:
            site.update(prob=[0.0] * 4, called="N", is_proposal=False, delta=0.0)
        else:
            prob = [v / total for v in m]
            best = prob.index(max(prob))
            site.update(prob=prob, called=LETTERS[best], is_proposal=ref in LETTERS and ref != LETTERS[best],
                        delta=max(prob) - prob[LETTERS.index(ref)] if ref in LETTERS else 0.0)
        out.append(site)
    return out


def group_sites(sites, window=6, keep_last=False):
    """group_sites_in_window over (pos, delta) pairs; keep_last: a trailing site that starts a group of its own is kept"""
    sites = sorted(sites)
    groups = []
    i = 0
    while i + 1 < len(sites) or (keep_last and i < len(sites)):
        g = [sites[i]]
        while i + 1 < len(sites) and sites[i + 1][0] - sites[i][0] < window:
            g.append(sites[i + 1])
            i += 1
        groups.append(g)
        i += 1
    out = []
    for g in groups:
        best = g[0]
        for s in g[1:]:
            if s[1] > best[1]:
                best = s
        out.append(best[0])
    return out


def marginals_file(sites, contig_names):
    return "".join("\t".join([contig_names[s["contig"]], str(s["pos"]), str(s["depth"])] + [repr(float(v)) for v in s["prob"]] +
                             [s["called"], s["ref"], repr(float(s["delta"]))]) + "\n" for s in sites)


def apply_calls(ref, sites, contig):
    out = list(ref)
    for s in sites:
        if s["contig"] == contig and s["is_proposal"]:
            out[s["pos"]] = s["called"]
    return "".join(out)
