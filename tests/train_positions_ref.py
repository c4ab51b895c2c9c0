"""Restatement of the k-mer training table built only from the rows that cover labelled positions, which the library runs on the GPU
(sa_kmer_table_set_positions, sa_kmer_table_add_batch_at, sa_kmer_table_position_counts) -- trainModels.py:161-286:
generate_build_alignments_positions, build_alignments_positions, get_kmers_covering_positions, filter_top_n_kmers and
write_and_generate_build_alignments_positions -- in plain Python, no pandas.

A row of the full output is (contig, reference_index, read strand 't' / 'c', forward-mapped, ...): forward-mapped means the
reference would write it to a forward.tsv rather than a backward.tsv.  With k the model's k-mer length the row COVERS the positions
line (contig, p, S) when the contigs are equal, p - (k - 1) <= reference_index <= p (get_kmers_covering_positions: the same window
for both site strands, taken literally), and S is the site strand build_alignments_positions pairs with the row (strand_pairs):
forward t '+', forward c '-', backward t '-', backward c '+'.  Only the first three columns of a line take part, duplicate lines
are one key.  A row is OFFERED when its printed posterior is >= min_prob and it covers at least one key; the offered rows then go
through the table's selection unchanged (kmer_training_ref.top_n: per strand and path k-mer the top N, ties by run order).

Two deliberate differences from the script: filter_top_n_kmers pools t and c rows of a k-mer, here the table's per-strand rule
stays; the script's tie order comes from a directory listing and an unstable sort, here it is run order, as for the unfiltered
table.

Coverage counts: per distinct key the number of offered rows that cover it over the whole run; a row within k - 1 of two labelled
positions counts once for each."""


def parse_positions(text):
    """the lines of a positions file as (contig, position, strand '+' / '-'): its first three columns, in file order"""
    out = []
    for line in text.splitlines():
        if not line.strip() or line.startswith("#"):
            continue
        f = line.split()
        assert f[2] in ("+", "-"), line
        out.append((f[0], int(f[1]), f[2]))
    return out


def site_strand(forward, read_strand):
    """strand_pairs of build_alignments_positions"""
    if forward:
        return "+" if read_strand == "t" else "-"
    return "-" if read_strand == "t" else "+"


def covered(keys, k, contig, reference_index, read_strand, forward):
    """the keys of the set `keys` that a row covers, in ascending position"""
    s = site_strand(forward, read_strand)
    return [(contig, p, s) for p in range(reference_index, reference_index + k) if (contig, p, s) in keys]


def offered(rows, lines, k, min_prob):
    """rows: (contig, reference_index, read strand, forward-mapped, posterior text) in run order; lines: parse_positions'.
    -> (indices of the offered rows in run order, {key: offered rows that cover it} with every distinct key present)"""
    keys = set(lines)
    counts = {key: 0 for key in keys}
    idx = []
    for i, (contig, ri, strand, forward, prob) in enumerate(rows):
        if not float(prob) >= min_prob:
            continue
        hit = covered(keys, k, contig, int(ri), strand, forward)
        if hit:
            idx.append(i)
            for key in hit:
                counts[key] += 1
    return idx, counts


def coverage_lines(lines, counts):
    """the coverage file: contigs in order of first appearance in the positions file, '+' before '-', then by position"""
    order = []
    for contig, _, _ in lines:
        if contig not in order:
            order.append(contig)
    keys = sorted(counts, key=lambda key: (order.index(key[0]), key[2] == "-", key[1]))
    return "".join("%s\t%d\t%s\t%d\n" % (c, p, s, counts[(c, p, s)]) for c, p, s in keys)
