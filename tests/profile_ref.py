"""Plain-Python restatement of src/signalalign/scripts/multipleAlignmentAnalysis.py (:52-69, :118-242) over full-TSV text, for the
tests of sa_position_profile_*.  Columns 0, 1, 2, 9, 12, 15 as the script reads them; what differs from the script on purpose:
  - the direction of a file is given by the caller, not guessed (is_forward_alignment below restates the guess, and the CLI test
    asserts that it agrees with the given direction on its 1-D files);
  - a printed posterior becomes an integer of 1e-6 (round(float(s) * 1e6)) and every sum is an integer: per position the count,
    the letters' units and the entropy terms llrint((q log2 q + (1 - q) log2 (1 - q)) 2^40);
  - ref_char comes from the reference sequence (upper-cased; 'N' without one), not from the first row naming the position;
  - contigs come in the order of the reference's records, not sorted by name.
"""
import math

CONTIG, REF_POS, REF_KMER, PATH_KMER, POSTERIOR, KMER = 0, 1, 2, 9, 12, 15
UNITS_1 = 10 ** 6
COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C"}
HEADER = "#contig\tposition\tref_char\tshannon_entropy\tkmer_aln_count\tread_aln_count"


def complement(c):
    return COMPLEMENT.get(c, c)


def reverse_complement(s):
    return "".join(complement(c) for c in reversed(s))


def entropy_term(u):
    """the summand of shannon_entropy (:101) in units of 2^-40, with 1 - q as the script writes it"""
    if u == 0 or u == UNITS_1:
        return 0
    q = u / 1e6
    return round((q * math.log2(q) + (1.0 - q) * math.log2(1.0 - q)) * 2.0 ** 40)


def printed_units(text):
    return round(float(text) * 1e6)


def is_forward_alignment(tsv_text):
    """:52-69 over the text of one file: True / False, or None when every row is a palindrome"""
    for line in tsv_text.splitlines():
        f = line.split("\t")
        ref_kmer, path_kmer = f[REF_KMER].upper(), f[PATH_KMER].upper()
        if ref_kmer != path_kmer:
            return False
        if reverse_complement(ref_kmer) != path_kmer:
            return True
    return None


def rows_of_tsv(tsv_text):
    """(contig name, reference position, k-mer of column 15, printed units) of every line"""
    rows = []
    for line in tsv_text.splitlines():
        f = line.split("\t")
        rows.append((f[CONTIG], int(f[REF_POS]), f[KMER].strip().upper(), printed_units(f[POSTERIOR])))
    return rows


class Profile:
    def __init__(self, term=entropy_term):
        self.term = term
        self.sites = {}      # (contig, position) -> [kmer_count, entropy_units, {letter: units}, read_count]
        self.letters = set()

    def _site(self, key):
        return self.sites.setdefault(key, [0, 0, {}, 0])

    def add_file(self, rows, forward):
        """one file (:143-201): `rows` as rows_of_tsv gives them, all of one contig"""
        lo = hi = None
        contig = None
        for contig, ref_pos, kmer, units in rows:
            t = self.term(units)
            for i, c in enumerate(kmer):
                if forward:
                    pos, char = ref_pos + i, c
                else:
                    pos, char = ref_pos - i + len(kmer) - 1, complement(c)
                self.letters.add(char)
                lo = pos if lo is None else min(lo, pos)
                hi = pos if hi is None else max(hi, pos)
                s = self._site((contig, pos))
                s[0] += 1
                s[1] += t
                s[2][char] = s[2].get(char, 0) + units
        if contig is not None:
            for pos in range(lo, hi + 1):
                self._site((contig, pos))[3] += 1

    def finish(self, alphabet, contig_names, refs=None):
        """the sites in (contig index, position) order, as dicts with the fields of sa_profile_site_t"""
        index = {name: i for i, name in enumerate(contig_names)}
        out = []
        for (contig, pos), (kc, eu, by_letter, rc) in sorted(self.sites.items(), key=lambda kv: (index[kv[0][0]], kv[0][1])):
            units = [by_letter.get(c, 0) for c in alphabet]
            total = sum(units)
            ref = ""
            if kc > 0:
                ref = refs[index[contig]][pos].upper() if refs is not None else "N"
            out.append({"contig": index[contig], "pos": pos, "read_count": rc, "kmer_count": kc, "entropy_units": eu, "units": units,
                        "prob": [u / total if total else 0.0 for u in units],
                        "entropy": 0.0 if eu == 0 else (eu * 2.0 ** -40 / kc) / -2.0, "ref": ref})
        return out

    def letters_seen(self, alphabet):
        return sum(1 << i for i, c in enumerate(alphabet) if c in self.letters)


def file_text(sites, alphabet, letters_seen, contig_names):
    """the script's file (:203-242)"""
    seen = sorted(c for i, c in enumerate(alphabet) if letters_seen >> i & 1)
    out = [HEADER + "".join("\tp" + c for c in seen) + "\n"]
    for s in sites:
        out.append("%s\t%d\t%s\t%s\t%d\t%d" % (contig_names[s["contig"]], s["pos"], s["ref"], repr(float(s["entropy"])), s["kmer_count"],
                                                s["read_count"]))
        out.append("".join("\t" + repr(float(s["prob"][alphabet.index(c)])) for c in seen) + "\n")
    return "".join(out)


def kmer_of_id(kmer_id, alphabet, k):
    s = []
    for _ in range(k):
        s.append(alphabet[kmer_id % len(alphabet)])
        kmer_id //= len(alphabet)
    return "".join(reversed(s))


def rows_of_records(contig_name, pos0, pos_sign, k, alphabet, x, kmer_id, prob_e7):
    """a job's records as the rows its full TSV would hold: index x of the job's ref lies at contig position pos0 + pos_sign * x,
    a backward file names a k-mer by the position of its last letter, and the posterior is printed with "%f" """
    rows = []
    for xi, kid, pe7 in zip(x, kmer_id, prob_e7):
        ref_pos = pos0 + xi if pos_sign > 0 else pos0 - xi - (k - 1)
        rows.append((contig_name, ref_pos, kmer_of_id(int(kid), alphabet, k), printed_units("%f" % (int(pe7) / 1e7))))
    return rows
