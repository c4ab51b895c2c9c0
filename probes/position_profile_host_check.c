/* Stand-alone driver of the host half of the per-position profile (signalalign_amd/csrc/sa_profile.c) for
 * probes/position_profile_host_asan.sh: the entropy term over its whole domain, the argument checks at their edges, and the writer
 * on a site list with every kind of line.  sa_format_py_repr lives in a HIP source, so a plain shortest-round-trip formatter stands
 * in for it here: the numbers' characters are checked by the test-suite, this program is about memory. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sa_internal.h"

int sa_format_py_repr(char *out, double v) {
    for (int prec = 1; prec <= 17; prec++) {
        snprintf(out, 40, "%.*g", prec, v);
        if (strtod(out, NULL) == v) break;
    }
    return (int) strlen(out);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "/tmp/position_profile_host_check.tsv";
    /* the term: 0 at both ends and outside, -2^40 in the middle, symmetric */
    for (int64_t u = -2; u <= SA_PROFILE_UNITS_1 + 2; u++) {
        const int64_t t = sa_profile_entropy_term(u);
        CHECK(t == sa_profile_entropy_term(SA_PROFILE_UNITS_1 - u));
        CHECK(t <= 0 && t >= -((int64_t) 1 << 40));
        CHECK((t == 0) == (u <= 0 || u >= SA_PROFILE_UNITS_1));
    }
    CHECK(sa_profile_entropy_term(500000) == -((int64_t) 1 << 40));

    /* the map and the records */
    sa_profile_job_map_t map[2] = {{0, 1, 10}, {1, -1, 40}};
    CHECK(sa_profile_check_map(map, 2, 2) == SA_OK && sa_profile_check_map(map, 2, 1) == SA_EINVAL);
    CHECK(sa_profile_check_map(NULL, 0, 1) == SA_OK && sa_profile_check_map(NULL, 1, 1) == SA_EINVAL && sa_profile_check_map(map, -1, 2) == SA_EINVAL);
    map[1].pos_sign = 0;
    CHECK(sa_profile_check_map(map, 2, 2) == SA_EINVAL);
    map[1].pos_sign = -1;
    map[0].contig = -1;
    CHECK(sa_profile_check_map(map, 2, 2) == SA_EINVAL);
    map[0].contig = 0;
    int64_t first[3] = {0, 2, 3}, pe7[3] = {0, 10000000, 5};
    int32_t x[3] = {0, 5, 7}, kid[3] = {0, 1023, 4};
    CHECK(sa_profile_check_records(2, first, x, kid, pe7, 1024) == SA_OK);
    CHECK(sa_profile_check_records(2, first, x, kid, pe7, 1023) == SA_EINVAL);
    CHECK(sa_profile_check_records(2, first, NULL, kid, pe7, 1024) == SA_EINVAL && sa_profile_check_records(2, NULL, x, kid, pe7, 1024) == SA_EINVAL);
    pe7[1] = 10000001;
    CHECK(sa_profile_check_records(2, first, x, kid, pe7, 1024) == SA_EINVAL);
    pe7[1] = -1;
    CHECK(sa_profile_check_records(2, first, x, kid, pe7, 1024) == SA_EINVAL);
    pe7[1] = 1;
    x[2] = -1;
    CHECK(sa_profile_check_records(2, first, x, kid, pe7, 1024) == SA_EINVAL);
    x[2] = (int32_t) SA_PAIR16_MAX_COORD;
    CHECK(sa_profile_check_records(2, first, x, kid, pe7, 1024) == SA_EINVAL);
    x[2] = 7;
    first[1] = 4;
    CHECK(sa_profile_check_records(2, first, x, kid, pe7, 1024) == SA_EINVAL);
    first[1] = 2;
    first[0] = 1;
    CHECK(sa_profile_check_records(2, first, x, kid, pe7, 1024) == SA_EINVAL);
    first[0] = 0;
    int64_t empty[1] = {0};
    CHECK(sa_profile_check_records(0, empty, NULL, NULL, NULL, 1024) == SA_OK);

    /* the spans at the contig's two ends, both signs, and a position 0 that would overflow */
    int64_t lo = 0, hi = 0;
    CHECK(sa_profile_span(&map[0], 30, 0, 15, 5, &lo, &hi) == SA_OK && lo == 10 && hi == 29);
    CHECK(sa_profile_span(&map[0], 29, 0, 15, 5, &lo, &hi) == SA_EINVAL);
    CHECK(sa_profile_span(&map[1], 41, 0, 36, 5, &lo, &hi) == SA_OK && lo == 0 && hi == 40);
    CHECK(sa_profile_span(&map[1], 41, 0, 37, 5, &lo, &hi) == SA_EINVAL && sa_profile_span(&map[1], 40, 0, 36, 5, &lo, &hi) == SA_EINVAL);
    CHECK(sa_profile_span(&map[0], 30, 3, 2, 5, &lo, &hi) == SA_EINVAL && sa_profile_span(&map[0], 30, -1, 2, 5, &lo, &hi) == SA_EINVAL);
    map[0].pos0 = INT64_MAX;
    CHECK(sa_profile_span(&map[0], 30, 0, 15, 5, &lo, &hi) == SA_EINVAL);
    map[0].pos0 = INT64_MIN;
    map[0].pos_sign = -1;
    CHECK(sa_profile_span(&map[0], 30, 0, 15, 5, &lo, &hi) == SA_EINVAL);

    /* the writer: a full line, a covered position without rows, a zero total, eight letters, a second contig */
    sa_profile_site_t *sites = calloc(4, sizeof(*sites));
    CHECK(sites != NULL);
    sites[0].pos = 3; sites[0].read_count = 2; sites[0].kmer_count = 3; sites[0].entropy_units = -1991521358979;
    sites[0].units[0] = 750000; sites[0].units[1] = 1000000; sites[0].prob[0] = 0.42857142857142855; sites[0].prob[1] = 0.5714285714285714;
    sites[0].entropy = 0.30187968740983706; sites[0].ref = 'A';
    sites[1].pos = 4; sites[1].read_count = 1;
    sites[2].pos = 5; sites[2].read_count = 1; sites[2].kmer_count = 2; sites[2].ref = 'N';
    sites[3].contig = 1; sites[3].pos = ((int64_t) 1 << 40) - 1; sites[3].read_count = INT32_MAX; sites[3].kmer_count = INT64_MAX;
    sites[3].entropy_units = INT64_MIN; sites[3].entropy = 1e-300; sites[3].ref = 'T';
    for (int l = 0; l < SA_SITE_MAX_LETTERS; l++) { sites[3].units[l] = INT64_MAX; sites[3].prob[l] = 0.125; }
    const char *names[2] = {"chr_a", "a_contig_with_a_rather_long_name_that_no_fixed_buffer_should_be_sized_for_0123456789_0123456789_0123456789"};
    CHECK(sa_position_profile_write(path, "HGFEDCBA", 0xffu, names, sites, 4) == SA_OK);   /* (an unsorted alphabet: the letters are sorted) */
    CHECK(sa_position_profile_write(path, "ACGT", 0x0bu, names, sites, 3) == SA_OK);
    CHECK(sa_position_profile_write(path, "ACGT", 0x10u, names, sites, 3) == SA_EINVAL);     /* a letter outside the alphabet */
    CHECK(sa_position_profile_write(path, "ACEGHMOTX", 0, names, sites, 3) == SA_EINVAL);   /* more letters than a site holds */
    CHECK(sa_position_profile_write(path, "ACGT", 0, names, NULL, 0) == SA_OK && sa_position_profile_write(path, "ACGT", 0, names, NULL, 1) == SA_EINVAL);
    CHECK(sa_position_profile_write("/nonexistent-directory/p.tsv", "ACGT", 0, names, sites, 3) == SA_EIO);
    CHECK(sa_position_profile_write(path, "ACGT", 0x0bu, names, sites, 3) == SA_OK);
    FILE *fh = fopen(path, "r");
    CHECK(fh != NULL);
    char line[512];
    CHECK(fgets(line, sizeof line, fh) && strcmp(line, "#contig\tposition\tref_char\tshannon_entropy\tkmer_aln_count\tread_aln_count\tpA\tpC\tpT\n") == 0);
    CHECK(fgets(line, sizeof line, fh) && strcmp(line, "chr_a\t3\tA\t0.30187968740983706\t3\t2\t0.42857142857142855\t0.5714285714285714\t0\n") == 0);
    CHECK(fgets(line, sizeof line, fh) && strcmp(line, "chr_a\t4\t\t0\t0\t1\t0\t0\t0\n") == 0);
    fclose(fh);
    free(sites);
    remove(path);
    printf("position profile host half under the sanitizers: clean\n");
    return 0;
}
