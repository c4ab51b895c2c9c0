/* signalMachine's run-wide outputs (part of signalMachine.c's translation unit): what a run gathers over all of its slices and writes
 * at its end.  Each is an output_t in front of its own state; the run holds the ones its options ask for in R->out, and main, the
 * slice loop and the modes' batches go through that array (outputs_open .. outputs_finish, at the end of this file). */
struct output {
    const char *opt;   /* the option its messages name: "signalMachine: <opt>: checkpoint failed" */
    run_t *R;
    void (*open)(output_t *o);         /* (any may be NULL) before the first slice: create, read the truth files, write a header */
    int (*checkpoint)(output_t *o);    /* before a slice's GPU stage ... */
    int (*rollback)(output_t *o);      /* ... and back to it, when the slice starts over without the reads the planner refused */
    int (*add_batch)(output_t *o, slice_t *sl, int s, sa_batch_t *b);   /* strand s's batch has run: its records are still in HBM */
    void (*add_read)(output_t *o, slice_t *sl, int64_t j);              /* read who[j] is rendered; called in read order */
    void (*rendered)(output_t *o, slice_t *sl);                         /* every read of the slice is */
    void (*finish)(output_t *o);       /* after the last slice: write and destroy */
};

static void die_opt(const char *opt, const char *what) { fprintf(stderr, "signalMachine: %s: %s\n", opt, what); exit(1); }

/* the records of the -f reference, for the tables that are laid over them */
static void load_ref_records(run_t *R, const char *opt) {
    if (R->ref_names == NULL && sa_fasta_read_all(R->fwd_ref, &R->ref_names, &R->ref_seqs, &R->ref_lens, &R->n_refs) != SA_OK) {
        fprintf(stderr, "signalMachine: %s: cannot read %s\n", opt, R->fwd_ref ? R->fwd_ref : "");
        exit(1);
    }
}

/* contig coordinate of index t of a strand's target (the TSV's reference_index of a k-mer at t covers t .. t + k - 1) */
static int snp_contig_pos_is_forward(const read_t *rd, int s) { return (s == 0 && rd->forward) || (s == 1 && !rd->forward); }
static int64_t snp_contig_pos(const read_t *rd, int s, int64_t t) {
    const int64_t off = rd->st[s].r_shift;
    return snp_contig_pos_is_forward(rd, s) ? off + t : off - 1 - t;
}

/* --snp-marginals, --position-profile: which record of the -f reference a read lies on */
static int64_t snp_contig_index(const run_t *R, const read_t *rd) {
    const char *name = rd->seq_name ? rd->seq_name : rd->pA->contig1;
    int64_t ci = 0;
    while (ci < R->n_refs && strcmp(R->ref_names[ci], name) != 0) ci++;
    if (ci == R->n_refs) die("signalMachine: %s is no record of the -f reference", name);
    return ci;
}

/* ---- --site-calls-aggregate: the over-reads table (_normalize_all_data :393-407): per (contig, position, strand, forward_mapped)
 * and letter the per-read probabilities summed in read order, as the reads are rendered; written at the end of the run. ---- */
#define AGG_MAX_LETTERS 16
typedef struct {
    int64_t pos;
    int contig, n;
    char strand, mapped, used;
    char letter[AGG_MAX_LETTERS];
    double sum[AGG_MAX_LETTERS];
} agg_entry_t;
typedef struct {
    output_t o;
    agg_entry_t *tab;
    size_t cap, n;
    char **contigs;
    int n_contigs;
} agg_t;
static uint64_t agg_hash(int contig, int64_t pos, char strand, char mapped) {
    uint64_t h = (uint64_t) pos * 0x9E3779B97F4A7C15ull ^ ((uint64_t) (unsigned) contig << 17) ^ ((uint64_t) (unsigned char) strand << 8) ^
                 (uint64_t) (unsigned char) mapped;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return h;
}
static agg_entry_t *agg_slot(agg_t *ag, int contig, int64_t pos, char strand, char mapped) {
    if (2 * (ag->n + 1) > ag->cap) {   /* grow: rehash into twice the room */
        const size_t ncap = ag->cap ? 2 * ag->cap : 1 << 16;
        agg_entry_t *nt = calloc(ncap, sizeof(agg_entry_t));
        if (!nt) die("signalMachine: out of memory%s", "");
        for (size_t i = 0; i < ag->cap; i++) {
            const agg_entry_t *e = &ag->tab[i];
            if (!e->used) continue;
            size_t h = (size_t) agg_hash(e->contig, e->pos, e->strand, e->mapped) & (ncap - 1);
            while (nt[h].used) h = (h + 1) & (ncap - 1);
            nt[h] = *e;
        }
        free(ag->tab);
        ag->tab = nt;
        ag->cap = ncap;
    }
    size_t h = (size_t) agg_hash(contig, pos, strand, mapped) & (ag->cap - 1);
    for (;; h = (h + 1) & (ag->cap - 1)) {
        agg_entry_t *e = &ag->tab[h];
        if (!e->used) {
            e->used = 1; e->contig = contig; e->pos = pos; e->strand = strand; e->mapped = mapped;
            ag->n++;
            return e;
        }
        if (e->contig == contig && e->pos == pos && e->strand == strand && e->mapped == mapped) return e;
    }
}
static void agg_add_strand(agg_t *ag, const read_t *rd, int s, int tmpl_amb, const sa_site_call_t *calls, int64_t n, int k) {
    if (n <= 0) return;
    int ci = 0;
    while (ci < ag->n_contigs && strcmp(ag->contigs[ci], rd->pA->contig1) != 0) ci++;
    if (ci == ag->n_contigs) {
        ag->contigs = realloc(ag->contigs, sizeof(char *) * (size_t) (ag->n_contigs + 1));
        ag->contigs[ag->n_contigs++] = strdup(rd->pA->contig1);
    }
    char mapped;
    call_pos_t *v = order_calls(rd, s, tmpl_amb, calls, n, k, &mapped);
    for (int64_t q = 0; q < n; q++) {
        const sa_site_call_t *c = &calls[v[q].i];
        agg_entry_t *e = agg_slot(ag, ci, v[q].pos, s == 0 ? 't' : 'c', mapped);
        for (int l = 0; l < c->n_letters; l++) {
            int t = 0;
            while (t < e->n && e->letter[t] != c->letters[l]) t++;
            if (t == e->n) {
                if (e->n == AGG_MAX_LETTERS) die("signalMachine: --site-calls-aggregate: more than 16 letters at one site%s", "");
                e->letter[e->n] = c->letters[l]; e->sum[e->n] = 0.0; e->n++;
            }
            e->sum[t] += c->prob[l];
        }
    }
    free(v);
}
/* (the sums over reads are taken here, in read order: they do not depend on the rendering threads) */
static void agg_add_read(output_t *o, slice_t *sl, int64_t j) {
    const run_t *R = o->R;
    for (int s = 0; s < n_strands(R); s++)
        agg_add_strand((agg_t *) o, &sl->reads[sl->who[j]], s, sl->tmpl_amb && sl->tmpl_amb[j], sl->sr[s].calls[j], sl->sr[s].n_calls[j], R->sm[s].k);
}
static int cmp_agg(const void *a, const void *b, void *ctx) {
    const agg_t *ag = ctx;
    const agg_entry_t *x = *(const agg_entry_t *const *) a, *y = *(const agg_entry_t *const *) b;
    const int c = strcmp(ag->contigs[x->contig], ag->contigs[y->contig]);
    if (c) return c;
    if (x->strand != y->strand) return x->strand < y->strand ? -1 : 1;
    if (x->mapped != y->mapped) return x->mapped < y->mapped ? -1 : 1;
    return x->pos < y->pos ? -1 : x->pos > y->pos;
}
/* write_data (:409-411): header, then the rows as pandas prints them -- np.round(sum / total, 6) through repr.  Columns: the sorted
 * union of the letters; a letter a site does not have counts 0. */
static void agg_finish(output_t *o) {
    agg_t *ag = (agg_t *) o;
    const char *path = o->R->agg_path;
    if (!path) return;   /* (--site-calls-accuracy alone: the table is its level 2, and is not written) */
    int have[256] = {0};
    agg_entry_t **rows = xalloc((int64_t) ag->n, sizeof(agg_entry_t *), 0);
    size_t n = 0;
    for (size_t i = 0; i < ag->cap; i++)
        if (ag->tab[i].used) {
            rows[n++] = &ag->tab[i];
            for (int t = 0; t < ag->tab[i].n; t++) have[(unsigned char) ag->tab[i].letter[t]] = 1;
        }
    qsort_r(rows, n, sizeof(agg_entry_t *), cmp_agg, ag);
    FILE *fh = fopen(path, "w");
    if (!fh) die("signalMachine: cannot open output %s", path);
    setvbuf(fh, NULL, _IOFBF, 1 << 20);
    char cols[256];
    int nc = 0;
    for (int ch = 0; ch < 256; ch++)
        if (have[ch]) cols[nc++] = (char) ch;
    fprintf(fh, "contig\tposition\tstrand\tforward_mapped");
    for (int c = 0; c < nc; c++) fprintf(fh, "\t%c", cols[c]);
    fputc('\n', fh);
    char num[40];
    for (size_t r = 0; r < n; r++) {
        const agg_entry_t *e = rows[r];
        double total = 0.0;   /* sum over the letters in column order, as the reference's generator adds them */
        for (int c = 0; c < nc; c++)
            for (int t = 0; t < e->n; t++)
                if (e->letter[t] == cols[c]) total += e->sum[t];
        fprintf(fh, "%s\t%" PRId64 "\t%c\t%c", ag->contigs[e->contig], e->pos, e->strand, e->mapped);
        for (int c = 0; c < nc; c++) {
            double v = 0.0;
            for (int t = 0; t < e->n; t++)
                if (e->letter[t] == cols[c]) v = e->sum[t];
            sa_format_py_round6(num, v / total);
            fprintf(fh, "\t%s", num);
        }
        fputc('\n', fh);
    }
    fclose(fh);
    free(rows);
}

/* ---- --site-calls-accuracy: the calls scored against known truth (plot_variant_accuracy.py:44-175) in one sa_call_scores_t.
 * Levels 0 and 1 are added batch by batch while the batch's records lie in HBM (acc_add_batch), level 2 at the end of the run from
 * the over-reads table, in the six decimals it prints (acc_add_aggregate).  The accumulator's letters are those of the run's first
 * call, so it is made when that call is there.  A read named in --site-calls-truth-reads is labelled as a whole (generate_labels2),
 * every other site by the positions file (generate_labels); level 2 takes the positions file only. ---- */
typedef struct { int contig, strand; int64_t pos, line; char letter; } acc_truth_t;
typedef struct { char *label; char letter; } acc_label_t;
typedef struct {
    output_t o;
    agg_t *agg;                          /* the run's over-reads table: level 2 */
    sa_call_scores_t *acc;
    int ck;                              /* the accumulator was there, and checkpointed, when the slice began */
    char letters[SA_SITE_MAX_LETTERS + 1];
    char **contigs;                      /* a contig's index is its place here: the positions file's names first */
    int n_contigs;
    acc_truth_t *truth;                  /* sorted by (contig, pos, strand, line) */
    int64_t n_truth;
    acc_label_t *labels;                 /* sorted by label */
    int64_t n_labels;
} acc_t;
static int acc_contig(acc_t *ac, const char *name) {
    int ci = 0;
    while (ci < ac->n_contigs && strcmp(ac->contigs[ci], name) != 0) ci++;
    if (ci == ac->n_contigs) {
        ac->contigs = realloc(ac->contigs, sizeof(char *) * (size_t) (ac->n_contigs + 1));
        ac->contigs[ac->n_contigs++] = strdup(name);
    }
    return ci;
}
static int cmp_acc_truth(const void *a, const void *b) {
    const acc_truth_t *x = a, *y = b;
    if (x->contig != y->contig) return x->contig < y->contig ? -1 : 1;
    if (x->pos != y->pos) return x->pos < y->pos ? -1 : 1;
    if (x->strand != y->strand) return x->strand < y->strand ? -1 : 1;
    return x->line < y->line ? -1 : x->line > y->line;
}
static int cmp_acc_label(const void *a, const void *b) { return strcmp(((const acc_label_t *) a)->label, ((const acc_label_t *) b)->label); }
/* the two truth files, read before the run starts so that a bad one stops it */
static void acc_open(output_t *o) {
    acc_t *ac = (acc_t *) o;
    const run_t *R = o->R;
    char line[4096], a[1024], st[64], from[64], to[64];
    if (R->acc_truth_path) {
        FILE *fh = fopen(R->acc_truth_path, "r");
        if (!fh) die("signalMachine: --site-calls-truth: cannot read %s", R->acc_truth_path);
        int64_t cap = 0, pos = 0;
        while (fgets(line, sizeof line, fh)) {
            if (line[0] == '\n' || line[0] == '#') continue;
            if (sscanf(line, "%1023s %" SCNd64 " %63s %63s %63s", a, &pos, st, from, to) != 5 || (strcmp(st, "+") && strcmp(st, "-")) || strlen(to) != 1)
                die("signalMachine: --site-calls-truth: not 'contig position +|- change_from change_to': %s", line);
            if (ac->n_truth == cap) ac->truth = realloc(ac->truth, sizeof(acc_truth_t) * (size_t) (cap = cap ? 2 * cap : 1024));
            ac->truth[ac->n_truth] = (acc_truth_t) {acc_contig(ac, a), st[0] == '-', pos, ac->n_truth, to[0]};
            ac->n_truth++;
        }
        fclose(fh);
        qsort(ac->truth, (size_t) ac->n_truth, sizeof(acc_truth_t), cmp_acc_truth);
    }
    if (R->acc_reads_path) {
        FILE *fh = fopen(R->acc_reads_path, "r");
        if (!fh) die("signalMachine: --site-calls-truth-reads: cannot read %s", R->acc_reads_path);
        int64_t cap = 0;
        while (fgets(line, sizeof line, fh)) {
            if (line[0] == '\n' || line[0] == '#') continue;
            if (sscanf(line, "%1023s %63s", a, to) != 2 || strlen(to) != 1) die("signalMachine: --site-calls-truth-reads: not 'label letter': %s", line);
            if (ac->n_labels == cap) ac->labels = realloc(ac->labels, sizeof(acc_label_t) * (size_t) (cap = cap ? 2 * cap : 1024));
            ac->labels[ac->n_labels++] = (acc_label_t) {strdup(a), to[0]};
        }
        fclose(fh);
        qsort(ac->labels, (size_t) ac->n_labels, sizeof(acc_label_t), cmp_acc_label);
    }
}
/* index of the read's label letter in the accumulator's letters, -1 for a read without a label */
static int acc_read_letter(const acc_t *ac, const char *label) {
    const acc_label_t key = {(char *) label, 0};
    const acc_label_t *e = ac->n_labels ? bsearch(&key, ac->labels, (size_t) ac->n_labels, sizeof(acc_label_t), cmp_acc_label) : NULL;
    if (!e) return -1;
    const char *at = strchr(ac->letters, e->letter);
    if (!at) die("signalMachine: --site-calls-truth-reads: the letter of read %s is not one of the sites' letters", label);
    return (int) (at - ac->letters);
}
/* the first line of the positions file that names (contig, pos, mapped strand): its change_to, 0 when none does */
static char acc_truth_letter(const acc_t *ac, int contig, int64_t pos, int strand) {
    int64_t lo = 0, hi = ac->n_truth;
    const acc_truth_t key = {contig, strand, pos, -1, 0};
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (cmp_acc_truth(&ac->truth[mid], &key) < 0) lo = mid + 1; else hi = mid;
    }
    const acc_truth_t *e = lo < ac->n_truth ? &ac->truth[lo] : NULL;
    return e && e->contig == contig && e->pos == pos && e->strand == strand ? e->letter : 0;
}
/* the accumulator, made when the run has its first call: its letters are that call's */
static void acc_create(acc_t *ac, const strand_result_t *sr, int64_t n) {
    const run_t *R = ac->o.R;
    for (int64_t j = 0; j < n && !ac->acc; j++) {
        if (sr->n_calls[j] <= 0) continue;
        const sa_site_call_t *c = &sr->calls[j][0];
        memcpy(ac->letters, c->letters, (size_t) c->n_letters);
        ac->letters[c->n_letters] = 0;
        sa_truth_site_t *t = xalloc(ac->n_truth, sizeof(*t), 1);
        for (int64_t i = 0; i < ac->n_truth; i++) {
            t[i].contig = ac->truth[i].contig; t[i].mapped_strand = ac->truth[i].strand; t[i].pos = ac->truth[i].pos;
            t[i].change_to = ac->truth[i].letter;
        }
        const int rc = sa_call_scores_create(&ac->acc, ac->letters, R->acc_bins, R->acc_threshold, t, ac->n_truth, R->device);
        free(t);
        if (rc == SA_EINVAL) die("signalMachine: --site-calls-truth: a change_to letter is not one of the sites' letters %s, or a position is negative", ac->letters);
        if (rc != SA_OK) die("signalMachine: --site-calls-accuracy: %s", sa_strerror(rc));
    }
}
/* Where every job of the slice's strand s lies: adjust_ref as x0 + x_sign * x, the mapping strand the one order_calls gives the job's
 * calls, the read's label where --site-calls-truth-reads names it. */
static sa_score_job_map_t *acc_job_map(acc_t *ac, const slice_t *sl, int s) {
    const run_t *R = ac->o.R;
    const int64_t nj = sl->n_ok;
    sa_score_job_map_t *map = xalloc(nj, sizeof(*map), 1);
    for (int64_t j = 0; j < nj; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        const int idx = (s == 1 && sl->tmpl_amb && sl->tmpl_amb[j]) ? 1 : 0;
        const int along = (s == 0 && rd->forward) || (s == 1 && !rd->forward);
        map[j].contig = acc_contig(ac, rd->pA->contig1);
        map[j].x_sign = along ? 1 : -1;
        map[j].x0 = along ? rd->st[s].r_shift : rd->st[s].r_shift - R->sm[s].k;
        map[j].strand = s;
        map[j].mapped_strand = (idx == 0) == (rd->forward != 0) ? 0 : 1;
        map[j].true_letter = acc_read_letter(ac, rd->label);
    }
    return map;
}
/* levels 0 and 1 of the slice's finished batch of strand s */
static void acc_add(acc_t *ac, const slice_t *sl, int s, sa_batch_t *b) {
    const int64_t nj = sl->n_ok;
    acc_create(ac, &sl->sr[s], nj);
    if (!ac->acc) return;   /* (no call so far: nothing to score) */
    sa_score_job_map_t *map = acc_job_map(ac, sl, s);
    const int rc = sa_call_scores_add_batch(ac->acc, b, map, nj, NULL);
    free(map);
    if (rc != SA_OK) die_opt(ac->o.opt, sa_strerror(rc));
}
/* A 2-D run's complement waits for the rendering, which finds out its calls' mapping strand (tmpl_amb): the records go up again from the host copy */
static int acc_add_batch(output_t *o, slice_t *sl, int s, sa_batch_t *b) {
    if (!(s == 1 && o->R->two_d)) acc_add((acc_t *) o, sl, s, b);
    return SA_OK;
}
static void acc_rendered(output_t *o, slice_t *sl) {
    if (o->R->two_d && sl->sr[1].batch && sl->n_ok > 0) acc_add((acc_t *) o, sl, 1, sl->sr[1].batch);
}
/* an accumulator that the slice itself made is given up when the slice starts over, not rolled back */
static int acc_checkpoint(output_t *o) {
    acc_t *ac = (acc_t *) o;
    ac->ck = ac->acc != NULL;
    return ac->ck ? sa_call_scores_checkpoint(ac->acc) : SA_OK;
}
static int acc_rollback(output_t *o) {
    acc_t *ac = (acc_t *) o;
    if (ac->acc && ac->ck) return sa_call_scores_rollback(ac->acc);
    sa_call_scores_destroy(ac->acc);
    ac->acc = NULL;
    return SA_OK;
}
/* level 2: every row of the over-reads table whose letters are the accumulator's and whose site the positions file names, with
 * the values agg_finish prints */
static void acc_add_aggregate(acc_t *ac) {
    const agg_t *ag = ac->agg;
    const size_t nl = strlen(ac->letters);
    for (int strand = 0; strand < 2 && ac->acc; strand++) {
        double *prob = xalloc((int64_t) (ag->n * nl), sizeof(double), 0);
        int8_t *tl = xalloc((int64_t) ag->n, 1, 0);
        int64_t n = 0;
        for (size_t i = 0; i < ag->cap; i++) {
            const agg_entry_t *e = &ag->tab[i];
            if (!e->used || (e->strand == 't') != (strand == 0) || (size_t) e->n != nl) continue;
            double v[SA_SITE_MAX_LETTERS], total = 0.0;
            int ok = 1;
            for (size_t l = 0; l < nl && ok; l++) {   /* (the accumulator's letters are sorted: the table's column order) */
                int t = 0;
                while (t < e->n && e->letter[t] != ac->letters[l]) t++;
                ok = t < e->n;
                if (ok) { v[l] = e->sum[t]; total += v[l]; }
            }
            const char letter = ok ? acc_truth_letter(ac, acc_contig(ac, ag->contigs[e->contig]), e->pos, e->mapped == '-') : 0;
            const char *at = letter ? strchr(ac->letters, letter) : NULL;
            if (!at) continue;
            char num[40];
            for (size_t l = 0; l < nl; l++) {
                sa_format_py_round6(num, v[l] / total);
                prob[(size_t) n * nl + l] = strtod(num, NULL);
            }
            tl[n++] = (int8_t) (at - ac->letters);
        }
        const int rc = sa_call_scores_add_records(ac->acc, 2, strand, prob, tl, n);
        if (rc != SA_OK) die("signalMachine: --site-calls-accuracy: %s", sa_strerror(rc));
        free(prob); free(tl);
    }
}
static void acc_finish(output_t *o) {
    acc_t *ac = (acc_t *) o;
    const run_t *R = o->R;
    sa_call_score_row_t *rows = NULL;
    int64_t n_rows = 0, *curves = NULL;
    sa_call_scores_counts_t counts = {0, 0};
    if (ac->acc) {
        acc_add_aggregate(ac);
        const int rc = sa_call_scores_finish(ac->acc, &rows, &n_rows, &curves, &counts, NULL);
        if (rc != SA_OK) die("signalMachine: --site-calls-accuracy: %s", sa_strerror(rc));
    }
    if (sa_call_scores_write(R->acc_path, R->acc_curves_path, R->acc_bins, rows, n_rows, curves) != SA_OK)
        die("signalMachine: cannot write %s", R->acc_path);
    fprintf(stderr, "[signalMachine] accuracy: %" PRId64 " rows; %" PRId64 " calls without truth dropped, %" PRId64 " sites of other letters skipped\n",
            n_rows, counts.unlabelled, counts.other_sites);
    sa_free(rows); sa_free(curves);
    sa_call_scores_destroy(ac->acc);
    ac->acc = NULL;
}

/* ---- --site-calls-accuracy-quality: every template batch's labelled calls against the distance of their band from the guide, and
 * the breaks of the MEA paths (sa_batch_call_quality), with the letters, threshold and positions table of the run's accumulator;
 * written read by read as the reads are rendered.  A read given as .npRead has no raw starts: its job goes into the call with
 * one-sample events (the call wants every job of the batch) and nothing is written for it. ---- */
typedef struct {
    output_t o;
    acc_t *acc;
    FILE *fh, *calls_fh;
    int64_t total[(SA_CQ_MAX_BINS + 2) * 2];   /* the histogram rows of the reads written so far, summed: the H lines */
} callq_t;
static void cq_open(output_t *o) {
    callq_t *cq = (callq_t *) o;
    const run_t *R = o->R;
    if (!(cq->fh = fopen(R->cq_path, "w"))) die("signalMachine: cannot open output %s", R->cq_path);
    fprintf(cq->fh, "#call-quality bin_lo=%" PRId64 " bin_width=%" PRId64 " n_bins=%d min_gap=%d; R label strand status n_calls n_correct n_unlabelled "
                    "n_other_sites n_outside sum_abs_delta2 max_abs_delta2 max_reference_index n_path n_gaps sum_gap max_gap; G label strand "
                    "event_before event_after gap; H bin_lo wrong correct\n", R->cq_params.bin_lo, R->cq_params.bin_width, R->cq_params.n_bins,
            R->cq_params.min_gap);
    if (R->cq_calls_path) {
        if (!(cq->calls_fh = fopen(R->cq_calls_path, "w"))) die("signalMachine: cannot open output %s", R->cq_calls_path);
        fprintf(cq->calls_fh, "#label\tstrand\treference_index\traw_start\traw_length\tguide_event\tdelta\ttrue_letter\tprob\tcorrect\toutside\n");
    }
}
/* the finished template batch against its own jobs' anchors, with the MEA paths just made of it (after acc_add_batch, which makes
 * the accumulator at the run's first call; before that there is nothing to label) */
static int cq_add_batch(output_t *o, slice_t *sl, int s, sa_batch_t *b) {
    callq_t *cq = (callq_t *) o;
    const run_t *R = o->R;
    strand_result_t *sr = &sl->sr[s];
    const int64_t n = sl->n_ok, n_slots = ((int64_t) R->cq_params.n_bins + 2) * 2;
    if (s != 0 || !cq->acc->acc) return SA_OK;
    sa_callq_job_t *cj = xalloc(n, sizeof(*cj), 1);
    int64_t *plain = NULL, n_plain = 0;   /* 0, 1, 2, ...: the raw starts of the reads that have none */
    for (int64_t j = 0; j < n; j++)
        if (!sl->reads[sl->who[j]].raw_start && sl->jobs[s][j].n_events > n_plain) n_plain = sl->jobs[s][j].n_events;
    if (n_plain > 0) {
        plain = xalloc(2 * n_plain, sizeof(int64_t), 0);
        for (int64_t y = 0; y < n_plain; y++) { plain[y] = y; plain[n_plain + y] = 1; }
    }
    for (int64_t j = 0; j < n; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        const sa_job_t *q = &sl->jobs[s][j];
        cj[j] = (sa_callq_job_t) {q->anchor_x, q->anchor_y, q->n_anchors, rd->raw_start ? rd->raw_start + rd->st[s].lo : plain,
                                  rd->raw_start ? rd->raw_length + rd->st[s].lo : plain + n_plain, q->n_events};
    }
    sa_score_job_map_t *map = acc_job_map(cq->acc, sl, s);
    sr->cq_reads = xalloc(n, sizeof(sa_callq_read_t), 1);
    sr->cq_hist = xalloc(n * n_slots, sizeof(int64_t), 1);
    int64_t n_calls = 0, n_gaps = 0;
    const int rc = sa_batch_call_quality(cq->acc->acc, b, map, cj, n, (const sa_mea_pair_t *const *) sr->mea, sr->n_mea, &R->cq_params,
                                         cq->calls_fh ? SA_CQ_CALLS : 0u, sr->cq_reads, cq->calls_fh ? &sr->cq_calls : NULL,
                                         cq->calls_fh ? &n_calls : NULL, &sr->cq_gaps, &n_gaps, sr->cq_hist, NULL, NULL);
    free(map); free(cj); free(plain);
    if (rc != SA_OK) die_opt(o->opt, sa_strerror(rc));
    return SA_OK;
}
/* ... and the lines of job j.  Events are printed as the TSV's event_index column prints them, positions as the .calls file prints
 * them; delta is delta2 / 2, an integer or <n>.5 */
static void cq_add_read(output_t *o, slice_t *sl, int64_t j) {
    callq_t *cq = (callq_t *) o;
    const run_t *R = o->R;
    const read_t *rd = &sl->reads[sl->who[j]];
    const strand_result_t *sr = &sl->sr[0];
    if (!rd->raw_start) {
        fprintf(stderr, "[signalMachine]NOTICE: %s is not given as raw current: no call quality\n", rd->label);
        return;
    }
    if (!sr->cq_reads) return;   /* (the run had no site call yet when the read's batch finished) */
    const sa_callq_read_t *r = &sr->cq_reads[j];
    const int64_t n_slots = ((int64_t) R->cq_params.n_bins + 2) * 2, lo = rd->st[0].lo;
    const int64_t ref_len = (int64_t) strlen(rd->st[0].target), ref_len_kmers = ref_len - R->sm[0].k, off = rd->st[0].r_shift;
    fprintf(cq->fh, "R\t%s\tt\t%d\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64
                    "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\n", rd->label, r->status, r->n_calls, r->n_correct, r->n_unlabelled, r->n_other_sites,
            r->n_outside, r->sum_abs_delta2, r->max_abs_delta2,
            r->max_x >= 0 ? adjust_ref(r->max_x, off, ref_len_kmers, ref_len, 1, rd->forward) : (int64_t) -1, r->n_path, r->n_gaps, r->sum_gap,
            r->max_gap);
    for (int64_t i = 0; i < r->n_gaps; i++) {
        const sa_callq_gap_t *g = &sr->cq_gaps[r->gap_first + i];
        fprintf(cq->fh, "G\t%s\tt\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\n", rd->label, lo + g->y_before, lo + g->y_after, g->gap);
    }
    for (int64_t q = 0; q < n_slots; q++) cq->total[q] += sr->cq_hist[j * n_slots + q];
    for (int64_t i = 0; cq->calls_fh && i < r->n_calls; i++) {
        const sa_callq_call_t *c = &sr->cq_calls[r->call_first + i];
        const int64_t half = c->delta2 < 0 ? -c->delta2 : c->delta2;
        char prob[40];
        sa_format_py_repr(prob, c->prob_true);
        fprintf(cq->calls_fh, "%s\tt\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%s%" PRId64 "%s\t%c\t%s\t%d\t%d\n", rd->label,
                adjust_ref(c->x, off, ref_len_kmers, ref_len, 1, rd->forward), c->raw_start, c->raw_length,
                c->guide_event >= 0 ? lo + c->guide_event : (int64_t) -1, c->delta2 < 0 ? "-" : "", half / 2, half % 2 ? ".5" : "",
                cq->acc->letters[c->true_letter], prob, c->correct, c->outside);
    }
}
static void cq_finish(output_t *o) {   /* the histogram summed over the reads written */
    callq_t *cq = (callq_t *) o;
    const sa_callq_params_t *p = &o->R->cq_params;
    for (int q = 0; q < p->n_bins + 2; q++) {
        if (q == 0) fprintf(cq->fh, "H\tunder");
        else if (q == p->n_bins + 1) fprintf(cq->fh, "H\tover");
        else fprintf(cq->fh, "H\t%" PRId64, p->bin_lo + (int64_t) (q - 1) * p->bin_width);
        fprintf(cq->fh, "\t%" PRId64 "\t%" PRId64 "\n", cq->total[2 * q], cq->total[2 * q + 1]);
    }
    if (fclose(cq->fh) != 0 || (cq->calls_fh && fclose(cq->calls_fh) != 0)) die("signalMachine: cannot write %s", o->R->cq_path);
}

/* ---- --train-*: the top-N assignments of the whole run in k-mer tables on the GPU, one per strand ---- */
typedef struct {
    output_t o;
    sa_kmer_table_t *tab[2];
    /* --train-positions: the lines of the positions file; a contig's index is its place in `contigs`, the file's names first */
    sa_train_site_t *pos;
    int64_t n_pos;
    char **contigs;
    int n_contigs;
} train_t;
static int train_contig(train_t *tr, const char *name) {
    int ci = 0;
    while (ci < tr->n_contigs && strcmp(tr->contigs[ci], name) != 0) ci++;
    if (ci == tr->n_contigs) {
        tr->contigs = realloc(tr->contigs, sizeof(char *) * (size_t) (tr->n_contigs + 1));
        tr->contigs[tr->n_contigs++] = strdup(name);
    }
    return ci;
}
/* --train-positions: the file is read before the run starts, so that a bad line stops it (its first three columns take part) */
static void train_open(output_t *o) {
    train_t *tr = (train_t *) o;
    const run_t *R = o->R;
    if (!R->train_pos) return;
    char line[4096], a[1024], st[64];
    FILE *fh = fopen(R->train_pos, "r");
    if (!fh) die("signalMachine: --train-positions: cannot read %s", R->train_pos);
    int64_t cap = 0, pos = 0;
    while (fgets(line, sizeof line, fh)) {
        if (line[0] == '\n' || line[0] == '#') continue;
        if (sscanf(line, "%1023s %" SCNd64 " %63s", a, &pos, st) != 3 || (strcmp(st, "+") && strcmp(st, "-")) || pos < 0)
            die("signalMachine: --train-positions: not 'contig position +|- ...': %s", line);
        if (tr->n_pos == cap) tr->pos = realloc(tr->pos, sizeof(sa_train_site_t) * (size_t) (cap = cap ? 2 * cap : 1024));
        tr->pos[tr->n_pos++] = (sa_train_site_t) {train_contig(tr, a), st[0] == '-', pos};
    }
    fclose(fh);
}
/* strand s's table, made when it is first needed; with --train-positions it takes only the rows that cover a line */
static int train_table(train_t *tr, int s) {
    const run_t *R = tr->o.R;
    if (tr->tab[s]) return SA_OK;
    int rc = sa_kmer_table_create(&tr->tab[s], R->sm[s].model, R->train_n, R->train_min_prob, R->device);
    if (rc == SA_OK && R->train_pos) rc = sa_kmer_table_set_positions(tr->tab[s], tr->pos, tr->n_pos);
    return rc;
}
/* --train-positions-coverage: per distinct line the offered rows of both strands' tables that cover it; contigs in the order the
 * positions file first names them, '+' before '-', then by position (the tables' own order of keys) */
static void write_train_coverage(const train_t *tr) {
    const run_t *R = tr->o.R;
    FILE *f = fopen(R->train_pos_cov, "w");
    if (!f) die("signalMachine: cannot write %s", R->train_pos_cov);
    sa_train_site_t *site[2] = {NULL, NULL};
    int64_t *cnt[2] = {NULL, NULL}, n[2] = {0, 0};
    for (int s = 0; s < n_strands(R); s++)
        if (sa_kmer_table_position_counts(tr->tab[s], &site[s], &cnt[s], &n[s]) != SA_OK || n[s] != n[0])
            die("signalMachine: --train-positions-coverage: no counts%s", "");
    for (int64_t i = 0; i < n[0]; i++)
        fprintf(f, "%s\t%" PRId64 "\t%c\t%" PRId64 "\n", tr->contigs[site[0][i].contig], site[0][i].pos, site[0][i].mapped_strand ? '-' : '+',
                cnt[0][i] + (n_strands(R) > 1 ? cnt[1][i] : 0));
    if (fclose(f) != 0) die("signalMachine: cannot write %s", R->train_pos_cov);
    for (int s = 0; s < 2; s++) { sa_free(site[s]); sa_free(cnt[s]); }
}

/* --train-mixture-motifs: the (canonical, modified) k-mer ids of every motif pair of the list, for the model of strand s:
 * get_motif_kmer_pairs with the reference's flanks (A, T, G, C), the pairs of all motifs as one sorted set (mixture_model.py
 * main(): a set union).  A malformed list or a letter outside the model's alphabet ends the run with the usage text. */
typedef struct {
    int32_t canonical, modified;
    char name[2][24];
} mix_pair_t;

static int cmp_mix_pair(const void *a, const void *b) {
    const mix_pair_t *x = a, *y = b;
    const int c = strcmp(x->name[0], y->name[0]);
    return c ? c : strcmp(x->name[1], y->name[1]);
}

static int64_t mixture_pairs(const run_t *R, int s, mix_pair_t **out) {
    const strand_model_t *sm = &R->sm[s];
    char *list = strdup(R->mix_motifs), *save = NULL;
    mix_pair_t *v = NULL;
    int64_t n = 0;
    if (R->mix_motifs[0] == 0 || R->mix_motifs[strlen(R->mix_motifs) - 1] == ',' || strstr(R->mix_motifs, ",,"))
        usage_die("signalMachine: --train-mixture-motifs: malformed list %s", R->mix_motifs);
    for (char *item = strtok_r(list, ",", &save); item; item = strtok_r(NULL, ",", &save)) {
        char *colon = strchr(item, ':');
        if (!colon || colon == item || colon[1] == 0 || strchr(colon + 1, ':'))
            usage_die("signalMachine: --train-mixture-motifs: expected <canonical>:<modified>, got %s", item);
        *colon = 0;
        for (const char *m = item; m; m = m == item ? colon + 1 : NULL)
            for (const char *c = m; *c; c++)
                if (!memchr(sm->alphabet, toupper((unsigned char) *c), (size_t) sm->n_alpha))
                    usage_die("signalMachine: --train-mixture-motifs: a letter of %s is not in the model's alphabet", m);
        char *pairs = NULL;
        int64_t np = 0;
        if (sm->k >= (int) sizeof(v->name[0]) || sa_motif_kmer_pairs(sm->k, item, colon + 1, NULL, &pairs, &np) != SA_OK)
            usage_die("signalMachine: --train-mixture-motifs: %s and its partner must differ in one letter, the first of them made of A, C, G, T", item);
        v = realloc(v, (size_t) (n + np + 1) * sizeof(mix_pair_t));
        if (!v) die("signalMachine: out of memory%s", "");
        for (int64_t i = 0; i < np; i++) {
            mix_pair_t *q = &v[n];
            snprintf(q->name[0], sizeof q->name[0], "%s", pairs + (2 * i) * (sm->k + 1));
            snprintf(q->name[1], sizeof q->name[1], "%s", pairs + (2 * i + 1) * (sm->k + 1));
            q->canonical = (int32_t) sa_kmer_id(sm->model, q->name[0]);
            q->modified = (int32_t) sa_kmer_id(sm->model, q->name[1]);
            if (q->canonical >= 0 && q->modified >= 0) n++;
        }
        sa_free(pairs);
    }
    free(list);
    if (n) qsort(v, (size_t) n, sizeof(mix_pair_t), cmp_mix_pair);
    int64_t m = 0;
    for (int64_t i = 0; i < n; i++)
        if (m == 0 || cmp_mix_pair(&v[m - 1], &v[i]) != 0) v[m++] = v[i];
    *out = v;
    return m;
}

typedef struct {
    const char *kmer;
    double v[7];            /* canonical model mean, sd; canonical mixture mean, sd; modified mixture mean, sd; distance */
    int strand;
} mix_row_t;

static int cmp_mix_row(const void *a, const void *b) {   /* distance descending, then k-mer, then strand */
    const mix_row_t *x = a, *y = b;
    if (x->v[6] != y->v[6]) return x->v[6] > y->v[6] ? -1 : 1;
    const int c = strcmp(x->kmer, y->kmer);
    return c ? c : x->strand - y->strand;
}

/* generate_gaussian_mixture_model_for_motifs (mixture_model.py:122-186) per strand: K = 2 with sklearn's defaults on the rows of
 * every pair's canonical k-mer, closest_to_canonical against the -T / -C file's level mean, the other component into the
 * modified k-mer's row ({n = 1, m, s} at weight 0 gives m and s back exactly, and the mean^3 / sd^2 lambda of
 * set_kmer_event_mean_params).  The distances of all strands go into one file. */
static void write_mixture(const train_t *tr) {
    const run_t *R = tr->o.R;
    if (!R->mix_motifs) return;
    mix_row_t *rows = NULL;
    mix_pair_t *pairs[2] = {NULL, NULL};
    int64_t n_rows = 0;
    for (int s = 0; s < n_strands(R); s++) {
        if (!R->mix_model[s] && !R->mix_dist) continue;
        const strand_model_t *sm = &R->sm[s];
        int64_t nk = 1;
        for (int i = 0; i < sm->k; i++) nk *= sm->n_alpha;
        const int64_t np = mixture_pairs(R, s, &pairs[s]);
        int32_t *ids = xalloc(np, sizeof(int32_t), 1);
        sa_mixture_fit_t *fit = xalloc(np, sizeof(sa_mixture_fit_t), 1);
        sa_kmer_stat_t *st = xalloc(nk, sizeof(sa_kmer_stat_t), 1);
        uint8_t *mask = xalloc(nk, 1, 1);
        for (int64_t i = 0; i < np; i++) ids[i] = pairs[s][i].canonical;
        const sa_mixture_params_t mp = {2, 100, 1e-3, 1e-6};
        if (np > 0 && sa_kmer_table_mixture(tr->tab[s], s, ids, np, &mp, NULL, fit, NULL) != SA_OK)
            die("signalMachine: --train-mixture-*: the fit failed%s", "");
        rows = realloc(rows, (size_t) (n_rows + np + 1) * sizeof(mix_row_t));
        if (!rows) die("signalMachine: out of memory%s", "");
        for (int64_t i = 0; i < np; i++) {
            const mix_pair_t *q = &pairs[s][i];
            int32_t match = 0, other = 1;
            double distance = 0;
            if (fit[i].status != 0 || sa_mixture_assign(&fit[i], sm->table_orig[5 * q->canonical], &match, &other, &distance) != SA_OK) {
                fprintf(stderr, "No alignments found for kmer: %s\n", q->name[0]);
                continue;
            }
            st[q->modified].n = 1;
            st[q->modified].m = fit[i].mean[other];
            st[q->modified].s = fit[i].sd[other];
            mask[q->modified] = 1;
            mix_row_t *r = &rows[n_rows++];
            r->kmer = q->name[0];
            r->strand = s;
            r->v[0] = sm->table_orig[5 * q->canonical]; r->v[1] = sm->table_orig[5 * q->canonical + 1];
            r->v[2] = fit[i].mean[match]; r->v[3] = fit[i].sd[match];
            r->v[4] = fit[i].mean[other]; r->v[5] = fit[i].sd[other];
            r->v[6] = distance;
        }
        if (R->mix_model[s] && sa_model_write_trained(R->model_path[s], st, 0.0, 0.0, 0, mask, R->mix_model[s]) != SA_OK)
            die("signalMachine: cannot write %s", R->mix_model[s]);
        free(ids);
        free(fit);
        free(st);
        free(mask);
    }
    if (R->mix_dist) {
        FILE *f = fopen(R->mix_dist, "w");
        if (!f) die("signalMachine: cannot write %s", R->mix_dist);
        if (n_rows) qsort(rows, (size_t) n_rows, sizeof(mix_row_t), cmp_mix_row);
        fprintf(f, "kmer\tcanonical_model_mean\tcanonical_model_sd\tcanonical_mixture_mean\tcanonical_mixture_sd\tmodified_mixture_mean\t"
                   "modified_mixture_sd\tdistance\tstrand\n");
        for (int64_t i = 0; i < n_rows; i++) {
            fputs(rows[i].kmer, f);
            for (int q = 0; q < 7; q++) {
                char num[40];
                sa_format_py_repr(num, rows[i].v[q]);
                fprintf(f, "\t%s", num);
            }
            fprintf(f, "\t%c\n", rows[i].strand ? 'c' : 't');
        }
        if (fclose(f) != 0) die("signalMachine: cannot write %s", R->mix_dist);
    }
    free(rows);
    free(pairs[0]);
    free(pairs[1]);
}

/* --train-*: the assignments table (generate_top_n_kmers_from_sa_output) and the retrained models (train_normal_emmissions:
 * the prior is the -T / -C file as written on disk) */
static void train_finish(output_t *o) {
    train_t *tr = (train_t *) o;
    const run_t *R = o->R;
    for (int s = 0; s < n_strands(R); s++)   /* (a run without a read that aligned: empty tables) */
        if (train_table(tr, s) != SA_OK) die("signalMachine: --train-*: no k-mer table%s", "");
    if (R->train_pos_cov) write_train_coverage(tr);
    if (R->train_assign) {   /* the template table's 't' rows, then the complement table's 'c' rows */
        for (int s = 0; s < n_strands(R); s++)
            if (sa_kmer_table_write(tr->tab[s], s, R->train_assign, s > 0) != SA_OK) die("signalMachine: cannot write %s", R->train_assign);
    }
    for (int s = 0; s < n_strands(R); s++) {
        if (!R->train_model[s]) continue;
        const strand_model_t *sm = &R->sm[s];
        int64_t nk = 1;
        for (int i = 0; i < sm->k; i++) nk *= sm->n_alpha;
        sa_kmer_stat_t *st = calloc((size_t) nk, sizeof(sa_kmer_stat_t));
        uint8_t *mask = NULL;
        if (R->train_kmers) {   /* load_training_kmers (trainModels.py:704-719): a duplicate line is an error */
            FILE *f = fopen(R->train_kmers, "r");
            if (!f) die("signalMachine: cannot read %s", R->train_kmers);
            mask = calloc((size_t) nk, 1);
            char line[256];
            while (fgets(line, sizeof line, f)) {
                line[strcspn(line, "\r\n")] = 0;
                const int64_t id = (int64_t) strlen(line) == sm->k ? sa_kmer_id(sm->model, line) : -1;
                if (id < 0 || id >= nk) continue;   /* (a k-mer outside the model never matches, as in the reference) */
                if (mask[id]) die("signalMachine: --train-kmers: duplicate k-mer %s", line);
                mask[id] = 1;
            }
            fclose(f);
        }
        if (!st || sa_kmer_table_stats(tr->tab[s], s, R->train_median, st, NULL) != SA_OK)
            die("signalMachine: --train-*: statistics failed%s", "");
        if (sa_model_write_trained(R->model_path[s], st, R->train_weight, R->train_min_sd, R->train_mod_only, mask, R->train_model[s]) != SA_OK)
            die("signalMachine: cannot write %s", R->train_model[s]);
        free(st);
        free(mask);
    }
    write_mixture(tr);
    for (int s = 0; s < 2; s++) { sa_kmer_table_destroy(tr->tab[s]); tr->tab[s] = NULL; }
}
/* The tables are made at the run's first slice; a slice that starts over (a read the planner refuses) takes its rows back. */
static int train_checkpoint(output_t *o) {
    train_t *tr = (train_t *) o;
    const run_t *R = o->R;
    for (int s = 0; s < n_strands(R); s++) {
        int rc = train_table(tr, s);
        if (rc == SA_OK) rc = sa_kmer_table_checkpoint(tr->tab[s]);
        if (rc != SA_OK) die_opt(o->opt, sa_strerror(rc));
    }
    return SA_OK;
}
static int train_rollback(output_t *o) {
    int rc = SA_OK;
    for (int s = 0; s < n_strands(o->R) && rc == SA_OK; s++) rc = sa_kmer_table_rollback(((train_t *) o)->tab[s]);
    return rc;
}
static int train_add_batch(output_t *o, slice_t *sl, int s, sa_batch_t *b) {   /* (a batch that ran: nothing a retry without some reads would change) */
    train_t *tr = (train_t *) o;
    const run_t *R = o->R;
    int rc;
    if (R->train_pos) {   /* where each read's rows lie: write_full's reference_index (adjust_ref) as x0 + x_sign * x */
        sa_train_job_map_t *map = xalloc(sl->n_ok, sizeof(*map), 1);
        for (int64_t j = 0; j < sl->n_ok; j++) {
            const read_t *rd = &sl->reads[sl->who[j]];
            const int along = (s == 0 && rd->forward) || (s == 1 && !rd->forward);
            map[j].contig = train_contig(tr, rd->pA->contig1);
            map[j].x_sign = along ? 1 : -1;
            map[j].x0 = along ? rd->st[s].r_shift : rd->st[s].r_shift - R->sm[s].k;   /* len_kmers - (x + (len - off)), len_kmers = len - k */
            map[j].site_strand = along ? 0 : 1;   /* strand_pairs: forward t '+', c '-'; backward t '-', c '+' */
        }
        rc = sa_kmer_table_add_batch_at(tr->tab[s], b, sl->jobs[s], sl->n_ok, s, map, NULL);
        free(map);
    } else {
        rc = sa_kmer_table_add_batch(tr->tab[s], b, sl->jobs[s], sl->n_ok, s, NULL);
    }
    if (rc != SA_OK) die_opt(o->opt, sa_strerror(rc));
    return SA_OK;
}

/* ---- --position-profile: the profile of the run's template batches in one table on the GPU, laid over every record of -f ---- */
typedef struct {
    output_t o;
    sa_position_profile_t *tab;
} prof_t;
static void prof_open(output_t *o) {
    run_t *R = o->R;
    load_ref_records(R, o->opt);
    const int rc = sa_position_profile_create(&((prof_t *) o)->tab, R->sm[0].model, R->ref_lens, R->n_refs, R->device);
    if (rc != SA_OK) die_opt(o->opt, sa_strerror(rc));
}
static int prof_checkpoint(output_t *o) { return sa_position_profile_checkpoint(((prof_t *) o)->tab); }
static int prof_rollback(output_t *o) { return sa_position_profile_rollback(((prof_t *) o)->tab); }
/* the slice's finished template batch added to the run's table.  Job j is read j's template strand, and where its target lies on the
 * contig is snp_contig_pos written as an affine map, as marg_add_batch does */
static int prof_add_batch(output_t *o, slice_t *sl, int s, sa_batch_t *b) {
    const run_t *R = o->R;
    const int64_t nj = sl->n_ok;
    if (s != 0) return SA_OK;
    sa_profile_job_map_t *map = xalloc(nj, sizeof(*map), 1);
    for (int64_t j = 0; j < nj; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        const int same = snp_contig_pos_is_forward(rd, 0);
        map[j].contig = (int32_t) snp_contig_index(R, rd);
        map[j].pos_sign = same ? 1 : -1;
        map[j].pos0 = same ? rd->st[0].r_shift : rd->st[0].r_shift - 1;
    }
    const int rc = sa_position_profile_add_batch(((prof_t *) o)->tab, b, map, nj, 0, NULL);
    free(map);
    if (rc != SA_OK) die_opt(o->opt, sa_strerror(rc));
    return SA_OK;
}
/* at the end of the run: finish on the device, the script's file */
static void prof_finish(output_t *o) {
    prof_t *pr = (prof_t *) o;
    const run_t *R = o->R;
    sa_profile_site_t *sites = NULL;
    int64_t n = 0;
    uint32_t seen = 0;
    if (sa_position_profile_finish(pr->tab, (const char *const *) R->ref_seqs, &sites, &n, &seen, NULL) != SA_OK)
        die_opt(o->opt, "the final step failed");
    if (sa_position_profile_write(R->prof_path, R->sm[0].alphabet, seen, (const char *const *) R->ref_names, sites, n) != SA_OK)
        die("signalMachine: cannot write %s", R->prof_path);
    sa_free(sites);
    sa_position_profile_destroy(pr->tab);
    pr->tab = NULL;
}

/* ---- --guide-deviation: every strand batch's deviation from its guide (sa_batch_guide_deviation), written read by read ---- */
typedef struct {
    output_t o;
    FILE *fh, *events_fh;
    int64_t total[SA_DEV_MAX_BUCKETS];   /* the H lines written so far, summed: the T line */
} deviation_t;
static void dev_open(output_t *o) {
    deviation_t *d = (deviation_t *) o;
    const run_t *R = o->R;
    if (!(d->fh = fopen(R->dev_path, "w"))) die("signalMachine: cannot open output %s", R->dev_path);
    fprintf(d->fh, "#guide-deviation threshold=%d bucket_size=%d n_buckets=%d; R label strand status n_aligned n_flagged n_on_mea mean_abs "
                   "max_abs max_abs_mea max_event n_sets; H label strand counts; S label strand first_event last_event count peak "
                   "mea_peak center_event open_end; T counts\n", R->dev_params.threshold, R->dev_params.bucket_size, R->dev_params.n_buckets);
    if (R->dev_events_path) {
        if (!(d->events_fh = fopen(R->dev_events_path, "w"))) die("signalMachine: cannot open output %s", R->dev_events_path);
        fprintf(d->events_fh, "#label\tstrand\tevent_index\treference_index\tguide_reference_index\tdiff\ton_mea\tflagged\n");
    }
}
/* the finished batch of strand s against its own jobs' anchors, with the MEA paths just made of it */
static int dev_add_batch(output_t *o, slice_t *sl, int s, sa_batch_t *b) {
    const run_t *R = o->R;
    strand_result_t *sr = &sl->sr[s];
    const int64_t n = sl->n_ok;
    sa_deviation_job_t *dj = xalloc(n, sizeof(*dj), 1);
    sr->dev_ev_first = xalloc(n + 1, sizeof(int64_t), 1);
    for (int64_t j = 0; j < n; j++) {
        const sa_job_t *q = &sl->jobs[s][j];
        dj[j] = (sa_deviation_job_t) {q->anchor_x, q->anchor_y, q->n_anchors, q->n_events};
        sr->dev_ev_first[j + 1] = sr->dev_ev_first[j] + q->n_events;
    }
    sr->dev_reads = xalloc(n, sizeof(sa_deviation_read_t), 1);
    sr->dev_hist = xalloc(n * R->dev_params.n_buckets, sizeof(int32_t), 1);
    int64_t n_sets = 0;
    const int rc = sa_batch_guide_deviation(b, dj, n, (const sa_mea_pair_t *const *) sr->mea, sr->n_mea, &R->dev_params,
                                            R->dev_events_path ? SA_DEV_EVENTS : 0u, sr->dev_reads, &sr->dev_sets, &n_sets, sr->dev_hist, NULL,
                                            R->dev_events_path ? &sr->dev_events : NULL, NULL);
    free(dj);
    if (rc != SA_OK) die_opt(o->opt, sa_strerror(rc));
    return SA_OK;
}
/* ... and the lines of job j's strand s.  Events are printed as the TSV's event_index column prints them, positions as its
 * reference_index maps x; diff stays in the job's coordinates. */
static void dev_write_strand(deviation_t *d, const read_t *rd, int s, const strand_result_t *sr, int64_t j) {
    const run_t *R = d->o.R;
    const sa_deviation_read_t *r = &sr->dev_reads[j];
    const int nb = R->dev_params.n_buckets;
    const int64_t lo = rd->st[s].lo;
    const char *strand = s == 0 ? "t" : "c";
    char mean[400];
    mean[sa_format_f6(mean, r->n_aligned ? (double) r->sum_abs / (double) r->n_aligned : 0.0)] = 0;
    fprintf(d->fh, "R\t%s\t%s\t%d\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%s\t%d\t%d\t%" PRId64 "\t%d\n", rd->label, strand, r->status,
            r->n_aligned, r->n_flagged, r->n_on_mea, mean, r->max_abs, r->max_abs_mea, r->n_aligned ? lo + r->max_event : (int64_t) -1, r->n_sets);
    fprintf(d->fh, "H\t%s\t%s", rd->label, strand);
    for (int q = 0; q < nb; q++) {
        fprintf(d->fh, "\t%d", sr->dev_hist[j * nb + q]);
        d->total[q] += sr->dev_hist[j * nb + q];
    }
    fputc('\n', d->fh);
    for (int64_t i = 0; i < r->n_sets; i++) {
        const sa_deviation_set_t *t = &sr->dev_sets[r->set_first + i];
        fprintf(d->fh, "S\t%s\t%s\t%" PRId64 "\t%" PRId64 "\t%d\t%d\t%d\t%" PRId64 "\t%d\n", rd->label, strand, lo + t->first_event,
                lo + t->last_event, t->count, t->peak, t->mea_peak, lo + t->center_event, t->open_end);
    }
    if (!d->events_fh) return;
    const int64_t ref_len = (int64_t) strlen(rd->st[s].target), ref_len_kmers = ref_len - R->sm[s].k, off = rd->st[s].r_shift;
    const sa_deviation_event_t *ev = sr->dev_events + sr->dev_ev_first[j];
    for (int64_t y = 0; y < sr->dev_ev_first[j + 1] - sr->dev_ev_first[j]; y++) {
        if (!(ev[y].flags & 1u)) continue;
        fprintf(d->events_fh, "%s\t%s\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%d\t%d\t%d\n", rd->label, strand, lo + y,
                adjust_ref(ev[y].best_x, off, ref_len_kmers, ref_len, s == 0, rd->forward),
                adjust_ref(ev[y].guide, off, ref_len_kmers, ref_len, s == 0, rd->forward), ev[y].diff, (int) ((ev[y].flags >> 1) & 1u),
                (int) ((ev[y].flags >> 2) & 1u));
    }
}
static void dev_add_read(output_t *o, slice_t *sl, int64_t j) {
    for (int s = 0; s < n_strands(o->R); s++) dev_write_strand((deviation_t *) o, &sl->reads[sl->who[j]], s, &sl->sr[s], j);
}
static void dev_finish(output_t *o) {   /* the histogram summed over the reads written */
    deviation_t *d = (deviation_t *) o;
    fprintf(d->fh, "T");
    for (int q = 0; q < o->R->dev_params.n_buckets; q++) fprintf(d->fh, "\t%" PRId64, d->total[q]);
    fputc('\n', d->fh);
    if (fclose(d->fh) != 0 || (d->events_fh && fclose(d->events_fh) != 0)) die("signalMachine: cannot write %s", o->R->dev_path);
}

/* ---- --signal-labels: the labelled signal of every raw read of a template batch (sa_batch_signal_labels), written read by read as
 * the reads are rendered -- so a read the planner refused, whose slice started over, never has a file.  A read given as .npRead has
 * no raw starts: its job goes into the call with one-sample events (the call wants every job of the batch) and nothing is written. ---- */
static int lab_add_batch(output_t *o, slice_t *sl, int s, sa_batch_t *b) {
    const run_t *R = o->R;
    strand_result_t *sr = &sl->sr[s];
    const int64_t n = sl->n_ok;
    const int k = R->sm[s].k;
    sa_label_job_t *lj = xalloc(n, sizeof(*lj), 1);
    int64_t *plain = NULL, n_plain = 0;   /* 0, 1, 2, ...: the raw starts of the reads that have none */
    for (int64_t j = 0; j < n; j++)
        if (!sl->reads[sl->who[j]].raw_start && sl->jobs[s][j].n_events > n_plain) n_plain = sl->jobs[s][j].n_events;
    if (n_plain > 0) {
        plain = xalloc(2 * n_plain, sizeof(int64_t), 0);
        for (int64_t y = 0; y < n_plain; y++) { plain[y] = y; plain[n_plain + y] = 1; }
    }
    for (int64_t j = 0; j < n; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        const sa_job_t *q = &sl->jobs[s][j];
        const int same = (s == 0 && rd->forward) || (s == 1 && !rd->forward);   /* adjust_ref: x + off, or off - k - x */
        sa_label_job_t *l = &lj[j];
        l->n_events = q->n_events;
        l->ref_first = same ? rd->st[s].r_shift : rd->st[s].r_shift - k;
        l->ref_step = same ? 1 : -1;
        l->base_shift = same ? R->lab_kmer_index : (k - 1) - R->lab_kmer_index;
        if (rd->raw_start) {
            l->raw_start = rd->raw_start + rd->st[s].lo; l->raw_length = rd->raw_length + rd->st[s].lo; l->n_samples = rd->n_raw_samples;
        } else {
            l->raw_start = plain; l->raw_length = plain + n_plain; l->n_samples = q->n_events;
        }
    }
    sr->lab_reads = xalloc(n, sizeof(sa_label_read_t), 1);
    const unsigned flags = SA_LABEL_MEA | (R->lab_full ? SA_LABEL_FULL : 0u) | (R->lab_bands ? SA_LABEL_BANDS : 0u) | (R->lab_samples ? SA_LABEL_SAMPLES : 0u);
    const int rc = sa_batch_signal_labels(b, lj, n, (const sa_mea_pair_t *const *) sr->mea, sr->n_mea, flags, sr->lab_reads, &sr->lab_mea,
                                          R->lab_full ? &sr->lab_full : NULL, R->lab_bands ? &sr->lab_bands : NULL,
                                          R->lab_samples ? &sr->lab_samples : NULL, NULL);
    free(lj); free(plain);
    if (rc != SA_OK) die_opt(o->opt, sa_strerror(rc));
    return SA_OK;
}
static FILE *lab_file(const run_t *R, const read_t *rd, const char *suffix) {
    char *path = xalloc((int64_t) (strlen(R->lab_dir) + strlen(rd->label) + strlen(suffix) + 4), 1, 0);
    sprintf(path, "%s/%s.%s", R->lab_dir, rd->label, suffix);
    FILE *fh = fopen(path, "w");
    if (!fh) die("signalMachine: cannot open output %s", path);
    free(path);
    return fh;
}
/* raw_start raw_length reference_index posterior_probability kmer: the label dtype's fields in create_label_from_events' order, the
 * posterior as "%f" prints it, the k-mer spelled in full */
static void lab_write_segments(const run_t *R, const read_t *rd, const char *suffix, const sa_label_segment_t *seg, int64_t n) {
    FILE *fh = lab_file(R, rd, suffix);
    char kmer[16];
    for (int64_t i = 0; i < n; i++) {
        kmer_string(&R->sm[0], seg[i].kmer_id, kmer);
        fprintf(fh, "%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%d.%06d\t%s\n", seg[i].raw_start, seg[i].raw_length, seg[i].reference_index,
                seg[i].prob_units / 1000000, seg[i].prob_units % 1000000, kmer);
    }
    if (fclose(fh) != 0) die("signalMachine: cannot write the label files of %s", rd->label);
}
static void lab_add_read(output_t *o, slice_t *sl, int64_t j) {
    const run_t *R = o->R;
    const read_t *rd = &sl->reads[sl->who[j]];
    const strand_result_t *sr = &sl->sr[0];
    const sa_label_read_t *r = &sr->lab_reads[j];
    if (!rd->raw_start) {
        fprintf(stderr, "[signalMachine]NOTICE: %s is not given as raw current: no label files\n", rd->label);
        return;
    }
    lab_write_segments(R, rd, "labels.tsv", sr->lab_mea + r->mea_first, r->n_mea);
    if (R->lab_full) lab_write_segments(R, rd, "full.tsv", sr->lab_full + r->full_first, r->n_full);
    if (R->lab_bands) {
        FILE *fh = lab_file(R, rd, "bands.tsv");
        for (int64_t i = 0; i < r->n_bands; i++) {
            const sa_label_band_t *b = &sr->lab_bands[r->band_first + i];
            fprintf(fh, "%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%d\n", b->reference_index, b->raw_start, b->raw_length, b->n_records);
        }
        if (fclose(fh) != 0) die("signalMachine: cannot write the label files of %s", rd->label);
    }
    if (R->lab_samples) {   /* the covering MEA segment's reference_index per raw sample, little-endian int64 */
        FILE *fh = lab_file(R, rd, "samples.i64");
        const int32_t *at = sr->lab_samples + r->sample_first;
        const sa_label_segment_t *seg = sr->lab_mea + r->mea_first;
        unsigned char *buf = xalloc(r->n_samples > 0 ? r->n_samples : 1, 8, 0);
        for (int64_t t = 0; t < r->n_samples; t++) {
            const uint64_t v = (uint64_t) (at[t] < 0 ? (int64_t) -1 : seg[at[t]].reference_index);
            for (int q = 0; q < 8; q++) buf[8 * t + q] = (unsigned char) (v >> (8 * q));
        }
        if (fwrite(buf, 8, (size_t) r->n_samples, fh) != (size_t) r->n_samples || fclose(fh) != 0) die("signalMachine: cannot write the label files of %s", rd->label);
        free(buf);
    }
}

/* ---- --snp-marginals / --snp-proposals: the probabilities summed over all reads in one table on the GPU, laid over every record of -f ---- */
typedef struct {
    output_t o;
    sa_snp_marginals_t *tab;
} marg_t;
static int marg_checkpoint(output_t *o) { return sa_snp_marginals_checkpoint(((marg_t *) o)->tab); }
static int marg_rollback(output_t *o) { return sa_snp_marginals_rollback(((marg_t *) o)->tab); }
/* The finished batch of strand q added to the run's table.  Job j * N + s is read j's copy s: where its target lies on the contig
 * (snp_contig_pos), the reference_index of its records (adjust_ref), its direction, the read's place in the manifest as run
 * ordinal, and one window per (read, step).  (What it returns is the strand batch's: a refusal starts the slice over.) */
static int marg_add_batch(output_t *o, slice_t *sl, int q, sa_batch_t *b) {
    const run_t *R = o->R;
    const int64_t N = sl->per_read, nj = sl->n_ok * N;
    sa_snp_job_map_t *map = xalloc(nj, sizeof(*map), 1);
    for (int64_t j = 0; j < sl->n_ok; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        const int64_t ci = snp_contig_index(R, rd);
        const int same = (q == 0 && rd->forward) || (q == 1 && !rd->forward);
        const int64_t off = rd->st[q].r_shift, run = (int64_t) (rd - R->reads0);
        for (int64_t s = 0; s < N; s++) {
            sa_snp_job_map_t *m = &map[j * N + s];
            m->contig = (int32_t) ci;
            m->pos_sign = m->x_sign = same ? 1 : -1;
            m->pos0 = same ? off : off - 1;
            m->x0 = same ? off : off - R->sm[q].k;   /* adjust_ref: len_kmers - (x + (len - off)) with len_kmers = len - k */
            m->strand = q;
            m->direction = same;
            m->run = run;
            m->group = run * N + s;
        }
    }
    const int rc = sa_snp_marginals_add_batch(((marg_t *) o)->tab, b, map, nj, NULL);
    free(map);
    return rc;
}

static int cmp_i64(const void *a, const void *b) {
    const int64_t x = *(const int64_t *) a, y = *(const int64_t *) b;
    return x < y ? -1 : x > y;
}

/* --snp-sites: lines "contig<TAB>site[<TAB>...]" (a --snp-proposals file among them) into ascending lists per record */
static void load_snp_sites(run_t *R) {
    FILE *fh = fopen(R->snp_sites_path, "r");
    if (!fh) die("signalMachine: cannot read %s", R->snp_sites_path);
    R->sites = xalloc(R->n_refs, sizeof(int64_t *), 1);
    R->n_sites = xalloc(R->n_refs, sizeof(int64_t), 1);
    char line[4096], name[2048];
    while (fgets(line, sizeof line, fh)) {
        int64_t site = 0;
        if (line[0] == '\n' || line[0] == '#') continue;
        if (sscanf(line, "%2047[^\t]\t%" SCNd64, name, &site) != 2) die("signalMachine: --snp-sites: cannot parse a line of %s", R->snp_sites_path);
        int64_t ci = 0;
        while (ci < R->n_refs && strcmp(R->ref_names[ci], name) != 0) ci++;
        if (ci == R->n_refs || site < 0 || site >= R->ref_lens[ci]) die("signalMachine: --snp-sites: a site of %s is not in the -f reference", name);
        R->sites[ci] = realloc(R->sites[ci], sizeof(int64_t) * (size_t) (R->n_sites[ci] + 1));
        if (!R->sites[ci]) die("signalMachine: out of memory%s", "");
        R->sites[ci][R->n_sites[ci]++] = site;
    }
    fclose(fh);
    for (int64_t c = 0; c < R->n_refs; c++)
        if (R->n_sites[c]) qsort(R->sites[c], (size_t) R->n_sites[c], sizeof(int64_t), cmp_i64);
}
static void marg_open(output_t *o) {
    run_t *R = o->R;
    load_ref_records(R, o->opt);
    const int rc = sa_snp_marginals_create(&((marg_t *) o)->tab, R->ref_lens, R->n_refs, R->snp_step, R->device);
    if (rc != SA_OK) die_opt(o->opt, sa_strerror(rc));
    if (R->snp_sites_path) load_snp_sites(R);
}

/* --snp-reference-out: every record of -f with the calls applied, lines as wide as the input's first sequence line */
static void write_snp_reference(const run_t *R, const sa_snp_marginal_t *m, int64_t n) {
    int64_t width = 60;
    FILE *in = fopen(R->fwd_ref, "r");
    if (in) {
        char *buf = NULL;
        size_t cap = 0;
        ssize_t got;
        while ((got = getline(&buf, &cap, in)) >= 0)
            if (got > 0 && buf[0] != '>') {
                while (got > 0 && (buf[got - 1] == '\n' || buf[got - 1] == '\r')) got--;
                if (got > 0) width = (int64_t) got;
                break;
            }
        free(buf);
        fclose(in);
    }
    FILE *fh = fopen(R->snp_ref_out, "w");
    if (!fh) die("signalMachine: cannot write %s", R->snp_ref_out);
    for (int64_t c = 0; c < R->n_refs; c++) {
        char *out = xalloc(R->ref_lens[c] + 1, 1, 0);
        if (sa_snp_apply_calls(R->ref_seqs[c], R->ref_lens[c], m, n, (int32_t) c, out) != SA_OK) die("signalMachine: --snp-reference-out failed%s", "");
        fprintf(fh, ">%s\n", R->ref_names[c]);
        for (int64_t i = 0; i < R->ref_lens[c]; i += width)
            fprintf(fh, "%.*s\n", (int) (R->ref_lens[c] - i < width ? R->ref_lens[c] - i : width), out + i);
        free(out);
    }
    if (fclose(fh) != 0) die("signalMachine: cannot write %s", R->snp_ref_out);
}

/* at the end of the run: finish on the device, the table, the thinned proposals per contig */
static void marg_finish(output_t *o) {
    marg_t *mg = (marg_t *) o;
    const run_t *R = o->R;
    sa_snp_marginal_t *m = NULL;
    int64_t n = 0;
    if (sa_snp_marginals_finish(mg->tab, 1, (const char *const *) R->ref_seqs, &m, &n, NULL) != SA_OK) die_opt(o->opt, "the final step failed");
    if (sa_snp_write_marginals(R->snp_marg, (const char *const *) R->ref_names, m, n) != SA_OK) die("signalMachine: cannot write %s", R->snp_marg);
    if (R->snp_prop) {
        FILE *fh = fopen(R->snp_prop, "w");
        if (!fh) die("signalMachine: cannot write %s", R->snp_prop);
        int64_t *pos = xalloc(n, sizeof(int64_t), 0), *keep = xalloc(n, sizeof(int64_t), 0);
        double *delta = xalloc(n, sizeof(double), 0);
        for (int64_t a = 0; a < n;) {   /* the sites come in (contig, position) order: one contig after the other */
            int64_t e = a, np = 0, nk = 0;
            for (; e < n && m[e].contig == m[a].contig; e++)
                if (m[e].is_proposal) { pos[np] = m[e].pos; delta[np] = m[e].delta; np++; }
            if (sa_snp_group_sites(pos, delta, np, 6, 1, keep, &nk) != SA_OK) die("signalMachine: --snp-proposals failed%s", "");
            for (int64_t i = 0, j = 0; i < nk; i++) {   /* keep[] ascends, and so does pos[] */
                while (pos[j] != keep[i]) j++;
                char num[40];
                sa_format_py_repr(num, delta[j]);
                fprintf(fh, "%s\t%" PRId64 "\t%s\n", R->ref_names[m[a].contig], keep[i], num);
            }
            a = e;
        }
        free(pos); free(keep); free(delta);
        if (fclose(fh) != 0) die("signalMachine: cannot write %s", R->snp_prop);
    }
    if (R->snp_ref_out) write_snp_reference(R, m, n);
    sa_free(m);
    sa_snp_marginals_destroy(mg->tab);
    mg->tab = NULL;
}

/* ---- the outputs of this run, in the order they are opened in: the only place that knows which there are ---- */
static output_t *output_new(run_t *R, int wanted, size_t size, output_t hooks) {
    if (!wanted) return NULL;
    output_t *o = xalloc(1, size, 1);
    *o = hooks;
    o->R = R;
    return R->out[R->n_out++] = o;
}
static void outputs_open(run_t *R) {
    output_new(R, R->snp_marg != NULL, sizeof(marg_t), (output_t) {.opt = "--snp-marginals", .open = marg_open, .checkpoint = marg_checkpoint, .rollback = marg_rollback, .add_batch = marg_add_batch, .finish = marg_finish});
    output_new(R, R->prof_path != NULL, sizeof(prof_t), (output_t) {.opt = "--position-profile", .open = prof_open, .checkpoint = prof_checkpoint, .rollback = prof_rollback, .add_batch = prof_add_batch, .finish = prof_finish});
    output_t *agg = output_new(R, R->want_agg, sizeof(agg_t), (output_t) {.opt = "--site-calls-aggregate", .add_read = agg_add_read, .finish = agg_finish});
    output_t *acc = output_new(R, R->acc_path != NULL, sizeof(acc_t), (output_t) {.opt = "--site-calls-accuracy", .open = acc_open, .checkpoint = acc_checkpoint, .rollback = acc_rollback, .add_batch = acc_add_batch, .rendered = acc_rendered, .finish = acc_finish});
    if (acc) ((acc_t *) acc)->agg = (agg_t *) agg;
    output_t *cq = output_new(R, R->cq_path != NULL, sizeof(callq_t), (output_t) {.opt = "--site-calls-accuracy-quality", .open = cq_open, .add_batch = cq_add_batch, .add_read = cq_add_read, .finish = cq_finish});
    if (cq) ((callq_t *) cq)->acc = (acc_t *) acc;
    output_new(R, R->want_train, sizeof(train_t), (output_t) {.opt = "--train-*", .open = train_open, .checkpoint = train_checkpoint, .rollback = train_rollback, .add_batch = train_add_batch, .finish = train_finish});
    output_new(R, R->dev_path != NULL, sizeof(deviation_t), (output_t) {.opt = "--guide-deviation", .open = dev_open, .add_batch = dev_add_batch, .add_read = dev_add_read, .finish = dev_finish});
    output_new(R, R->lab_dir != NULL, sizeof(output_t), (output_t) {.opt = "--signal-labels", .add_batch = lab_add_batch, .add_read = lab_add_read});
    for (int i = 0; i < R->n_out; i++)
        if (R->out[i]->open) R->out[i]->open(R->out[i]);
}
static void outputs_checkpoint(run_t *R, int back) {   /* ... or, with `back`, roll back to it */
    for (int i = 0; i < R->n_out; i++) {
        int (*const step)(output_t *) = back ? R->out[i]->rollback : R->out[i]->checkpoint;
        if (step && step(R->out[i]) != SA_OK) die_opt(R->out[i]->opt, back ? "rollback failed" : "checkpoint failed");
    }
}
static int outputs_add_batch(slice_t *sl, int s, sa_batch_t *b) {
    int rc = SA_OK;
    for (int i = 0; i < sl->R->n_out && rc == SA_OK; i++)
        if (sl->R->out[i]->add_batch) rc = sl->R->out[i]->add_batch(sl->R->out[i], sl, s, b);
    return rc;
}
static void outputs_add_read(slice_t *sl, int64_t j) {
    for (int i = 0; i < sl->R->n_out; i++)
        if (sl->R->out[i]->add_read) sl->R->out[i]->add_read(sl->R->out[i], sl, j);
}
static void outputs_rendered(slice_t *sl) {
    for (int i = 0; i < sl->R->n_out; i++)
        if (sl->R->out[i]->rendered) sl->R->out[i]->rendered(sl->R->out[i], sl);
}
static void outputs_finish(run_t *R) {
    for (int i = 0; i < R->n_out; i++)
        if (R->out[i]->finish) R->out[i]->finish(R->out[i]);
}
