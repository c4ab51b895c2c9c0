/* signalMachine's writers of per-read files: the TSV renderings, the .expectations, .mea and .calls files (part of signalMachine.c's translation unit) */
static double descale(double e, double level, double scale, double shift, double var) {
    return (e + var * level - scale * level - shift) / var;
}

/* Rows are put together in a line buffer and handed to stdio as bytes: "%f" through sa_format_f6 (the same characters as
 * printf, tests/test_host_ambig.py), integers and strings by hand.  With fprintf a row of the full format cost 0.8 us of
 * formatter on every one of 11 million rows of a 1000-read batch; rendering was the largest stage of the front door. */
static char *put_s(char *p, const char *s) {
    while (*s) *p++ = *s++;
    return p;
}
static char *put_i64(char *p, int64_t v) {
    char t[24];
    int n = 0;
    uint64_t u = v < 0 ? (uint64_t) 0 - (uint64_t) v : (uint64_t) v;
    if (v < 0) *p++ = '-';
    do { t[n++] = (char) ('0' + u % 10); u /= 10; } while (u);
    while (n) *p++ = t[--n];
    return p;
}
static char *put_f(char *p, double v) { return p + sa_format_f6(p, v); }
static void reverse_complement_into(const char *s, int k, char *out) {   /* sa_reverse_complement of a k-mer, no allocation */
    for (int i = 0; i < k; i++) {
        const char c = s[k - 1 - i];
        out[i] = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C'
               : c == 'a' ? 't' : c == 't' ? 'a' : c == 'c' ? 'g' : c == 'g' ? 'c' : c;
    }
    out[k] = 0;
}
static FILE *open_rows(const char *path) {
    FILE *fh = fopen(path, "a");
    if (!fh) die("signalMachine: cannot open output %s", path);
    setvbuf(fh, NULL, _IOFBF, 1 << 20);
    return fh;
}

/* writePosteriorProbsFull, impl/signalMachine.c:89-159 */
static void write_full(const char *path, const out_ctx_t *o) {
    FILE *fh = open_rows(path);
    const size_t fixed = strlen(o->contig) + strlen(o->label);
    char *line = xalloc((int64_t) fixed + 640, 1, 0);   /* nine "%f" of at most 320 characters... in theory; 24 for sane values */
    const int k = o->sm->k;
    int64_t ref_len = (int64_t) strlen(o->target), ref_len_kmers = ref_len - k;
    char k_i[16], path_kmer[16];
    for (int64_t i = 0; i < o->n_pairs; i++) {
        const sa_pair_t *p = &o->pairs[i];
        int64_t x_adj = adjust_ref(p->x, o->ref_offset, ref_len_kmers, ref_len, o->is_template, o->forward);
        int64_t y = p->y + o->event_offset;
        double prob = ((double) p->prob_e7) / PROB_1;
        double ev_mean = o->events[y * 4], ev_noise = o->events[y * 4 + 1], ev_dur = o->events[y * 4 + 2];
        memcpy(k_i, o->target + p->x, k);
        k_i[k] = 0;
        kmer_string(o->sm, p->kmer_id, path_kmer);
        double E_mean = o->sm->table[(int64_t) p->kmer_id * 5];
        /* emissions_signal_scaleNoise (impl/stateMachine.c:721-741) rescales the table per read; applied on the fly here */
        double E_noise = o->sm->table[(int64_t) p->kmer_id * 5 + 2] * o->npp.scale_sd;
        double scaled_Emean = E_mean * o->npp.scale + o->npp.shift;
        double scaled_Enoise = E_noise * o->npp.scale_sd;
        double descaled = descale(ev_mean, E_mean, o->npp.scale, o->npp.shift, o->npp.var);
        char ref_kmer[16], tmp[16];
        if ((o->is_template && o->forward) || (!o->is_template && !o->forward)) memcpy(ref_kmer, k_i, (size_t) k + 1);
        else reverse_complement_into(k_i, k, ref_kmer);
        if (o->rna) {
            reverse_complement_into(ref_kmer, k, tmp);
            memcpy(ref_kmer, tmp, (size_t) k + 1);
        }
        const double vals[9] = {ev_mean, ev_noise, ev_dur, scaled_Emean, scaled_Enoise, prob, descaled, E_mean, 0.0};
        int wide = 0;   /* a value the 24-character budget does not hold: the formatter's own path */
        for (int q = 0; q < 8; q++) wide |= !(fabs(vals[q]) < 9.0e15);
        if (wide) {
            fprintf(fh, "%s\t%" PRId64 "\t%s\t%s\t%s\t%" PRId64 "\t%f\t%f\t%f\t%s\t%f\t%f\t%f\t%f\t%f\t%s\n", o->contig, x_adj,
                    ref_kmer, o->label, o->is_template ? "t" : "c", y, ev_mean, ev_noise, ev_dur, k_i, scaled_Emean,
                    scaled_Enoise, prob, descaled, E_mean, path_kmer);
            continue;
        }
        char *w = line;
        w = put_s(w, o->contig); *w++ = '\t';
        w = put_i64(w, x_adj); *w++ = '\t';
        w = put_s(w, ref_kmer); *w++ = '\t';
        w = put_s(w, o->label); *w++ = '\t';
        *w++ = o->is_template ? 't' : 'c'; *w++ = '\t';
        w = put_i64(w, y); *w++ = '\t';
        w = put_f(w, ev_mean); *w++ = '\t';
        w = put_f(w, ev_noise); *w++ = '\t';
        w = put_f(w, ev_dur); *w++ = '\t';
        w = put_s(w, k_i); *w++ = '\t';
        w = put_f(w, scaled_Emean); *w++ = '\t';
        w = put_f(w, scaled_Enoise); *w++ = '\t';
        w = put_f(w, prob); *w++ = '\t';
        w = put_f(w, descaled); *w++ = '\t';
        w = put_f(w, E_mean); *w++ = '\t';
        w = put_s(w, path_kmer); *w++ = '\n';
        fwrite(line, 1, (size_t) (w - line), fh);
    }
    free(line);
    fclose(fh);
}

/* writePosteriorProbsVC, impl/signalMachine.c:161-232: only k-mers holding the internal ambiguity letter X */
static void write_vc(const char *path, const out_ctx_t *o) {
    int forward = o->forward;
    int label_forward = (o->rna || !o->is_template) ? !forward : forward;
    FILE *fh = open_rows(path);
    char *line = xalloc((int64_t) (strlen(o->contig) + strlen(o->label)) + 768, 1, 0);
    const int k = o->sm->k;
    int64_t ref_len = (int64_t) strlen(o->target), ref_len_kmers = ref_len - k;
    char k_i[16], path_kmer[16];
    for (int64_t i = 0; i < o->n_pairs; i++) {
        const sa_pair_t *p = &o->pairs[i];
        memcpy(k_i, o->target + p->x, k);
        k_i[k] = 0;
        int same = (o->is_template && forward) || (!o->is_template && !forward);
        char ref_kmer[16];
        if (same) memcpy(ref_kmer, k_i, (size_t) k + 1);
        else reverse_complement_into(k_i, k, ref_kmer);
        if (!strchr(ref_kmer, 'X')) continue;
        int64_t x_adj = adjust_ref(p->x, o->ref_offset, ref_len_kmers, ref_len, o->is_template, forward);
        int64_t y = p->y + o->event_offset;
        double prob = ((double) p->prob_e7) / PROB_1;
        kmer_string(o->sm, p->kmer_id, path_kmer);
        for (int q = 0; q < k; q++) {
            if (ref_kmer[q] != 'X') continue;
            int qp = same ? q : (k - 1) - q; /* adjustQueryPosition :81-87 */
            char *w = line;
            w = put_i64(w, y); *w++ = '\t';
            w = put_i64(w, x_adj + q); *w++ = '\t';
            *w++ = path_kmer[qp]; *w++ = '\t';
            w = put_f(w, prob); *w++ = '\t';
            *w++ = o->is_template ? 't' : 'c'; *w++ = '\t';
            w = put_s(w, label_forward ? "forward" : "backward"); *w++ = '\t';
            w = put_s(w, o->label); *w++ = '\t';
            w = put_f(w, o->score); *w++ = '\t';
            w = put_s(w, o->contig); *w++ = '\n';
            fwrite(line, 1, (size_t) (w - line), fh);
        }
    }
    free(line);
    fclose(fh);
}

/* writeAssignments, impl/signalMachine.c:234-270 */
static void write_assignments(const char *path, const out_ctx_t *o) {
    FILE *fh = open_rows(path);
    char path_kmer[16], line[704];
    for (int64_t i = 0; i < o->n_pairs; i++) {
        const sa_pair_t *p = &o->pairs[i];
        int64_t y = p->y + o->event_offset;
        double prob = ((double) p->prob_e7) / PROB_1;
        kmer_string(o->sm, p->kmer_id, path_kmer);
        double E_mean = o->sm->table[(int64_t) p->kmer_id * 5];
        double descaled = descale(o->events[y * 4], E_mean, o->npp.scale, o->npp.shift, o->npp.var);
        char *w = line;
        w = put_s(w, path_kmer); *w++ = '\t';
        *w++ = o->is_template ? 't' : 'c'; *w++ = '\t';
        w = put_f(w, descaled); *w++ = '\t';
        w = put_f(w, prob); *w++ = '\n';
        fwrite(line, 1, (size_t) (w - line), fh);
    }
    fclose(fh);
}

static void output_alignment(int64_t fmt, const char *f1, const char *f2, const out_ctx_t *o) {
    switch (fmt) {
        case 0: write_full(f1, o); break;
        case 1: write_vc(f1, o); break;
        case 2: write_assignments(f1, o); break;
        case 3: write_full(f1, o); write_vc(f2, o); break;
        default: fprintf(stderr, "signalAlign - No valid output format provided\n");
    }
}

/* continuousPairHmm_writeToFile (impl/continuousHmm.c:352-408) / hdpHmm_writeToFile (:572-623): the library's Hmm object
 * (sa_hmm_*), filled with what sa_expect_batch returned for the read.  `trans` already holds the transition pseudocount. */
static void write_expectations(const char *path, const strand_model_t *sm, const sa_strand_params_t *npp, int hdp, double threshold,
                               const double *trans, double lik, const sa_job_t *job, const sa_assignment_t *as,
                               int64_t n_as) {
    sa_hmm_t *h = NULL;
    int rc = sa_hmm_create(&h, sm->model, hdp ? SA_HMM_HDP : SA_HMM_GAUSSIAN, threshold, 0.0, 0.001 /* emissionsPseudocount, :785 */);
    if (rc != SA_OK) die("signalMachine: cannot build the expectations object: %s", sa_strerror(rc));
    int64_t n_kmers = 1;
    for (int i = 0; i < sm->k; i++) n_kmers *= sm->n_alpha;
    /* the event model is the state machine's table after this read's emissions_signal_scaleNoise
     * (impl/stateMachine.c:721-741: noise_mean *= scale_sd, noise_lambda *= var_sd, noise_sd = sqrt(mean^3 / lambda)) */
    double *em = malloc(sizeof(double) * 5 * (size_t) n_kmers);
    if (!em) die("signalMachine: out of memory%s", "");
    for (int64_t i = 0; i < n_kmers * 5; i += 5) {
        const double nm = sm->table[i + 2] * npp->scale_sd, nl = sm->table[i + 4] * npp->var_sd;
        em[i] = sm->table[i]; em[i + 1] = sm->table[i + 1]; em[i + 2] = nm; em[i + 3] = sqrt(pow(nm, 3.0) / nl); em[i + 4] = nl;
    }
    sa_hmm_set_event_model(h, em);
    free(em);
    sa_hmm_add_expectations(h, trans, lik);
    for (int64_t i = 0; hdp && i < n_as; i++)
        sa_hmm_add_assignment(h, job->ref + as[i].ref_pos, job->events[as[i].event * job->event_stride]);
    rc = sa_hmm_write(h, path);
    sa_hmm_destroy(h);
    if (rc != SA_OK) die("signalMachine: cannot open %s for writing", path);
}

/* The rows of the full output that lie on the maximum-expected-accuracy path -- what mea_alignment_from_signal_align
 * (src/signalalign/mea_algorithm.py:323-341) returns as its final event table, here as a TSV next to the posteriors file.
 * The path holds one (x, y) per event; where several rows share a cell (ambiguous positions) the row with the lowest
 * posterior is the one the reference's matrix keeps (get_mea_params_from_events :305-318). */
static void write_mea(const char *post_path, const out_ctx_t *o, const sa_mea_pair_t *path, int64_t n_path) {
    char *out_path = malloc(strlen(post_path) + 8);
    sprintf(out_path, "%s.mea", post_path);
    int64_t y_max = -1;
    for (int64_t i = 0; i < n_path; i++) y_max = path[i].event_idx > y_max ? path[i].event_idx : y_max;
    int64_t *x_of = malloc(sizeof(int64_t) * (size_t) (y_max + 2)), *best = malloc(sizeof(int64_t) * (size_t) (y_max + 2));
    for (int64_t y = 0; y <= y_max; y++) { x_of[y] = -1; best[y] = -1; }
    for (int64_t i = 0; i < n_path; i++) x_of[path[i].event_idx] = path[i].ref_idx;
    for (int64_t i = 0; i < o->n_pairs; i++) {
        const sa_pair_t *p = &o->pairs[i];
        if (p->y > y_max || x_of[p->y] != p->x) continue;
        if (best[p->y] < 0 || p->prob_e7 < o->pairs[best[p->y]].prob_e7) best[p->y] = i;
    }
    sa_pair_t *rows = xalloc(n_path, sizeof(sa_pair_t), 0);
    int64_t n = 0;
    for (int64_t i = 0; i < o->n_pairs; i++) {   /* output order of the posteriors file */
        const sa_pair_t *p = &o->pairs[i];
        if (p->y <= y_max && best[p->y] == i) rows[n++] = *p;
    }
    out_ctx_t m = *o;
    m.pairs = rows;
    m.n_pairs = n;
    write_full(out_path, &m);
    free(rows); free(x_of); free(best); free(out_path);
}

/* ---- --site-calls / --site-calls-aggregate: MarginalizeFullVariants.get_data and AggregateOverReadsFull
 * (src/signalalign/variantCaller.py:92-187, :393-410) over the calls sa_batch_site_calls made on the device ---- */
typedef struct { int64_t pos, i; } call_pos_t;
/* does any of the strand's pairs sit on a reference k-mer that holds an ambiguity letter (a variant_data row of get_data, :112)? */
static int has_ambiguous_rows(const char *const *ambig, const char *target, int k, const sa_pair_t *pairs, int64_t n) {
    const int64_t len = (int64_t) strlen(target);
    int64_t *last = malloc(sizeof(int64_t) * (size_t) (len + 1));   /* last[i]: the last ambiguous position below i, -1 none */
    int64_t prev = -1;
    for (int64_t i = 0; i <= len; i++) {
        last[i] = prev;
        if (i < len && ambig[(unsigned char) target[i]]) prev = i;
    }
    int found = 0;
    for (int64_t i = 0; i < n && !found; i++) {
        const int64_t end = (int64_t) pairs[i].x + k;
        found = end <= len && last[end] >= pairs[i].x;
    }
    free(last);
    return found;
}
static int cmp_call_pos(const void *a, const void *b) {
    const int64_t x = ((const call_pos_t *) a)->pos, y = ((const call_pos_t *) b)->pos;
    return x < y ? -1 : x > y;
}
/* The calls of one strand of a read in the order get_data walks them (:141-144): by the reference_index the TSV prints for the
 * site's k-mer (adjust_ref), ascending, reversed when the strand's mapping strand is '-'.  The mapping strand (:128-131, :179):
 * mapping_strands[mapping_index], where the index starts at 0 and moves on after every read strand that has variant_data rows --
 * rows whose reference k-mer holds an ambiguity letter (:112), whether or not one of them is a site.  So the complement gets
 * mapping_strands[1] exactly when the template has such a row (`tmpl_amb`, template_has_ambiguous_rows). */
static call_pos_t *order_calls(const read_t *rd, int s, int tmpl_amb, const sa_site_call_t *calls, int64_t n, int k, char *mapped) {
    const int idx = (s == 1 && tmpl_amb) ? 1 : 0;
    *mapped = (idx == 0) == (rd->forward != 0) ? '+' : '-';
    const int64_t ref_len = (int64_t) strlen(rd->st[s].target), ref_len_kmers = ref_len - k, off = rd->st[s].r_shift;
    call_pos_t *v = xalloc(n, sizeof(call_pos_t), 0);
    for (int64_t i = 0; i < n; i++) {
        v[i].pos = adjust_ref(calls[i].x, off, ref_len_kmers, ref_len, s == 0, rd->forward);
        v[i].i = i;
    }
    qsort(v, (size_t) n, sizeof(call_pos_t), cmp_call_pos);
    if (*mapped == '-')
        for (int64_t a = 0, b = n - 1; a < b; a++, b--) { call_pos_t t = v[a]; v[a] = v[b]; v[b] = t; }
    return v;
}
/* <posteriors>.calls: label contig position strand forward_mapped letters p_1 .. p_n (one row per reported site) */
static void write_calls(const char *post_path, const read_t *rd, int s, int tmpl_amb, const sa_site_call_t *calls, int64_t n, int k) {
    char *out_path = malloc(strlen(post_path) + 8);
    sprintf(out_path, "%s.calls", post_path);
    FILE *fh = open_rows(out_path);
    char mapped;
    call_pos_t *v = order_calls(rd, s, tmpl_amb, calls, n, k, &mapped);
    char *line = malloc(strlen(rd->label) + strlen(rd->pA->contig1) + 512);
    for (int64_t q = 0; q < n; q++) {
        const sa_site_call_t *c = &calls[v[q].i];
        char *w = line;
        w = put_s(w, rd->label); *w++ = '\t';
        w = put_s(w, rd->pA->contig1); *w++ = '\t';
        w = put_i64(w, v[q].pos); *w++ = '\t';
        *w++ = s == 0 ? 't' : 'c'; *w++ = '\t';
        *w++ = mapped; *w++ = '\t';
        for (int l = 0; l < c->n_letters; l++) *w++ = c->letters[l];
        for (int l = 0; l < c->n_letters; l++) { *w++ = '\t'; w = put_f(w, c->prob[l]); }
        *w++ = '\n';
        fwrite(line, 1, (size_t) (w - line), fh);
    }
    free(line); free(v); free(out_path);
    fclose(fh);
}

static out_ctx_t out_ctx_for(const run_t *R, const read_t *rd, int s, const sa_pair_t *pairs, int64_t n_pairs, double score) {
    out_ctx_t o;
    o.label = rd->label; o.contig = rd->pA->contig1; o.sm = &R->sm[s]; o.npp = *np_params(rd->np, s);
    o.events = np_events(rd->np, s); o.target = rd->st[s].target; o.forward = rd->forward; o.is_template = s == 0;
    o.rna = R->rna; o.event_offset = rd->st[s].lo; o.ref_offset = rd->st[s].r_shift; o.pairs = pairs;
    o.n_pairs = n_pairs; o.score = score;
    return o;
}
