/* signalMachine's reads: the manifest, the host side of one read (prepare_read) and the stages that run ahead of it on the GPU -- raw
 * current, locate, guide alignment (part of signalMachine.c's translation unit) */
static int estimate_strand(const strand_model_t *sm, const int64_t *strand_map, double *events, int64_t n_events,
                           const char *read, int64_t read_len, sa_strand_params_t *out, sa_model_t **read_model) {
    int64_t n = 5;
    for (int i = 0; i < sm->k; i++) n *= sm->n_alpha;
    double *scratch = malloc(sizeof(double) * (size_t) n); /* the estimation rescales the noise columns in place */
    if (!scratch) return SA_ENOMEM;
    memcpy(scratch, sm->table_orig, sizeof(double) * (size_t) n);
    double est[7];
    int rc = sa_estimate_params(sm->model, scratch, strand_map, events, n_events, read, read_len, est);
    if (rc == SA_OK && read_model) {   /* the model this read is aligned with: the rescaled noise columns, two-distribution emission */
        rc = sa_model_clone_with_table(read_model, sm->model, scratch);
        if (rc == SA_OK) rc = sa_model_set_emission(*read_model, SA_EMISSION_TWO_DIST);
    }
    free(scratch);
    if (rc != SA_OK) return rc;
    out->scale = est[0]; out->shift = est[1]; out->var = est[2]; out->drift = est[3];
    out->scale_sd = est[4]; out->var_sd = est[5]; out->shift_sd = est[6];
    return SA_OK;
}

/* plans `per_read` jobs per strand alone on the host (integer geometry only, no GPU); marks the read failed when the planner
 * rejects one */
static int validate_read(const run_t *R, read_t *rd, const sa_job_t *const jobs[2], int64_t per_read) {
    for (int s = 0; s < n_strands(R); s++)
        for (int64_t i = 0; i < per_read; i++) {
            int rc = sa_plan_describe(R->sm[s].model, &R->p, &jobs[s][i], R->ambig, 0, NULL, NULL, 0, NULL, 0, NULL, 0);
            if (rc != SA_OK) return fail(rd, 0, "alignment job rejected: %s", sa_strerror(rc));
        }
    return 0;
}

/* one strand of a read: estimate the read's parameters (signalUtils_estimateNanoporeParams), build the job from the guide
 * alignment's anchors */
static int build_strand_job(const run_t *R, read_t *rd, int s, const int64_t *gx, const int64_t *gy) {
    sa_npread_t *np = rd->np;
    sa_strand_params_t *pp = np_params(np, s);
    if (estimate_strand(&R->sm[s], np_strand_map(np, s), np_events(np, s), np_n_events(np, s), np_read(np, s), np_read_length(np, s), pp,
                        R->two_dist && !R->batch_mode ? &rd->model[s] : NULL) != SA_OK)
        return -1;
    sa_job_t *job = &rd->jobs[s];
    rd->ax[s] = xalloc(rd->n_guide + 1, sizeof(int64_t), 0);
    rd->ay[s] = xalloc(rd->n_guide + 1, sizeof(int64_t), 0);
    job->n_anchors = sa_remap_anchors(gx, gy, rd->n_guide, np_event_map(np, s, R->two_d), rd->pA->start2, rd->ax[s], rd->ay[s]);
    job->anchor_x = rd->ax[s]; job->anchor_y = rd->ay[s];
    job->ref = rd->st[s].target;
    job->ref_len = (int64_t) strlen(rd->st[s].target);
    job->events = np_events(np, s) + 4 * rd->st[s].lo;
    job->event_stride = 4;
    job->n_events = rd->st[s].hi - rd->st[s].lo;
    job->scale = pp->scale; job->shift = pp->shift; job->var = pp->var;
    return 0;
}

/* everything of impl/signalMachine.c:main between option parsing and performSignalAlignment, for one read */
static int prepare_read(const run_t *R, read_t *rd, int fatal) {
    const double tp0 = now_s();
    if (rd->failed) return -1;   /* the guide stage gave up on it */
    if (rd->pA == NULL) {        /* (a read with a guide window has its alignment, and its .npRead, from guide_stage) */
        if (rd->cigar_path == NULL) return fail(rd, fatal, "[signalMachine]ERROR: Need to provide input guide alignments, exiting", NULL);
        if (sa_cigar_load(rd->cigar_path, &rd->pA) != SA_OK)
            return fail(rd, fatal, "[signalMachine]ERROR: Didn't find input alignment file, looked %s", rd->cigar_path);
        fprintf(stderr, "[signalMachine]NOTICE: Using guide alignments from %s\n", rd->cigar_path);
    }
    sa_cigar_t *pA = rd->pA;
    if (rd->np == NULL && (rd->npread_path == NULL || sa_npread_load(rd->npread_path, &rd->np) != SA_OK))
        return fail(rd, fatal, "signalMachine: could not load the nanopore read %s", rd->npread_path);
    sa_npread_t *np = rd->np;
    if (pA->start2 < 0 || pA->end2 <= pA->start2 || pA->end2 > (R->two_d ? np->read_length : np->template_read_length))
        return fail(rd, fatal, "signalMachine: guide alignment of %s does not fit the read", rd->label);
    if (R->rna) {
        int64_t tmp = pA->start2;
        pA->start2 = np->template_read_length - pA->end2;
        pA->end2 = np->template_read_length - tmp;
    }
    const double tp1 = now_s();
    t_add(&g_ts_parse, tp1 - tp0);
    const char *seq_name = rd->seq_name ? rd->seq_name : pA->contig1;
    if (R->fwd_ref == NULL || seq_name == NULL)
        return fail(rd, fatal, "[signalMachine] ERROR: need -f <fasta> and -n <sequence name>", NULL);

    /* fastaHandler_ReferenceSequenceConstructFull, impl/fasta_handler.c:47-102 */
    if (R->rna) { /* listReverse(pA->operationList) */
        for (int64_t i = 0, j = pA->n_ops - 1; i < j; i++, j--) {
            int32_t t = pA->op_type[i]; pA->op_type[i] = pA->op_type[j]; pA->op_type[j] = t;
            int64_t l = pA->op_len[i]; pA->op_len[i] = pA->op_len[j]; pA->op_len[j] = l;
        }
    }
    int ferr = 0;
    rd->forward_seq = pA->strand1 ? sa_fasta_fetch(R->fwd_ref, seq_name, pA->start1, pA->end1 - 1, &ferr)
                                  : sa_fasta_fetch(R->fwd_ref, seq_name, pA->end1, pA->start1 - 1, &ferr);
    if (ferr == -2) {
        fprintf(stderr, "[signalMachine] ERROR %d: sequence name: %s is not in reference fasta: %s \n", ferr, seq_name, R->fwd_ref);
        if (fatal) exit(1);
        return fail(rd, 0, "sequence name %s is not in the reference fasta", seq_name);
    }
    if (rd->forward_seq == NULL) return fail(rd, fatal, "[signalMachine] ERROR: Unable to fetch reference sequence.  ", NULL);
    rd->win_lo = pA->strand1 ? pA->start1 : pA->end1;
    if (R->bwd_ref) {
        rd->backward_seq = pA->strand1 ? sa_fasta_fetch(R->bwd_ref, seq_name, pA->start1, pA->end1 - 1, &ferr)
                                       : sa_fasta_fetch(R->bwd_ref, seq_name, pA->end1, pA->start1 - 1, &ferr);
        if (rd->backward_seq == NULL) return fail(rd, fatal, "[signalMachine] ERROR: Unable to fetch reference sequence.  ", NULL);
        sa_reverse_in_place(rd->backward_seq);
    } else {
        rd->backward_seq = sa_complement(rd->forward_seq);
        sa_reverse_in_place(rd->backward_seq);
    }
    int strand1 = pA->strand1;
    if (R->rna) {
        char *tmp = rd->backward_seq;
        rd->backward_seq = strdup(rd->forward_seq);
        sa_reverse_in_place(rd->backward_seq);
        free(rd->forward_seq);
        rd->forward_seq = tmp;
        sa_reverse_in_place(rd->forward_seq);
        int64_t t2 = pA->start1;
        pA->start1 = pA->end1;
        pA->end1 = t2;
        pA->strand1 = !pA->strand1;
        strand1 = pA->strand1;
    }
    rd->st[0].target = strand1 ? rd->forward_seq : rd->backward_seq;
    rd->st[1].target = strand1 ? rd->backward_seq : rd->forward_seq;

    /* event slices and coordinate shifts (impl/signalMachine.c:726-750) */
    for (int s = 0; s < n_strands(R); s++) {
        const int64_t *map = np_event_map(np, s, R->two_d);
        rd->st[s].lo = map[pA->start2];
        rd->st[s].hi = map[pA->end2 - 1];
    }
    rd->st[0].r_shift = pA->start1;
    rd->st[1].r_shift = R->two_d ? pA->end1 : 0;
    rd->forward = pA->strand1;

    const double tp2 = now_s();
    t_add(&g_ts_fetch, tp2 - tp1);
    /* anchors from the guide alignment (pA is rebased inside, impl/signalMachineUtils.c:142-164) */
    int64_t cap = 0;
    for (int64_t i = 0; i < pA->n_ops; i++) cap += pA->op_len[i];
    int64_t *gx = xalloc(cap + 1, sizeof(int64_t), 0), *gy = xalloc(cap + 1, sizeof(int64_t), 0);
    rd->n_guide = sa_guide_to_anchors(pA->start1, pA->end1, pA->strand1, pA->start2, pA->op_type, pA->op_len, pA->n_ops,
                                      R->constraint_trim, gx, gy, cap + 1);
    int built = rd->n_guide < 0 ? -1 : 0;
    memset(rd->jobs, 0, sizeof(rd->jobs));
    for (int s = 0; s < n_strands(R) && built == 0; s++) built = build_strand_job(R, rd, s, gx, gy);
    free(gx);
    free(gy);
    if (rd->n_guide < 0) return fail(rd, fatal, "signalMachine: could not convert the guide alignment", NULL);
    if (built != 0) return fail(rd, fatal, "Cannot get scale params with no assignments", NULL);
    t_add(&g_ts_estimate, now_s() - tp2);
    /* batch mode: the reads of a slice share one GPU batch, and the planner rejects a whole batch for one bad job (a
     * reference window with a letter outside the alphabet, anchors that give an invalid diagonal).  The reference runs one
     * process per read, so only that read may fail.  Alignment runs find the offender when -- and only when -- a batch is
     * turned down (drop_refused_reads below); the expectation routine writes files strand by strand and cannot be re-run, so
     * its jobs are planned alone on the host here. */
    if (!fatal && R->expect_mode) {
        const sa_job_t *const own[2] = {&rd->jobs[0], &rd->jobs[1]};
        return validate_read(R, rd, own, 1);
    }
    return 0;
}

static char *dup_field(const char *s) { return (s == NULL || s[0] == 0 || strcmp(s, "-") == 0) ? NULL : strdup(s); }

/* manifest of --batch: label, npRead, cigar, posteriors [, posteriors2, sequence_name, template expectations, complement expectations] */
static int64_t load_manifest(const char *path, read_t **out) {
    FILE *fh = fopen(path, "r");
    if (!fh) return -1;
    int64_t n = 0, cap = 0;
    read_t *reads = NULL;
    char *line = NULL;
    size_t lcap = 0;
    while (getline(&line, &lcap, fh) >= 0) {
        size_t len = strlen(line);
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (len == 0 || line[0] == '#') continue;
        char *f[8] = {0};
        int nf = 0;
        for (char *tok = line; tok && nf < 8;) {
            char *tab = strchr(tok, '\t');
            if (tab) *tab = 0;
            f[nf++] = tok;
            tok = tab ? tab + 1 : NULL;
        }
        if (nf < 4) { fprintf(stderr, "[signalMachine] batch manifest: line with %d fields ignored (need at least 4)\n", nf); continue; }
        if (n == cap) {
            cap = cap ? cap * 2 : 64;
            reads = realloc(reads, sizeof(read_t) * (size_t) cap);
        }
        read_t *rd = &reads[n++];
        memset(rd, 0, sizeof(*rd));
        rd->label = strdup(f[0]);
        rd->npread_path = dup_field(f[1]);
        rd->cigar_path = dup_field(f[2]);
        if (rd->cigar_path && rd->cigar_path[0] == '@') {   /* @<contig>:<start>-<end>[:+|:-]: computed, not read; @ alone: located first */
            if (rd->cigar_path[1] == 0) rd->guide_locate = 1;
            else rd->guide_window = strdup(rd->cigar_path + 1);
            free(rd->cigar_path);
            rd->cigar_path = NULL;
        }
        rd->post_path = dup_field(f[3]);
        rd->post_path2 = dup_field(f[4]);
        rd->seq_name = dup_field(f[5]);
        rd->expect[0] = dup_field(f[6]);
        rd->expect[1] = dup_field(f[7]);
    }
    free(line);
    fclose(fh);
    *out = reads;
    return n;
}

/* ---- reads given as raw current --------------------------------------------------------------------------------------------- */
/* The reads of a slice whose -q / manifest file is a raw-read file (sa_io.h): ONE sa_npread_from_raw_batch call -- event detection,
 * MoM scalings, event alignment and the base-to-event map on the GPU -- gives each the sa_npread_t that sa_npread_load would have
 * read from the .npRead the reference's Python writes for a 1D read: template read, strand event map, events, the default
 * parameters (estimate_strand replaces them).  From there on it is a read like any other.  A read the chain rejects fails as a
 * read with an unreadable .npRead does. */
static void raw_stage(const run_t *R, read_t *reads, int64_t n_reads) {
    int64_t n = 0;
    for (int64_t i = 0; i < n_reads; i++) n += reads[i].raw && !reads[i].failed;
    if (n == 0) return;
    const int fatal = !R->batch_mode;
    read_t **rd = xalloc(n, sizeof(read_t *), 0);
    sa_rawread_t **rr = xalloc(n, sizeof(sa_rawread_t *), 1);
    sa_raw_job_t *jobs = xalloc(n, sizeof(sa_raw_job_t), 1);
    const char **seq = xalloc(n, sizeof(char *), 0);
    n = 0;
    for (int64_t i = 0; i < n_reads; i++) {
        read_t *r = &reads[i];
        if (!r->raw || r->failed) continue;
        sa_rawread_t *w = NULL;
        const int rc = sa_rawread_load(r->npread_path, &w);
        if (rc != SA_OK) { fail(r, fatal, "signalMachine: could not load the raw read %s", r->npread_path); continue; }
        if (w->seq_len < R->sm[0].k) {
            sa_rawread_free(w);
            fail(r, fatal, "signalMachine: the sequence of the raw read %s is shorter than the model's k-mers", r->npread_path);
            continue;
        }
        rd[n] = r;
        rr[n] = w;
        jobs[n] = (sa_raw_job_t) {w->samples, w->n_samples, w->digitisation, w->offset, w->range, w->sample_rate, w->start_time};
        seq[n++] = w->sequence;
    }
    sa_raw_npread_t *out = xalloc(n, sizeof(sa_raw_npread_t), 1);
    const int rc = n > 0 ? sa_npread_from_raw_batch(R->sm[0].model, jobs, seq, n, R->raw_detector_set ? &R->raw_detector : NULL, R->device, 0,
                                                    out, NULL) : SA_OK;
    for (int64_t q = 0; q < n; q++) {
        read_t *r = rd[q];
        const sa_raw_npread_t *o = &out[q];
        if (rc != SA_OK) { fail(r, fatal, "signalMachine: the raw reads could not be turned into events: %s", sa_strerror(rc)); continue; }
        if (o->status != 0) {
            char what[160];
            snprintf(what, sizeof(what), "%s (status %d)", (o->status & SA_RAW_MAP_LENGTH) ? "Read and event map lengths do not match"
                     : (o->status & SA_RAW_NO_PEAK) ? "the event detector found no event boundary"
                     : "its events do not align to its sequence", (int) o->status);
            fail(r, fatal, "signalMachine: no event table for the raw read: %s", what);
            continue;
        }
        if (R->npread_out) {
            char *path = xalloc((int64_t) (strlen(R->npread_out) + strlen(r->label) + 16), 1, 0);
            sprintf(path, "%s/%s.npRead", R->npread_out, r->label);
            if (sa_raw_npread_write(o, seq[q], R->sm[0].model, path) != SA_OK) fprintf(stderr, "[signalMachine]WARNING: cannot write %s\n", path);
            free(path);
        }
        sa_npread_t *np = xalloc(1, sizeof(sa_npread_t), 1);
        np->template_params = np->complement_params = (sa_strand_params_t) {1, 1, 1, 1, 1, 0, 0};   /* the .npRead's 1 1 1 1 1 0 */
        np->n_template_events = o->n_events;
        np->template_read_length = o->read_len;
        np->two_d_read = strdup("");
        np->complement_read = strdup("");
        np->template_read = strdup(seq[q]);
        np->template_strand_event_map = xalloc(o->read_len, sizeof(int64_t), 0);
        memcpy(np->template_strand_event_map, o->strand_event_map, sizeof(int64_t) * (size_t) o->read_len);
        np->template_events = xalloc(4 * o->n_events, sizeof(double), 0);
        memcpy(np->template_events, o->events4, sizeof(double) * 4 * (size_t) o->n_events);
        r->np = np;
        if (R->lab_dir || R->cq_path) {   /* --signal-labels, --site-calls-accuracy-quality: where every event lies in the raw current */
            r->raw_start = xalloc(o->n_events, sizeof(int64_t), 0);
            r->raw_length = xalloc(o->n_events, sizeof(int64_t), 0);
            memcpy(r->raw_start, o->raw_start, sizeof(int64_t) * (size_t) o->n_events);
            memcpy(r->raw_length, o->raw_length, sizeof(int64_t) * (size_t) o->n_events);
            r->n_raw_samples = rr[q]->n_samples;
        }
        fprintf(stderr, "[signalMachine]NOTICE: %s from raw current: %" PRId64 " samples, %" PRId64 " events on %" PRId64 " bases (shift %f, scale %f)\n",
                r->label, rr[q]->n_samples, o->n_events, o->read_len, o->mom_shift, o->mom_scale);
    }
    sa_raw_npread_free(out, n);
    for (int64_t q = 0; q < n; q++) sa_rawread_free(rr[q]);
    free(out); free(seq); free(jobs); free(rr); free(rd);
}

/* ---- guide alignment on the GPU --------------------------------------------------------------------------------------------- */
/* <contig>:<start>-<end>[:+|:-], read from the right (a contig name may hold colons); strand: 1 '+', 0 '-', -1 not given */
static int parse_guide_window(const char *spec, char **contig, int64_t *start, int64_t *end, int *strand) {
    size_t len = strlen(spec);
    *strand = -1;
    if (len >= 2 && spec[len - 2] == ':' && (spec[len - 1] == '+' || spec[len - 1] == '-')) {
        *strand = spec[len - 1] == '+';
        len -= 2;
    }
    size_t colon = len;
    while (colon > 0 && spec[colon - 1] != ':') colon--;
    if (colon < 2) return -1;   /* no colon, or an empty contig name */
    char range[64];
    if (len - colon == 0 || len - colon >= sizeof(range)) return -1;
    memcpy(range, spec + colon, len - colon);
    range[len - colon] = 0;
    char *dash = NULL, *stop = NULL;
    if (!isdigit((unsigned char) range[0])) return -1;
    const long long a = strtoll(range, &dash, 10);
    if (*dash != '-' || !isdigit((unsigned char) dash[1])) return -1;
    const long long b = strtoll(dash + 1, &stop, 10);
    if (*stop != 0 || b <= a) return -1;
    *contig = strndup(spec, colon - 1);
    *start = a;
    *end = b;
    return 0;
}

typedef struct {
    read_t *rd;
    char *contig, *oriented;   /* the window as the read is aligned to it: forward or reverse complement */
    int64_t w_start, w_len, crop;
    int reverse;
    sa_guide_job_t job;
} guide_item_t;

typedef struct {
    const run_t *R;
    guide_item_t *items;
} guide_ctx_t;

/* host side of one read: the .npRead, the window, the seed */
static void guide_prepare_one(int64_t i, void *ctx) {
    const guide_ctx_t *g = ctx;
    const run_t *R = g->R;
    guide_item_t *it = &g->items[i];
    read_t *rd = it->rd;
    const int fatal = !R->batch_mode;
    int64_t w_end = 0;
    if (rd->failed) return;   /* the raw stage gave up on it */
    int strand = -1;
    if (parse_guide_window(rd->guide_window, &it->contig, &it->w_start, &w_end, &strand) != 0) {
        fail(rd, fatal, "signalMachine: cannot read the guide window %s (want <contig>:<start>-<end>[:+|:-])", rd->guide_window);
        return;
    }
    if (R->fwd_ref == NULL) { fail(rd, fatal, "[signalMachine] ERROR: a guide window needs -f <fasta>", NULL); return; }
    if (rd->np == NULL && (rd->npread_path == NULL || sa_npread_load(rd->npread_path, &rd->np) != SA_OK)) {   /* (locate_stage loads it too) */
        fail(rd, fatal, "signalMachine: could not load the nanopore read %s", rd->npread_path);
        return;
    }
    const char *read = R->two_d ? rd->np->two_d_read : rd->np->template_read;
    const int64_t read_len = R->two_d ? rd->np->read_length : rd->np->template_read_length;
    int ferr = 0;
    char *window = sa_fasta_fetch(R->fwd_ref, it->contig, it->w_start, w_end - 1, &ferr);
    if (window == NULL) {
        fail(rd, fatal, ferr == -2 ? "sequence name %s is not in the reference fasta" : "[signalMachine] ERROR: Unable to fetch the guide window %s",
             ferr == -2 ? it->contig : rd->guide_window);
        return;
    }
    it->w_len = (int64_t) strlen(window);
    int64_t diag = 0, votes = 0, hits = 0;
    int reverse = 0, seeded;
    if (strand == 0) {   /* told: minus */
        it->oriented = sa_reverse_complement(window);
        free(window);
        seeded = sa_guide_seed(read, read_len, it->oriented, it->w_len, 0, &diag, &reverse, &votes, &hits) == 0;
        reverse = 1;
    } else {
        seeded = sa_guide_seed(read, read_len, window, it->w_len, strand < 0, &diag, &reverse, &votes, &hits) == 0;
        if (seeded && reverse) {
            it->oriented = sa_reverse_complement(window);
            free(window);
        } else {
            it->oriented = window;
            reverse = 0;
        }
    }
    if (!seeded) diag = 0;
    it->reverse = reverse;
    /* the band absorbs what lies within it of the seed's diagonal: the window starts band / 2 before */
    it->crop = seeded && diag > R->guide_band / 2 ? diag - R->guide_band / 2 : 0;
    it->job.read = read;
    it->job.read_len = read_len;
    it->job.ref = it->oriented + it->crop;
    it->job.ref_len = it->w_len - it->crop;
    it->job.diag = diag - it->crop;
}

/* The -f reference's index: built on first need, once per process, resident on the device until the process ends */
static sa_ref_index_t *g_ref_index = NULL;
static int g_ref_index_rc = SA_OK, g_ref_index_tried = 0;
static pthread_mutex_t g_ref_index_mu = PTHREAD_MUTEX_INITIALIZER;

static int ref_index_get(const run_t *R, sa_ref_index_t **out) {
    pthread_mutex_lock(&g_ref_index_mu);
    if (!g_ref_index_tried) {
        g_ref_index_tried = 1;
        g_ref_index_rc = sa_ref_index_build_fasta(&g_ref_index, R->fwd_ref, R->device);
        sa_ref_index_info_t info;
        if (g_ref_index_rc == SA_OK && sa_ref_index_info(g_ref_index, &info) == SA_OK)
            fprintf(stderr, "[signalMachine]NOTICE: Indexed %s: %" PRId64 " contigs, %" PRId64 " bases, %" PRId64 " 15-mers, %.2f s\n", R->fwd_ref,
                    info.n_contigs, info.total_bases, info.n_entries, info.build_seconds);
    }
    *out = g_ref_index;
    const int rc = g_ref_index_rc;
    pthread_mutex_unlock(&g_ref_index_mu);
    return rc;
}

typedef struct {
    const run_t *R;
    read_t **rd;
} locate_ctx_t;

static void locate_load_one(int64_t i, void *ctx) {
    const locate_ctx_t *c = ctx;
    read_t *rd = c->rd[i];
    if (rd->np == NULL && (rd->npread_path == NULL || sa_npread_load(rd->npread_path, &rd->np) != SA_OK))   /* (raw_stage fills it too) */
        fail(rd, !c->R->batch_mode, "signalMachine: could not load the nanopore read %s", rd->npread_path);
}

/* The reads of a slice that name neither a cigar file nor a window: ONE sa_guide_locate_batch call against the index of the whole
 * -f reference; a located read gets the window spec that sa_locate_window gives and is a read with a guide window from there on.
 * A read without a location fails as a read with an unreadable cigar file does. */
static void locate_stage(const run_t *R, read_t *reads, int64_t n_reads) {
    int64_t n = 0;
    for (int64_t i = 0; i < n_reads; i++) n += reads[i].guide_locate && reads[i].guide_window == NULL && !reads[i].failed;
    if (n == 0) return;
    const int fatal = !R->batch_mode;
    read_t **rd = xalloc(n, sizeof(read_t *), 0);
    n = 0;
    for (int64_t i = 0; i < n_reads; i++)
        if (reads[i].guide_locate && reads[i].guide_window == NULL && !reads[i].failed) rd[n++] = &reads[i];
    sa_ref_index_t *idx = NULL;
    int rc = R->fwd_ref == NULL ? SA_EINVAL : ref_index_get(R, &idx);
    if (rc != SA_OK) {
        for (int64_t i = 0; i < n; i++)
            fail(rd[i], fatal, R->fwd_ref == NULL ? "[signalMachine] ERROR: --guide-locate needs -f <fasta>%s"
                 : "signalMachine: the reference could not be indexed: %s", R->fwd_ref == NULL ? "" : sa_strerror(rc));
        free(rd);
        return;
    }
    locate_ctx_t ctx = {R, rd};
    parallel_for(n, locate_load_one, &ctx);
    const char **seq = xalloc(n, sizeof(char *), 0);
    int64_t *len = xalloc(n, sizeof(int64_t), 0), *who = xalloc(n, sizeof(int64_t), 0), n_live = 0;
    for (int64_t i = 0; i < n; i++) {
        if (rd[i]->failed) continue;
        seq[n_live] = R->two_d ? rd[i]->np->two_d_read : rd[i]->np->template_read;
        len[n_live] = R->two_d ? rd[i]->np->read_length : rd[i]->np->template_read_length;
        who[n_live++] = i;
    }
    sa_locate_result_t *res = xalloc(n_live, sizeof(sa_locate_result_t), 1);
    rc = n_live > 0 ? sa_guide_locate_batch(idx, seq, len, n_live, NULL, 0, res, NULL) : SA_OK;
    for (int64_t q = 0; q < n_live; q++) {
        read_t *r = rd[who[q]];
        const sa_locate_result_t *l = &res[q];
        if (rc != SA_OK) { fail(r, fatal, "signalMachine: the read could not be located: %s", sa_strerror(rc)); continue; }
        int64_t start = 0, end = 0;
        const char *contig = NULL;
        if ((l->status & (SA_LOCATE_NONE | SA_LOCATE_EMPTY)) || sa_locate_window(idx, l, len[q], R->guide_band, &start, &end) != SA_OK ||
            sa_ref_index_contig(idx, l->contig, &contig, NULL, NULL) != SA_OK) {
            fail(r, fatal, "signalMachine: no location for the read in %s", R->fwd_ref);
            continue;
        }
        r->guide_window = xalloc((int64_t) strlen(contig) + 64, 1, 0);
        sprintf(r->guide_window, "%s:%" PRId64 "-%" PRId64 ":%c", contig, start, end, l->reverse ? '-' : '+');
        fprintf(stderr, "[signalMachine]NOTICE: Read located at %s (%" PRId64 " votes, next %" PRId64 ")\n", r->guide_window, l->votes,
                l->second_votes);
        if (l->status & SA_LOCATE_AMBIGUOUS)
            fprintf(stderr, "[signalMachine]WARNING: the location of %s is ambiguous: another locus has %" PRId64 " votes against %" PRId64 "\n",
                    r->label, l->second_votes, l->votes);
        if (l->status & SA_LOCATE_OVERFLOW)
            fprintf(stderr, "[signalMachine]WARNING: %s has more 15-mer hits than the vote keeps (overflow): the later ones did not vote\n", r->label);
    }
    free(res); free(who); free(len); free(seq); free(rd);
}

/* The reads of a slice that name a window instead of a cigar file: ONE sa_guide_align_batch call, ahead of prepare_read's
 * remaining work; the result becomes the read's sa_cigar_t.  A read whose alignment is unusable fails as a read with an unusable
 * cigar file does. */
static void guide_stage(const run_t *R, read_t *reads, int64_t n_reads) {
    int64_t n = 0;
    for (int64_t i = 0; i < n_reads; i++) n += reads[i].guide_window != NULL;
    if (n == 0) return;
    const int fatal = !R->batch_mode;
    guide_item_t *items = xalloc(n, sizeof(guide_item_t), 1);
    n = 0;
    for (int64_t i = 0; i < n_reads; i++)
        if (reads[i].guide_window != NULL) items[n++].rd = &reads[i];
    guide_ctx_t ctx = {R, items};
    parallel_for(n, guide_prepare_one, &ctx);
    sa_guide_job_t *jobs = xalloc(n, sizeof(sa_guide_job_t), 1);
    int64_t *who = xalloc(n, sizeof(int64_t), 0), n_jobs = 0;
    for (int64_t i = 0; i < n; i++)
        if (!items[i].rd->failed) { jobs[n_jobs] = items[i].job; who[n_jobs++] = i; }
    sa_guide_result_t *res = xalloc(n_jobs, sizeof(sa_guide_result_t), 1);
    int32_t *op_type = NULL;
    int64_t *op_len = NULL;
    sa_guide_params_t prm = {2, -4, 4, 2, -1, R->guide_band, 0.5};
    int rc = n_jobs > 0 ? sa_guide_align_batch(jobs, n_jobs, &prm, R->device, 0, res, &op_type, &op_len, NULL) : SA_OK;
    for (int64_t q = 0; q < n_jobs; q++) {
        guide_item_t *it = &items[who[q]];
        read_t *rd = it->rd;
        if (rc != SA_OK) { fail(rd, fatal, "signalMachine: the guide alignment could not be computed: %s", sa_strerror(rc)); continue; }
        const sa_guide_result_t *r = &res[q];
        if (r->status & ~SA_GUIDE_BAND_EDGE) {
            fail(rd, fatal, r->status & (SA_GUIDE_NO_ALIGNMENT | SA_GUIDE_EMPTY) ? "signalMachine: no guide alignment of the read inside %s"
                 : r->status & SA_GUIDE_SHORT ? "signalMachine: the guide alignment inside %s covers less than half of the read"
                 : "signalMachine: the guide alignment inside %s could not be traced", rd->guide_window);
            continue;
        }
        if (r->status & SA_GUIDE_BAND_EDGE)
            fprintf(stderr, "[signalMachine]WARNING: the guide alignment of %s touches the edge of its band (--guide-band %d): it may be clipped\n",
                    rd->label, R->guide_band);
        /* window coordinates of the aligned stretch in the orientation it was aligned in, then forward contig coordinates */
        const int64_t a = it->crop + r->ref_start, b = it->crop + r->ref_end;
        const int64_t fs = it->w_start + (it->reverse ? it->w_len - b : a), fe = it->w_start + (it->reverse ? it->w_len - a : b);
        sa_cigar_t *c = xalloc(1, sizeof(sa_cigar_t), 1);
        c->contig1 = strdup(it->contig);
        c->contig2 = strdup(rd->label);
        c->start2 = r->read_start; c->end2 = r->read_end; c->strand2 = 1;
        c->start1 = it->reverse ? fe : fs; c->end1 = it->reverse ? fs : fe; c->strand1 = !it->reverse;
        c->score = (double) r->score;
        c->n_ops = r->n_ops;
        c->op_type = xalloc(r->n_ops, sizeof(int32_t), 0);
        c->op_len = xalloc(r->n_ops, sizeof(int64_t), 0);
        memcpy(c->op_type, op_type + r->op_first, sizeof(int32_t) * (size_t) r->n_ops);
        memcpy(c->op_len, op_len + r->op_first, sizeof(int64_t) * (size_t) r->n_ops);
        rd->pA = c;
        rd->seq_name = strdup(it->contig);   /* the window names the contig, whatever -n says */
        fprintf(stderr, "[signalMachine]NOTICE: Guide alignment computed on the GPU inside %s: read %" PRId64 "-%" PRId64 " on %s %" PRId64 "-%" PRId64
                        " %c, score %" PRId64 "\n", rd->guide_window, c->start2, c->end2, c->contig1, fs, fe, it->reverse ? '-' : '+', r->score);
        if (R->guide_cigars_out) {
            const int64_t need = sa_guide_format_cigar(rd->label, c->start2, c->end2, c->contig1, fs, fe, !it->reverse, r->score, c->op_type,
                                                       c->op_len, c->n_ops, NULL, 0);
            char *line = xalloc(need + 1, 1, 0);
            sa_guide_format_cigar(rd->label, c->start2, c->end2, c->contig1, fs, fe, !it->reverse, r->score, c->op_type, c->op_len, c->n_ops,
                                  line, need + 1);
            char *path = xalloc((int64_t) (strlen(R->guide_cigars_out) + strlen(rd->label) + 16), 1, 0);
            sprintf(path, "%s/%s.cigar", R->guide_cigars_out, rd->label);
            FILE *fh = fopen(path, "w");
            if (fh) { fprintf(fh, "%s\n", line); fclose(fh); }
            else fprintf(stderr, "[signalMachine]WARNING: cannot write %s\n", path);
            free(path);
            free(line);
        }
    }
    sa_free(op_type);
    sa_free(op_len);
    for (int64_t i = 0; i < n; i++) { free(items[i].contig); free(items[i].oriented); }
    free(res); free(who); free(jobs); free(items);
}

/* what a read holds once its outputs are written */
static void release_read(read_t *rd) {
    if (rd->pA) sa_cigar_free(rd->pA);
    if (rd->np) sa_npread_free(rd->np);
    free(rd->forward_seq); free(rd->backward_seq);
    free(rd->raw_start); free(rd->raw_length);
    rd->raw_start = rd->raw_length = NULL;
    for (int s = 0; s < 2; s++) { free(rd->ax[s]); free(rd->ay[s]); rd->ax[s] = rd->ay[s] = NULL; }
    for (int s = 0; s < 2; s++) { if (rd->model[s]) sa_model_destroy(rd->model[s]); rd->model[s] = NULL; }
    rd->pA = NULL; rd->np = NULL; rd->forward_seq = rd->backward_seq = NULL;
}
