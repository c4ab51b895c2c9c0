/* signalMachine's slices: the reads of one GPU batch per strand model, the loop that starts a slice over without the reads the
 * planner refuses, and the three modes (part of signalMachine.c's translation unit) */
static void prep_one(int64_t i, void *ctx) {
    const slice_t *sl = ctx;
    read_t *rd = &sl->reads[i];
    if (prepare_read(sl->R, rd, !sl->R->batch_mode) != 0)
        fprintf(stderr, "[signalMachine] ERROR: read %s skipped: %s\n", rd->label, rd->err);
}

/* host side of every read of a slice (files, parameter estimation, anchors): all host threads */
static void *slice_prepare(void *arg) {
    slice_t *sl = arg;
    const double ts0 = now_s();
    raw_stage(sl->R, sl->reads, sl->n_reads);
    locate_stage(sl->R, sl->reads, sl->n_reads);
    guide_stage(sl->R, sl->reads, sl->n_reads);
    parallel_for(sl->n_reads, prep_one, sl);
    t_add(&g_t_prep, now_s() - ts0);
    return NULL;
}

/* the GPU stage of a slice starts here: who[0 .. n_ok) are the reads whose host side went through */
static void slice_open(slice_t *sl, run_t *R, read_t *reads, int64_t n_reads) {
    memset(sl, 0, sizeof(*sl));
    sl->R = R; sl->reads = reads; sl->n_reads = n_reads;
    sl->validated = !R->batch_mode;   /* a single-read run has nobody to isolate a bad job from */
    sl->per_read = R->snp_step > 0 ? R->snp_step : 1;   /* (--snp-sites: one copy per read) */
    sl->who = xalloc(n_reads, sizeof(int64_t), 0);
    for (int64_t i = 0; i < n_reads; i++)
        if (!reads[i].failed) sl->who[sl->n_ok++] = i;
}

/* The jobs of the slice's batches, filled once: per_read copies of every read's own job per strand.  --snp-step N: copy s is aligned
 * to the read's window with X at the contig positions = s (mod N); --snp-sites: the one copy with X at the listed sites of the
 * read's contig (replace_periodic_reference_positions; the default ambiguity table makes X the four bases). */
static void slice_build_jobs(slice_t *sl) {
    const run_t *R = sl->R;
    const int64_t N = sl->per_read;
    sl->n_slots = sl->n_ok * N;
    for (int q = 0; q < n_strands(R); q++) {
        sl->jobs[q] = xalloc(sl->n_slots, sizeof(sa_job_t), 1);
        if (snp_mode(R)) sl->tgt[q] = xalloc(sl->n_slots, sizeof(char *), 1);
    }
    for (int64_t j = 0; j < sl->n_ok; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        for (int q = 0; q < n_strands(R); q++) {
            for (int64_t s = 0; s < N; s++) sl->jobs[q][j * N + s] = rd->jobs[q];
            if (!sl->tgt[q]) continue;
            const char *t = rd->st[q].target;
            const int from_fwd = t == rd->forward_seq;   /* forward_seq[i] at win_lo + i, backward_seq[i] at hi - i */
            const int64_t len = (int64_t) strlen(t), hi = rd->win_lo + (int64_t) strlen(rd->forward_seq) - 1;
            for (int64_t s = 0; s < N; s++) {
                char *o = xalloc(len + 1, 1, 0);
                if (R->sites) {
                    const int64_t ci = snp_contig_index(R, rd);
                    sa_snp_substitute_sites(t, len, from_fwd ? rd->win_lo : hi, !from_fwd, R->sites[ci], R->n_sites[ci], 'X', o);
                } else {
                    sa_snp_substitute(t, len, from_fwd ? rd->win_lo : hi, !from_fwd, N, s, 'X', o);
                }
                sl->tgt[q][j * N + s] = o;
                sl->jobs[q][j * N + s].ref = o;
            }
        }
    }
}

/* ... and ends here: the reads' memory goes back; returns the number of the slice's reads that failed */
static int64_t slice_close(slice_t *sl) {
    int64_t n_failed = 0;
    for (int64_t i = 0; i < sl->n_reads; i++) n_failed += sl->reads[i].failed ? 1 : 0;
    for (int64_t i = 0; i < sl->n_reads; i++) release_read(&sl->reads[i]);
    for (int q = 0; q < 2; q++) {
        for (int64_t i = 0; i < sl->n_slots && sl->tgt[q]; i++) free(sl->tgt[q][i]);
        free(sl->tgt[q]); free(sl->jobs[q]);
    }
    free(sl->who);
    return n_failed;
}

/* the summary line on stdout (n == NULL: none, the expectations mode) and the SUCCESS line on stderr of one alignment of a read */
static void report_read(const run_t *R, const read_t *rd, const int64_t *n, const double *score) {
    if (n) {
        fprintf(stdout, "%s %" PRId64 "\t%" PRId64 "(%f)\t", rd->label, rd->n_guide, n[0], score[0]);
        if (R->two_d) fprintf(stdout, "%" PRId64 "(%f)\n", n[1], score[1]);
        else fprintf(stdout, "\n");
    }
    fprintf(stderr, "signalAlign - SUCCESS: finished alignment of query %s, exiting\n", rd->label);
}

/* The planner turned a strand's batch down with `rc` (a letter outside the alphabet, anchors that give no band, a cell of more
 * paths or a matrix larger than the result records can name -- SA_EUNSUPPORTED --, ...): find the reads whose jobs it rejects
 * (each planned alone on the host, all host threads) and let them fail alone, as the reference's one-process-per-read runs
 * would.  Once per slice, never for a single read, nor when the device or its memory is what is missing.  Returns 1 when reads
 * were dropped: who, the jobs and their targets are closed up (a refused read's targets are freed, a kept read's move down to its
 * new place and leave their old slots empty, so that every target is owned by exactly one slot) and the caller starts both strands
 * over; on 0 the caller ends the run when rc is an error, for no read is to blame. */
static void validate_one(int64_t j, void *ctx) {
    const slice_t *sl = ctx;
    read_t *rd = &sl->reads[sl->who[j]];
    const sa_job_t *const jobs[2] = {sl->jobs[0] + j * sl->per_read, sl->jobs[1] ? sl->jobs[1] + j * sl->per_read : NULL};
    if (validate_read(sl->R, rd, jobs, sl->per_read) != 0)
        fprintf(stderr, "[signalMachine] ERROR: read %s skipped: %s\n", rd->label, rd->err);
}
static int drop_refused_reads(slice_t *sl, int rc) {
    if (sl->validated || rc == SA_OK || rc == SA_ENODEVICE || rc == SA_ENOMEM) return 0;
    sl->validated = 1;
    parallel_for(sl->n_ok, validate_one, sl);
    const int64_t N = sl->per_read;
    int64_t k = 0;
    for (int64_t j = 0; j < sl->n_ok; j++) {
        const int kept = !sl->reads[sl->who[j]].failed;
        for (int q = 0; q < n_strands(sl->R); q++)
            for (int64_t s = 0; s < N; s++) {
                const int64_t from = j * N + s, to = k * N + s;
                if (kept && to != from) sl->jobs[q][to] = sl->jobs[q][from];
                if (!sl->tgt[q] || (kept && to == from)) continue;
                if (kept) sl->tgt[q][to] = sl->tgt[q][from];
                else free(sl->tgt[q][from]);
                sl->tgt[q][from] = NULL;
            }
        if (kept) sl->who[k++] = sl->who[j];
    }
    const int dropped = k < sl->n_ok;
    sl->n_ok = k;
    return dropped;
}

/* a result of n_jobs jobs, filled as far as its batch got */
static void align_free_strand(slice_t *sl, int s, int64_t n_jobs) {
    strand_result_t *sr = &sl->sr[s];
    sa_batch_destroy(sr->batch);
    for (int64_t j = 0; j < n_jobs; j++) {
        if (sr->pairs) sa_free(sr->pairs[j]);
        if (sr->mea) sa_free(sr->mea[j]);
        if (sr->calls) sa_free(sr->calls[j]);
    }
    free(sr->pairs); free(sr->n_pairs); free(sr->mea); free(sr->n_mea); free(sr->all_n); free(sr->all_sum);
    free(sr->calls); free(sr->n_calls);
    free(sr->dev_reads); free(sr->dev_hist); free(sr->dev_ev_first);
    sa_free(sr->dev_sets); sa_free(sr->dev_events);
    free(sr->lab_reads); free(sr->cq_reads); free(sr->cq_hist);
    sa_free(sr->cq_calls); sa_free(sr->cq_gaps);
    sa_free(sr->lab_mea); sa_free(sr->lab_full); sa_free(sr->lab_bands); sa_free(sr->lab_samples);
    memset(sr, 0, sizeof(*sr));
}

/* kmer_id of the k letters at s (sorted alphabet, first letter most significant), -1 for a letter outside it */
static int32_t kmer_id_of(const strand_model_t *sm, const char *s) {
    int32_t id = 0;
    for (int i = 0; i < sm->k; i++) {
        const char *q = memchr(sm->alphabet, s[i], (size_t) sm->n_alpha);
        if (!q || !s[i]) return -1;
        id = id * sm->n_alpha + (int32_t) (q - sm->alphabet);
    }
    return id;
}

/* The rows of job j, expanded from the packed records the strand's batch holds in page-locked memory.  This runs job by job on
 * the rendering threads: the GPU stage does not expand every job's pairs into freshly allocated sa_pair_t arrays on the main
 * thread (523 MB per slice of 2048 long reads).  NULL, and the read marked failed, when the records cannot be had.
 * 8-byte records (-s 0 / 2 on reads without ambiguity letters -- half the bytes over PCIe where the pairs outweigh the kernels,
 * e.g. --sm3Hdp -D 0.01) hold x, y and the probability; the pair's k-mer is the reference's at x, its path 0. */
static sa_pair_t *expand_job_pairs(const run_t *R, read_t *rd, int s, const strand_result_t *sr, int64_t j) {
    const sa_pair8_t *pk8 = NULL;
    const sa_pair16_t *pk16 = NULL;
    int64_t n = 0;
    const int rc = sr->p8 ? sa_batch_pairs8(sr->batch, j, &pk8, &n) : sa_batch_pairs16(sr->batch, j, &pk16, &n);
    if (rc != SA_OK || n != sr->n_pairs[j]) {
        fprintf(stderr, "[signalMachine] ERROR: read %s: results of the batch are not readable\n", rd->label);
        rd->failed = 1;
        return NULL;
    }
    sa_pair_t *rows = xalloc(n, sizeof(sa_pair_t), 0);
    if (!sr->p8) {
        for (int64_t i = 0; i < n; i++) rows[i] = sa_pair16_unpack(pk16[i]);
        return rows;
    }
    int bad_kmer = 0;
    for (int64_t i = 0; i < n; i++) {
        sa_pair_t *q = &rows[i];
        sa_pair8_unpack(pk8[i], &q->prob_e7, &q->x, &q->y);
        q->path = 0;
        q->kmer_id = kmer_id_of(&R->sm[s], rd->st[s].target + q->x);
        bad_kmer |= q->kmer_id < 0;
    }
    if (bad_kmer) {   /* (cannot happen: the planner refuses a reference with a letter outside the model's alphabet) */
        fprintf(stderr, "[signalMachine] ERROR: read %s: a pair names a k-mer outside the model's alphabet\n", rd->label);
        rd->failed = 1;
        free(rows);
        return NULL;
    }
    return rows;
}

static void output_one(int64_t j, void *ctx) {
    slice_t *sl = ctx;
    const run_t *R = sl->R;
    read_t *rd = &sl->reads[sl->who[j]];
    if (R->out_fmt == 3 && rd->post_path2 == NULL) {
        fprintf(stderr, "[signalMachine] ERROR: read %s: 'both' output format needs a second output file\n", rd->label);
        rd->failed = 1;
        return;
    }
    sa_pair_t *mine[2] = {NULL, NULL};
    const sa_pair_t *pp[2] = {NULL, NULL};
    for (int s = 0; s < n_strands(R); s++) {
        const strand_result_t *sr = &sl->sr[s];
        pp[s] = sr->pairs[j];
        if (pp[s] != NULL || sr->batch == NULL) continue;
        pp[s] = mine[s] = expand_job_pairs(R, rd, s, sr, j);
        if (mine[s] == NULL) {
            free(mine[0]);
            return;
        }
    }
    for (int s = 0; s < n_strands(R); s++) {
        const strand_result_t *sr = &sl->sr[s];
        double tot = 0.0;
        int64_t n_all = sr->n_pairs[j];
        if (sr->all_n) {   /* (prob_e7 sums are integers below 2^53: the same double as the loop below gives) */
            n_all = sr->all_n[j];
            tot = (double) sr->all_sum[j];
        } else {
            for (int64_t i = 0; i < sr->n_pairs[j]; i++) tot += (double) pp[s][i].prob_e7;
        }
        sl->score[j][s] = 100.0 * tot / ((double) n_all * PROB_1); /* scoreByPosteriorProbabilityIgnoringGaps :407-412 */
    }
    const int tmpl_amb = sl->tmpl_amb && has_ambiguous_rows(R->ambig, rd->st[0].target, R->sm[0].k, pp[0], sl->sr[0].n_pairs[j]);
    if (sl->tmpl_amb) sl->tmpl_amb[j] = (unsigned char) tmpl_amb;
    for (int s = 0; s < n_strands(R) && rd->post_path != NULL; s++) {
        const strand_result_t *sr = &sl->sr[s];
        const out_ctx_t o = out_ctx_for(R, rd, s, pp[s], sr->n_pairs[j], sl->score[j][s]);
        output_alignment(R->out_fmt, rd->post_path, rd->post_path2, &o);
        if (R->mea) write_mea(rd->post_path, &o, sr->mea[j], sr->n_mea[j]);
        if (R->site_calls) write_calls(rd->post_path, rd, s, tmpl_amb, sr->calls[j], sr->n_calls[j], R->sm[s].k);
    }
    free(mine[0]); free(mine[1]);
}

static int cmp_str(const void *a, const void *b) { return strcmp(*(const char *const *) a, *(const char *const *) b); }

/* appending from several threads is only safe when no two reads share an output file */
static int outputs_distinct(const read_t *reads, const int64_t *who, int64_t n) {
    const char **v = malloc(sizeof(char *) * (size_t) (2 * n + 1));
    int64_t m = 0;
    for (int64_t j = 0; j < n; j++) {
        if (reads[who[j]].post_path) v[m++] = reads[who[j]].post_path;
        if (reads[who[j]].post_path2) v[m++] = reads[who[j]].post_path2;
    }
    qsort(v, (size_t) m, sizeof(char *), cmp_str);
    int ok = 1;
    for (int64_t i = 1; i < m && ok; i++) ok = strcmp(v[i], v[i - 1]) != 0;
    free(v);
    return ok;
}

/* One strand's batch of a slice, of all its jobs.  jobs[i] belongs to reads[who[i / per_read]] (per_read > 1: --snp-step's substituted copies).
 * --emission twoDist: a single read brings its own model; the reads of a manifest share the strand's two-distribution model and
 * each job gets the scale_sd / var_sd its read's parameter estimation left (emissions_signal_scaleNoise, applied inside the batch:
 * SA_FLAG_TWO_DIST_ALL_KERNELS, whatever kernel family a read's regions take). */
static int create_strand_batch(sa_batch_t **b, const slice_t *sl, int strand, unsigned flags) {
    const sa_job_t *jobs = sl->jobs[strand];
    const int64_t per_read = sl->per_read, n_jobs = sl->n_ok * per_read;
    const run_t *R = sl->R;
    const strand_model_t *sm = &R->sm[strand];
    if (!R->two_dist) return sa_batch_create(b, sm->model, &R->p, jobs, n_jobs, R->ambig, R->device, flags);
    if (!R->batch_mode) return sa_batch_create(b, sl->reads[sl->who[0]].model[strand], &R->p, jobs, n_jobs, R->ambig, R->device, flags);
    sa_noise_scale_t *nz = xalloc(n_jobs, sizeof(sa_noise_scale_t), 0);
    for (int64_t i = 0; i < n_jobs; i++) {
        const sa_strand_params_t *pp = np_params(sl->reads[sl->who[i / per_read]].np, strand);
        nz[i].scale_sd = pp->scale_sd;
        nz[i].var_sd = pp->var_sd;
    }
    const int rc = sa_batch_create_noise_scaled(b, sm->model_two, &R->p, jobs, nz, n_jobs, R->ambig, R->device,
                                                flags | SA_FLAG_TWO_DIST_ALL_KERNELS);
    free(nz);
    return rc;
}

/* Expectations mode (-t / -c, impl/signalMachine.c:772-848): sa_expect_batch per strand, the .expectations file of every read */
static int64_t run_slice_expect(run_t *R, read_t *reads, int64_t n_reads) {
    slice_t sl;
    slice_open(&sl, R, reads, n_reads);
    const int64_t n_ok = sl.n_ok;
    slice_build_jobs(&sl);
    if (n_ok > 0) fprintf(stderr, "Starting expectations routine\n");
    for (int s = 0; s < n_strands(R) && n_ok > 0; s++) {
        fprintf(stderr, "signalAlign - getting expectations for %s\n", strand_name(s));
        double *trans = xalloc(9 * n_ok, sizeof(double), 0), *lik = xalloc(n_ok, sizeof(double), 1);
        for (int64_t j = 0; j < 9 * n_ok; j++) trans[j] = 0.001; /* transitionsPseudocount, :785 */
        sa_assignment_t **as = xalloc(n_ok, sizeof(*as), 1);
        int64_t *n_as = xalloc(n_ok, sizeof(int64_t), 1);
        int rc = sa_expect_batch(R->sm[s].model, &R->p, sl.jobs[s], n_ok, R->ambig, R->device, 0, trans, lik, as, n_as);
        if (rc != SA_OK) die("signalMachine: expectations failed: %s", sa_strerror(rc));
        for (int64_t j = 0; j < n_ok; j++) {
            read_t *rd = &reads[sl.who[j]];
            if (R->hdp)
                fprintf(stderr, s == 0 ? "signalAlign - got %" PRId64 " template HDP assignments\n"
                                       : "signalAlign - got %" PRId64 "complement HDP assignments\n", n_as[j]);
            if (rd->expect[s] != NULL) {
                fprintf(stderr, "signalAlign - writing expectations to file: %s\n", rd->expect[s]);
                write_expectations(rd->expect[s], &R->sm[s], np_params(rd->np, s), R->hdp, R->p.threshold, trans + 9 * j, lik[j],
                                   &rd->jobs[s], as[j], n_as[j]);
            }
            sa_free(as[j]);
        }
        free(trans); free(lik); free(as); free(n_as);
    }
    for (int64_t j = 0; j < n_ok; j++) report_read(R, &reads[sl.who[j]], NULL, NULL);
    return slice_close(&sl);
}

/* ---- alignment mode: the pair-HMM on the GPU, one batch per strand model with all reads side by side, then the outputs ----
 * Creates, runs and harvests the batch of strand s into sl->sr[s]; whatever it returns, the result is one align_free_strand can take.
 * -s 1 prints only the rows whose reference k-mer holds an X: the others stay on the device (SA_FLAG_VC_ROWS), the run's pair
 * count and score come from the totals the device kept.
 * --site-calls / --site-calls-aggregate: every batch records its sites (SA_FLAG_SITE_CALLS) and keeps every row (the calls are
 * made of the rows SA_FLAG_VC_ROWS would drop; -s 1 then filters on the host, write_vc).
 * -s 0 / -s 2 without --mea: 8-byte result records where the batch allows them (one path per cell: no ambiguity letter in any
 * read's reference; fewer than 2^20 positions and events per read) -- the planner says SA_EUNSUPPORTED otherwise and the strand's
 * batch is made again with 16-byte records.  SA_CLI_PAIRS16=1: always 16-byte records (the test's checker).
 * --mea, --guide-deviation, --signal-labels, --site-calls-accuracy-quality: the pairs are copied out while the batch still has them
 * on the device for the path step.
 * The run-wide outputs take the batch while its records are in HBM (outputs_add_batch); with --mea the batch ends there.
 * Otherwise the batch stays alive for the rendering, which expands its packed records job by job. */
static int align_run_strand(slice_t *sl, int s) {
    const run_t *R = sl->R;
    strand_result_t *sr = &sl->sr[s];
    const int64_t n = sl->n_ok;
    const int want_calls = R->site_calls || R->want_agg;
    const int want_mea = R->mea || R->dev_path != NULL || R->lab_dir != NULL || R->cq_path != NULL;
    unsigned flags = want_calls ? SA_FLAG_SITE_CALLS : 0u, p8 = 0u;
    if (!want_mea && !want_calls) {
        if (R->out_fmt == 1 && !R->want_train && !getenv("SA_CLI_VC_ON_HOST")) flags |= SA_FLAG_VC_ROWS;
        if ((R->out_fmt == 0 || R->out_fmt == 2) && !getenv("SA_CLI_PAIRS16") && !R->prof_path) p8 = SA_FLAG_PAIRS8;   /* (the profile reads path k-mers) */
    }
    sr->pairs = xalloc(n, sizeof(sa_pair_t *), 1);
    sr->n_pairs = xalloc(n, sizeof(int64_t), 1);
    if (want_calls) {
        sr->calls = xalloc(n, sizeof(sa_site_call_t *), 1);
        sr->n_calls = xalloc(n, sizeof(int64_t), 1);
    }
    if (want_mea) {
        sr->mea = xalloc(n, sizeof(sa_mea_pair_t *), 1);
        sr->n_mea = xalloc(n, sizeof(int64_t), 1);
    }
    sa_batch_t *b = NULL;
    int rc = create_strand_batch(&b, sl, s, flags | p8);
    sr->p8 = rc == SA_OK && p8 != 0;
    if (rc == SA_EUNSUPPORTED && p8) rc = create_strand_batch(&b, sl, s, flags);
    if (rc == SA_OK) rc = sa_batch_run(b);
    if (rc == SA_OK && want_calls) rc = sa_batch_site_calls(b, 0, sr->calls, sr->n_calls, NULL);
    for (int64_t j = 0; j < n && rc == SA_OK && want_mea; j++) {
        sa_batch_n_pairs(b, j, &sr->n_pairs[j]);
        sr->pairs[j] = xalloc(sr->n_pairs[j], sizeof(sa_pair_t), 0);
        rc = sa_batch_pairs(b, j, sr->pairs[j], sr->n_pairs[j]);
    }
    if (rc == SA_OK && want_mea) rc = sa_batch_mea(b, 0, sr->mea, sr->n_mea, NULL, NULL, NULL);
    if (rc == SA_OK) rc = outputs_add_batch(sl, s, b);
    if (want_mea) {
        sa_batch_destroy(b);
        return rc;
    }
    for (int64_t j = 0; j < n && rc == SA_OK; j++) rc = sa_batch_n_pairs(b, j, &sr->n_pairs[j]);
    if ((flags & SA_FLAG_VC_ROWS) && rc == SA_OK) {
        sr->all_n = xalloc(n, sizeof(int64_t), 1);
        sr->all_sum = xalloc(n, sizeof(int64_t), 1);
        for (int64_t j = 0; j < n && rc == SA_OK; j++) rc = sa_batch_all_pairs_summary(b, j, &sr->all_n[j], &sr->all_sum[j]);
    }
    /* only the packed pairs (pinned host memory) are read from here on: the batch's HBM goes back now, so that the
     * complement strand's batch plans into the whole card */
    if (rc == SA_OK) rc = sa_batch_release_device(b);
    if (rc == SA_OK) sr->batch = b;
    else sa_batch_destroy(b);
    return rc;
}

/* rendering of an alignment slice (one file per read, in parallel), summary lines in read order */
static void align_render(slice_t *sl) {
    const run_t *R = sl->R;
    sl->score = xalloc(sl->n_ok, sizeof(*sl->score), 1);
    sl->tmpl_amb = (R->two_d && sl->sr[1].calls) ? xalloc(sl->n_ok, 1, 1) : NULL;
    if (outputs_distinct(sl->reads, sl->who, sl->n_ok)) parallel_for(sl->n_ok, output_one, sl);
    else for (int64_t j = 0; j < sl->n_ok; j++) output_one(j, sl);
    for (int64_t j = 0; j < sl->n_ok; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        if (rd->failed) continue;
        int64_t n_all[2] = {0, 0};
        for (int s = 0; s < n_strands(R); s++) n_all[s] = sl->sr[s].all_n ? sl->sr[s].all_n[j] : sl->sr[s].n_pairs[j];
        outputs_add_read(sl, j);
        report_read(R, rd, n_all, sl->score[j]);
    }
    outputs_rendered(sl);
    free(sl->tmpl_amb);
    free(sl->score);
    for (int s = 0; s < 2; s++) align_free_strand(sl, s, sl->n_ok);
}

/* ---- --snp-step N --snp-dir DIR: single-nucleotide probabilities (singleNucleotideProbabilities.py:551-723) ----
 * Every read strand becomes N jobs in one batch (slice_build_jobs).  sa_batch_position_calls folds the rows of every X position on
 * the device (CallMethylation.call_methyls); the N step files of a read are merged into DIR/<label>.tsv
 * (discover_single_nucleotide_probabilities).  fast5_input names the .npRead: the one deliberate difference.
 * --snp-marginals: every batch is also added to one over-reads table on the device, written at the end of the run; --snp-sites: the
 * same with one copy per read, X at the listed sites only (1-D runs). */
static void snp_free_strand(slice_t *sl, int q, int64_t n_jobs) {
    snp_result_t *r = &sl->snp[q];
    for (int64_t i = 0; i < n_jobs && r->calls; i++) sa_free(r->calls[i]);
    free(r->calls); free(r->n_calls); free(r->x_min); free(r->x_max); free(r->n_pairs); free(r->sum_e7);
    memset(r, 0, sizeof(*r));
}

/* creates, runs and harvests the batch of strand q into sl->snp[q] */
static int snp_run_strand(slice_t *sl, int q) {
    snp_result_t *r = &sl->snp[q];
    const int64_t nj = sl->n_ok * sl->per_read;
    r->calls = xalloc(nj, sizeof(sa_position_call_t *), 1);
    r->n_calls = xalloc(nj, sizeof(int64_t), 1);
    r->x_min = xalloc(nj, sizeof(int32_t), 1);
    r->x_max = xalloc(nj, sizeof(int32_t), 1);
    r->n_pairs = xalloc(nj, sizeof(int64_t), 1);
    r->sum_e7 = xalloc(nj, sizeof(int64_t), 1);
    sa_batch_t *b = NULL;
    int rc = create_strand_batch(&b, sl, q, SA_FLAG_POSITION_CALLS);
    if (rc == SA_OK) rc = sa_batch_run(b);
    if (rc == SA_OK && sl->R->snp_dir) rc = sa_batch_position_calls(b, 0, r->calls, r->n_calls, r->x_min, r->x_max, NULL);
    if (rc == SA_OK) rc = outputs_add_batch(sl, q, b);
    for (int64_t i = 0; i < nj && rc == SA_OK; i++) rc = sa_batch_all_pairs_summary(b, i, &r->n_pairs[i], &r->sum_e7[i]);
    sa_batch_destroy(b);
    return rc;
}

static void snp_output_one(int64_t j, void *ctx) {
    slice_t *sl = ctx;
    const run_t *R = sl->R;
    const int64_t N = sl->per_read;
    read_t *rd = &sl->reads[sl->who[j]];
    int64_t cap = 0;
    for (int64_t s = 0; s < N; s++)
        for (int q = 0; q < n_strands(R); q++) cap += sl->snp[q].n_calls[j * N + s];
    sa_snp_site_t *sites = xalloc(cap, sizeof(sa_snp_site_t), 0);
    int64_t n = 0;
    for (int64_t s = 0; s < N; s++) {   /* one step file after the other */
        const int64_t js = j * N + s;
        /* the window of call_methyls (:160-169) over the reference_index of every row of the step's file, both strands */
        int64_t lo_ref = INT64_MAX, hi_ref = INT64_MIN;
        for (int q = 0; q < n_strands(R); q++) {
            if (sl->snp[q].x_min[js] < 0) continue;
            const int k = R->sm[q].k;
            const int64_t len = (int64_t) strlen(rd->st[q].target), off = rd->st[q].r_shift;
            const int64_t a = adjust_ref(sl->snp[q].x_min[js], off, len - k, len, q == 0, rd->forward);
            const int64_t b = adjust_ref(sl->snp[q].x_max[js], off, len - k, len, q == 0, rd->forward);
            lo_ref = a < lo_ref ? a : lo_ref; lo_ref = b < lo_ref ? b : lo_ref;
            hi_ref = a > hi_ref ? a : hi_ref; hi_ref = b > hi_ref ? b : hi_ref;
        }
        if (lo_ref > hi_ref) continue;   /* no row at all: the reference's step file cannot be parsed and is missing */
        int64_t w_lo = 0, w_hi = 0;
        sa_snp_site_window(lo_ref, hi_ref, N, &w_lo, &w_hi);
        for (int q = 0; q < n_strands(R); q++) {   /* template sites, then complement sites, each ascending */
            const sa_position_call_t *pc = sl->snp[q].calls[js];
            const int64_t m = sl->snp[q].n_calls[js];
            const int same = snp_contig_pos_is_forward(rd, q);
            for (int64_t i0 = 0; i0 < m; i0++) {
                const sa_position_call_t *p = &pc[same ? i0 : m - 1 - i0];
                const int64_t pos = snp_contig_pos(rd, q, p->p);
                if (pos < w_lo || pos >= w_hi) continue;
                sa_snp_site_t *o = &sites[n++];
                o->pos = pos;
                o->strand = q;
                o->pad = 0;
                for (int l = 0; l < 4; l++) {
                    o->p[l] = 0.0;
                    for (int e = 0; e < p->n_letters; e++)
                        if (p->letters[e] == "ACGT"[l]) o->p[l] = p->prob[e];
                }
            }
        }
    }
    const char *np_name = strrchr(rd->npread_path, '/') ? strrchr(rd->npread_path, '/') + 1 : rd->npread_path;
    char *path = malloc(strlen(R->snp_dir) + strlen(rd->label) + 8);
    sprintf(path, "%s/%s.tsv", R->snp_dir, rd->label);
    if (sa_snp_write_read(path, np_name, rd->label, rd->pA->contig1, !rd->forward, sites, n) != SA_OK)
        die("signalMachine: cannot write %s", path);
    free(path);
    free(sites);
}

/* the per-read files, then the summary lines of the N -s 0 runs of every read, step after step */
static void snp_render(slice_t *sl) {
    const run_t *R = sl->R;
    const int64_t N = sl->per_read;
    if (R->snp_dir) parallel_for(sl->n_ok, snp_output_one, sl);
    for (int64_t j = 0; j < sl->n_ok; j++)
        for (int64_t s = 0; s < N; s++) {
            const int64_t js = j * N + s;
            int64_t n[2] = {0, 0};
            double score[2] = {0.0, 0.0};
            for (int q = 0; q < n_strands(R); q++) {
                n[q] = sl->snp[q].n_pairs[js];
                score[q] = 100.0 * (double) sl->snp[q].sum_e7[js] / ((double) n[q] * PROB_1);
            }
            report_read(R, &sl->reads[sl->who[j]], n, score);
        }
    for (int q = 0; q < n_strands(R); q++) snp_free_strand(sl, q, sl->n_ok * N);
}

/* ---- one slice: its GPU stage and its outputs.  A mode is what differs between the alignment and the SNP runs. ---- */
typedef struct {
    int (*run_strand)(slice_t *sl, int s);                       /* creates, runs and harvests strand s's batch */
    void (*free_strand)(slice_t *sl, int s, int64_t n_jobs);     /* what that left, of n_jobs jobs, filled as far as the batch got */
    void (*render)(slice_t *sl);                                 /* files and summary lines; frees the results */
} slice_mode_t;
static const slice_mode_t MODE_ALIGN = {align_run_strand, align_free_strand, align_render};
static const slice_mode_t MODE_SNP = {snp_run_strand, snp_free_strand, snp_render};

/* (the host side of the slice's reads has run: slice_prepare, a slice ahead of this function) */
static int64_t run_slice(run_t *R, read_t *reads, int64_t n_reads) {
    if (R->expect_mode) return run_slice_expect(R, reads, n_reads);
    const slice_mode_t *mode = snp_mode(R) ? &MODE_SNP : &MODE_ALIGN;
    slice_t slice, *sl = &slice;
    slice_open(sl, R, reads, n_reads);
    const double ts1 = now_s();
    slice_build_jobs(sl);
    /* the run-wide outputs are checkpointed here, so that starting over (a read the planner refuses) takes the slice's rows back */
    outputs_checkpoint(R, 0);
    for (int s = 0; s < n_strands(R) && sl->n_ok > 0; s++) {
        fprintf(stderr, "signalAlign - starting %s alignment\n", strand_name(s));
        const int64_t n_jobs = sl->n_ok * sl->per_read;
        const int rc = mode->run_strand(sl, s);
        if (drop_refused_reads(sl, rc)) {
            outputs_checkpoint(R, 1);
            for (int q = 0; q <= s; q++) mode->free_strand(sl, q, n_jobs);
            s = -1;   /* both strands again, without the offenders */
            continue;
        }
        if (rc != SA_OK) die("signalMachine: alignment failed: %s", sa_strerror(rc));
    }
    const double ts2 = now_s();
    g_t_gpu += ts2 - ts1;
    mode->render(sl);
    t_add(&g_t_render, now_s() - ts2);
    return slice_close(sl);
}
