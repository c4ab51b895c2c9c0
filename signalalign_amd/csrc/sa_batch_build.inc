// sa_batch_build.inc -- how a batch comes to be: its launch lists, the upload of its model tables and plan, its working storage, the
// public create calls and sa_dplan_compare.  Included by sa_hip.hip behind sa_dplan.inc and sa_batch_destroy.

// The upload ring a batch's creation goes through: the second one for a deferred batch only (with several batches in flight and
// creation in one piece the second upload stream measured 1.5-3 ms per step slower than one).
static SaUploader *batch_uploader(const sa_batch *b) { return b->c_deferred ? &g_uploader_tail : &g_uploader; }

// Launch lists: regions per forward-storage pass, traceback segments per result group (needs the plan, no device memory)
static int batch_build_lists(sa_batch *b) {
    sa_plan_t *pl = b->plan;
    const unsigned flags = b->flags;
    const bool host_finalize = (flags & SA_FLAG_EXACT) || b->expect;
    int want = 1;
    const char *envg = getenv("SA_GROUPS");  // test hook
    if (envg && atoi(envg) > 0) want = atoi(envg);
    else if (!host_finalize) want = pl->n_chunks == 1 ? 8 : (pl->n_chunks < 4 ? 4 : 2);
    // A caller that keeps batches in flight (sa_batch_start: another batch of this process is running while this one is
    // created) already overlaps a batch's result copy with its neighbours' kernels; what it wants is few, large launches:
    // 2000 x 5000-event reads, three in flight, step time with 1 / 2 / 3 / 8 groups: 13.9 / 13.1 / 12.9 / 14.9 ms.
    if (!(envg && atoi(envg) > 0) && !host_finalize && g_batches_started.load() > 0 && !(flags & SA_FLAG_DEVICE_TO_ITSELF) && want > 3) want = 3;
    b->ids_flat.clear(); b->chunks.clear(); b->groups.clear();
    // One-path ring-kernel regions go to the strip kernels (sa_strip.inc): Gaussian emissions, default arithmetic,
    // device-side finalisation, reference windows of fewer than 64 * STRIP_NS_MAX positions.  SA_STRIP=0: ring kernels.
    b->strip_on = !host_finalize && !(getenv("SA_STRIP") && atoi(getenv("SA_STRIP")) == 0);   // (HDP regions too: they read the emission plane)
    long long strip_max_n = 0, strip_max_seg = 0, strip_fwd_slots = 0, strip_bwd_slots = 0;
    // one list per launch class, longest first (the tail of a launch is then made of short waves), appended to ids_flat in class order
    auto append = [&](std::vector<int> (&lists)[LC_N], sa_ids *out, auto longer) {
        for (int c = 0; c < LC_N; c++) {
            std::stable_sort(lists[c].begin(), lists[c].end(), longer);
            out[c] = sa_ids{(long long) b->ids_flat.size(), (int) lists[c].size()};
            b->ids_flat.insert(b->ids_flat.end(), lists[c].begin(), lists[c].end());
        }
    };
    long long r = 0;
    for (int c = 0; c < pl->n_chunks; c++) {
        long long ra = r;
        while (r < pl->n_regions && pl->regions[r].chunk == c) r++;
        long long rb = r;
        sa_launch_chunk C;
        std::vector<int> ids[LC_N];
        double work = 0;
        for (long long q = ra; q < rb; q++) {
            const sa_region_t &Rq = pl->regions[q];
            const int lc = launch_class(Rq, b->strip_on);
            ids[lc].push_back((int) q);
            if (lc == LC_STRIP) strip_max_n = Rq.N > strip_max_n ? Rq.N : strip_max_n;
            work += (double) Rq.N;
        }
        append(ids, C.ids, [&](int a, int d) { return pl->regions[a].N > pl->regions[d].N; });
        strip_fwd_slots = std::max(strip_fwd_slots, (long long) C.ids[LC_STRIP].n);
        long long chunk_bwd_slots = 0;
        C.g0 = (int) b->groups.size();
        // a group should still be a sizeable launch: at least 2048 segments each (measured optimum 6-8 groups
        // for 18000 segments; 16 and more lose to launch gaps)
        long long nseg_chunk = 0, nseg_wide = 0;
        for (long long q = ra; q < rb; q++) {
            nseg_chunk += pl->regions[q].n_seg;
            if ((pl->regions[q].kind == SA_KIND_FAST && pl->regions[q].slots >= 2) ||
                (pl->regions[q].kind == SA_KIND_RING && pl->regions[q].max_rowpaths > 64))
                nseg_wide += pl->regions[q].n_seg;
        }
        // segments of wide-band regions live three to four times longer than those of dense anchors (4 ms against
        // 1.2 ms), and so do the tails of their launches: fewer, larger groups.  2000 reads with realistic anchors,
        // 17 300 segments, step time with 1 / 2 / 3 / 4 / 6 / 8 groups: 70.2 / 67.8 / 69.3 / 73.1 / 80.2 / 87 ms
        // (strip-kernel segments: 1 / 2 / 3 / 4 groups give 39.5 / 38.3 / 37.5 / 42.9 ms per step of fresh reads)
        const long long min_per_group = (2 * nseg_wide > nseg_chunk) ? (b->strip_on ? 5500 : 8192) : 2048;
        int ng = want;
        if (!(envg && atoi(envg) > 0))
            while (ng > 1 && nseg_chunk / ng < min_per_group) ng--;
        long long q = ra;
        double acc = 0;
        for (int g = 0; g < ng && q < rb; g++) {
            long long qa = q;
            double target = work * (double) (g + 1) / (double) ng;
            while (q < rb && (g == ng - 1 || acc < target)) { acc += (double) pl->regions[q].N; q++; }
            if (q == qa) continue;
            // a read's regions stay in one group so that its pairs are contiguous in the output
            while (q < rb && pl->regions[q].job == pl->regions[q - 1].job) { acc += (double) pl->regions[q].N; q++; }
            sa_launch_group G;
            G.seg0 = G.seg1 = G.ck0 = G.ck1 = 0;
            std::vector<int> sids[LC_N];
            bool any = false;
            for (long long t = qa; t < q; t++) {
                const sa_region_t *R = &pl->regions[t];
                const int lc = launch_class(*R, b->strip_on);
                for (long long sg = R->seg_off; sg < R->seg_off + R->n_seg; sg++) {
                    sids[lc].push_back((int) sg);
                    const sa_seg_t *S = &pl->segs[sg];
                    if (lc == LC_STRIP) strip_max_seg = std::max(strip_max_seg, (long long) (S->start - S->to));
                    if (!any) { G.seg0 = sg; G.ck0 = S->ck_base; any = true; }
                    G.seg1 = sg + 1;
                    G.ck1 = S->ck_base + S->n_ck;
                }
            }
            if (!any) continue;
            append(sids, G.ids, [&](int a, int d) { return pl->segs[a].start - pl->segs[a].to > pl->segs[d].start - pl->segs[d].to; });
            G.seam_first = (unsigned) chunk_bwd_slots;   // (rebased behind the forward slots below)
            chunk_bwd_slots += G.ids[LC_STRIP].n;
            b->groups.push_back(G);
        }
        strip_bwd_slots = chunk_bwd_slots > strip_bwd_slots ? chunk_bwd_slots : strip_bwd_slots;
        C.g1 = (int) b->groups.size();
        b->chunks.push_back(C);
    }
    b->lw_strip_max_n = strip_max_n; b->lw_strip_max_seg = strip_max_seg;
    b->lw_strip_fwd_slots = strip_fwd_slots; b->lw_strip_bwd_slots = strip_bwd_slots;
    return SA_OK;
}

// The model tables a batch's kernels read (tab6, the noise columns and every event's noise, the register kernels' `two` block with its
// per-job noise scaling, the HDP's slots, grid, spline tables and hot row), through this thread's uploader.
static int upload_model_tables(sa_batch *b, const sa_plan_t *pl) {
    const sa_model_t *m = b->c_m;
    const sa_job_t *jobs = b->c_jobs;
    const int64_t n_jobs = b->c_n;
    std::vector<double> tab6((size_t) m->n_kmers * 6);
    for (long long i = 0; i < m->n_kmers; i++) {
        double mu = m->table5[5 * i], sd = m->table5[5 * i + 1];
        double sdy = sd * SA_GAPY_SD_MULT;  // stateMachine3_loadFromFile multiplies the loaded sd (impl/stateMachine.c:1530-1532)
        tab6[6 * i + 0] = mu;
        tab6[6 * i + 1] = sd == 0.0 ? 1.0 : sd;
        tab6[6 * i + 2] = sd == 0.0 ? -INFINITY : (-0.91893853320467267 - log(sd));
        tab6[6 * i + 3] = sdy == 0.0 ? 1.0 : sdy;
        tab6[6 * i + 4] = sdy == 0.0 ? -INFINITY : (-0.91893853320467267 - log(sdy));
        tab6[6 * i + 5] = 0.0;
    }
    TRY(upload(&b->d_tab6, tab6.data(), (long long) tab6.size()));
    if (m->emission != 0) {   // noise columns of the table, and every event's noise with its logarithm (C library's log)
        if (m->hdp) return SA_EUNSUPPORTED;
        std::vector<double> nz((size_t) m->n_kmers * 3);
        for (long long i = 0; i < m->n_kmers; i++) {
            nz[3 * i] = m->table5[5 * i + 2];
            nz[3 * i + 1] = m->table5[5 * i + 4];
            nz[3 * i + 2] = log(m->table5[5 * i + 4]);
        }
        TRY(upload(&b->d_noise3, nz.data(), (long long) nz.size()));
        std::vector<double> evn((size_t) (2 * (pl->n_ev + 8)), 1.0);
        for (int64_t j = 0; j < n_jobs; j++) {
            const sa_job_t *jb = &jobs[j];
            if (jb->n_events > 0 && jb->event_stride < 2) return SA_EINVAL;   // the noise is the record's second value
            const sa_jobinfo_t *J = &pl->jobs[j];
            for (int64_t i = 0; i < J->n_events; i++) {
                double n = jb->events[i * jb->event_stride + 1];
                if (n == 0 && m->emission == SA_EMISSION_TWO_DIST) n = 0.000000001;   // (impl/stateMachine.c:619-621; :659-700 has no such guard)
                evn[(size_t) (2 * (J->ev_off + i))] = n;
                evn[(size_t) (2 * (J->ev_off + i) + 1)] = log(n);
            }
        }
        TRY(upload(&b->d_evn, evn.data(), (long long) evn.size()));
        if (!(b->flags & SA_FLAG_EXACT)) {
            // the register kernels' form of the same numbers (FastT.two_xn_off): per event {n, 1 / n, 1.5 log n, 0}, then per
            // path-space index {(log lambda - log 2 pi) / 2, 1 / noise mean, lambda / 2, 0} of the position's k-mer (zeros for the
            // NULL entry, whose Gaussian part is -inf already)
            const long long ne = pl->n_ev + 8, np_ = at_least_1(pl->n_pid);
            std::vector<double> two((size_t) (4 * (ne + np_)), 0.0);
            for (long long y = 0; y < ne; y++) {
                const double n = evn[(size_t) (2 * y)];
                two[(size_t) (4 * y)] = n; two[(size_t) (4 * y + 1)] = 1.0 / n; two[(size_t) (4 * y + 2)] = 1.5 * evn[(size_t) (2 * y + 1)];
            }
            for (long long i = 0; i < pl->n_pid && b->c_noise.empty(); i++) {
                const int id = pl->pid[i];
                if (id < 0) continue;
                double *q = &two[(size_t) (4 * (ne + i))];
                q[0] = 0.5 * (nz[(size_t) (3 * id + 2)] - 1.8378770664093453);
                q[1] = 1.0 / nz[(size_t) (3 * id)];
                q[2] = 0.5 * nz[(size_t) (3 * id + 1)];
            }
            // sa_batch_create_noise_scaled: the same from the job's own table, emissions_signal_scaleNoise of the model's
            // (impl/stateMachine.c:721-741: noise_mean * scale_sd, noise_lambda * var_sd, each product a double before anything is
            // derived from it).  A region's path-space indices are its own (pid_off, poff), and a region knows its job.
            for (long long r = 0; r < pl->n_regions && !b->c_noise.empty(); r++) {
                const sa_region_t *R = &pl->regions[r];
                const sa_noise_scale_t ns = b->c_noise[(size_t) R->job];
                const long long n_paths = pl->poff[R->poff_off + R->lX + 1];
                for (long long i = R->pid_off; i < R->pid_off + n_paths; i++) {
                    const int id = pl->pid[i];
                    if (id < 0) continue;
                    const double mean = nz[(size_t) (3 * id)] * ns.scale_sd, lambda = nz[(size_t) (3 * id + 1)] * ns.var_sd;
                    double *q = &two[(size_t) (4 * (ne + i))];
                    q[0] = 0.5 * (log(lambda) - 1.8378770664093453);
                    q[1] = 1.0 / mean;
                    q[2] = 0.5 * lambda;
                }
            }
            b->two_xn_off = ne;
            TRY(upload(&b->d_two, two.data(), (long long) two.size()));
        }
    }
    if (m->hdp) {
        const sa_hdp_t *h = m->hdp;
        std::vector<int> slot((size_t) m->n_kmers);
        for (long long i = 0; i < m->n_kmers; i++) {
            long long r = h->resolved[i];
            slot[i] = (r >= 0 && h->slot[r] >= 0) ? (int) h->slot[r] : -1;
        }
        {   // the row most k-mers resolve to (k_emit_hdp stages it in LDS): worth it from a quarter of the k-mers on
            std::vector<long long> cnt((size_t) at_least_1(h->n_slots), 0);
            for (long long i = 0; i < m->n_kmers; i++)
                if (slot[(size_t) i] >= 0) cnt[(size_t) slot[(size_t) i]]++;
            long long best = 0;
            for (long long s_ = 1; s_ < h->n_slots; s_++)
                if (cnt[(size_t) s_] > cnt[(size_t) best]) best = s_;
            b->hdp_hot = (h->n_slots > 0 && 4 * cnt[(size_t) best] >= m->n_kmers) ? (unsigned) (best * h->grid_length * 16) : 0xffffffffu;
            if (getenv("SA_HDP_HOT") && atoi(getenv("SA_HDP_HOT")) == 0) b->hdp_hot = 0xffffffffu;   // test hook: the flavours without a hot row
        }
        TRY(upload(&b->d_hdp_slot, slot.data(), (long long) slot.size()));
        TRY(upload(&b->d_hdp_y, h->y, h->n_slots * h->grid_length));
        TRY(upload(&b->d_hdp_slope, h->slope, h->n_slots * h->grid_length));
        TRY(upload(&b->d_hdp_grid, h->grid, h->grid_length));
        std::vector<double> tab((size_t) (h->n_slots * h->grid_length * 2));
        for (long long i = 0; i < h->n_slots * h->grid_length; i++) {
            tab[2 * i] = h->y[i];
            tab[2 * i + 1] = h->slope[i];
        }
        TRY(upload(&b->d_hdp_tab, tab.data(), (long long) tab.size()));
        // the same spline as a cubic in the position inside interval i (k_emit_hdp, sa_fast.inc): c0 + c1 t + c2 t^2 + c3 t^3 with
        // the combinations formed in long double; the last entry of a row (no interval to its right) stays zero
        std::vector<double> coef((size_t) (h->n_slots * h->grid_length * 4), 0.0);
        const long double dxl = (long double) h->grid[1] - (long double) h->grid[0];
        for (long long s = 0; s < h->n_slots; s++)
            for (long long i = 0; i + 1 < h->grid_length; i++) {
                const long long k = s * h->grid_length + i;
                const long double y0 = h->y[k], y1 = h->y[k + 1], s0 = h->slope[k], s1 = h->slope[k + 1], dy = y1 - y0;
                coef[4 * k] = (double) y0;
                coef[4 * k + 1] = (double) (s0 * dxl);
                coef[4 * k + 2] = (double) (3.0L * dy - (2.0L * s0 + s1) * dxl);
                coef[4 * k + 3] = (double) ((s0 + s1) * dxl - 2.0L * dy);
            }
        TRY(upload(&b->d_hdp_coef, coef.data(), (long long) coef.size()));
    }
    return SA_OK;
}

// SA_FLAG_VC_ROWS: which reference positions the variant-caller output reports on (k_finalize)
static int upload_vc_rows(sa_batch *b, const sa_plan_t *pl) {
    const sa_job_t *jobs = b->c_jobs;
    const int64_t n_jobs = b->c_n;
    const int kk = b->c_m->k;
    b->h_vc_off.assign((size_t) n_jobs + 1, 0);
    for (int64_t j = 0; j < n_jobs; j++) b->h_vc_off[(size_t) j + 1] = b->h_vc_off[(size_t) j] + ((jobs[j].ref_len + 63) / 64 + 1) * 64;
    b->h_vc_bits.assign((size_t) (b->h_vc_off[(size_t) n_jobs] / 64 + 1), 0ull);
    for (int64_t j = 0; j < n_jobs; j++) {
        const char *ref = jobs[j].ref;
        const long long base = b->h_vc_off[(size_t) j];
        long long last_x = -1;   // the last 'X' at or in front of position i + k - 1
        for (long long i = 0; i < kk - 1 && i < jobs[j].ref_len; i++)
            if (ref[i] == 'X') last_x = i;
        for (long long i = 0; i + kk <= jobs[j].ref_len; i++) {
            if (ref[i + kk - 1] == 'X') last_x = i + kk - 1;
            if (last_x >= i) b->h_vc_bits[(size_t) ((base + i) >> 6)] |= 1ull << ((base + i) & 63);
        }
    }
    TRY(upload(&b->d_vc_bits, b->h_vc_bits.data(), (long long) b->h_vc_bits.size()));
    TRY(upload(&b->d_vc_off, b->h_vc_off.data(), (long long) b->h_vc_off.size()));
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &b->d_seg_all, sizeof(long long) * 2 * (size_t) at_least_1(pl->n_segs), b->device) != hipSuccess)
        return SA_ENOMEM;
    return SA_OK;
}

// First step of finishing a batch, everything that needs no working storage: the plan (from the device planner, or built on the host)
// and the launch lists.  sa_batch_prepare runs it ahead of time for a deferred batch, while the batch before it is on the device.
static int batch_prepare_body(sa_batch *b) {
    const sa_model_t *m = b->c_m;
    const sa_params_t *p = &b->c_p;
    const sa_job_t *jobs = b->c_jobs;
    const int64_t n_jobs = b->c_n;
    const char *const *ambig = b->c_ambig;
    unsigned flags = b->flags;   // (gains SA_FLAG_EXACT when a two-distribution batch is planned again below)
    const long long budget = b->c_budget;
    const int device = b->device;
    const bool trace_c = getenv("SA_TRACE") != nullptr;
    const double tc0 = b->c_t0;
    HIPCHK(hipSetDevice(device));
    SaUploader *const UPT = batch_uploader(b);
    UseUploader use_upt_(UPT);
    sa_plan_t *pl = nullptr;
    if (b->pending) {
        DPlanPending *P = b->pending;
        b->pending = nullptr;
        const int rcd = dplan_back(b, P);
        if (rcd < 0) return rcd;
        if (rcd == SA_OK) pl = b->plan;
    }
    if (!pl) {
        // pinning memory costs about 0.25 ms per MB: it pays for a process that streams batches (the blocks are reused), not
        // for the one or two batches of a command-line run, which stage their plan through the uploader's ring instead
        static std::atomic<int> batches_created(0);
        if (SaPool::enabled() && batches_created.fetch_add(1) >= 2) sa_plan_use_allocator(plan_pinned_alloc, plan_pinned_free);
        int rc = sa_plan_build(&pl, m, p, jobs, n_jobs, ambig, flags | SA_FLAG_DEVICE_XC_INTERNAL, budget);
        // (SA_FLAG_TWO_DIST_ALL_KERNELS: the ring and strip kernels have it too; what is left are the regions that a MeanOnly model
        // would send to the memory-resident kernels as well)
        const long long n_two_regions = pl ? pl->n_fast_regions + ((flags & SA_FLAG_TWO_DIST_ALL_KERNELS) ? pl->n_ring_regions : 0) : 0;
        if (rc == SA_OK && m->emission != 0 && !(flags & SA_FLAG_EXACT) && n_two_regions != pl->n_regions) {
            // the two-distribution emission off these kernels: the reference-ordered kernels for the whole batch -- which know
            // nothing of a noise scaling per job
            if (!b->c_noise.empty()) {
                sa_plan_free(pl);
                sa_plan_use_allocator(nullptr, nullptr);
                return SA_EUNSUPPORTED;
            }
            sa_plan_free(pl);
            pl = nullptr;
            b->flags |= SA_FLAG_EXACT;
            flags = b->flags;
            rc = sa_plan_build(&pl, m, p, jobs, n_jobs, ambig, flags | SA_FLAG_DEVICE_XC_INTERNAL, budget);
        }
        sa_plan_use_allocator(nullptr, nullptr);
        if (rc) return rc;
        if (trace_c) fprintf(stderr, "[trace] create: planned at %.1f ms\n", now_ms() - tc0);
        b->plan = pl;
    }
    if (trace_c) fprintf(stderr, "[trace] create: planned (%s) at %.1f ms\n", b->dev_planned ? "device" : "host", now_ms() - tc0);

    b->expect = (flags & SA_FLAG_EXPECT_INTERNAL) != 0;
    b->plan_hdp = m->hdp != nullptr;
    b->p8 = (flags & SA_FLAG_PAIRS8) != 0 && !b->expect;
    if (b->p8) {   // 20 bits per coordinate, no path index, no k-mer: only what one path per cell and short matrices allow
        if (flags & SA_FLAG_VC_ROWS) return SA_EINVAL;
        for (int64_t j = 0; j < n_jobs; j++)
            if (jobs[j].ref_len >= SA_PAIR8_MAX_COORD || jobs[j].n_events >= SA_PAIR8_MAX_COORD) return SA_EUNSUPPORTED;
        for (long long r = 0; r < pl->n_regions; r++)
            if (pl->regions[r].max_p > 1) return SA_EUNSUPPORTED;
    }
    b->relax = !(flags & SA_FLAG_EXACT) && !b->expect && m->hdp == nullptr;
    b->ring_cap = 0;
    b->gen_threads = 64;
    b->wide_cap = 0;
    {   // register-kernel regions with diagonals too wide for the registers: an LDS ring of up to 256 cells per row
        long long widest = 0;
        for (long long r = 0; r < pl->n_regions; r++)
            if (pl->regions[r].kind == SA_KIND_FAST && pl->regions[r].slots > 1 && pl->regions[r].max_rowpaths > widest)
                widest = pl->regions[r].max_rowpaths;
        if (widest > 0) b->wide_cap = (int) (widest < 256 ? (widest + 31) / 32 * 32 : 256);
    }
    for (long long r = 0; r < pl->n_regions; r++)
        if (pl->regions[r].kind == SA_KIND_GENERIC && pl->regions[r].max_rowpaths > 64) b->gen_threads = 128;
    if (b->relax) {
        long long cap = 0;
        for (long long r = 0; r < pl->n_regions; r++)
            if (pl->regions[r].kind == SA_KIND_GENERIC && pl->regions[r].max_rowpaths > cap) cap = pl->regions[r].max_rowpaths;
        // diagonals wider than the ring go through global memory one by one; a small ring keeps many waves per CU
        b->ring_cap = (int) (cap < 128 ? cap : 128);
    }
    // (round 4: the model tables, the plan arrays of a host-built plan and the emission constants go up here too -- with
    // sa_batch_prepare that is while the batch before this one still runs; nothing of it needs the working storage)
    std::unique_lock<std::mutex> up_lock((*UPT).mu);
    TRY((*UPT).bind(device));
    if (trace_c) fprintf(stderr, "[trace] create: upload ring ready at %.1f ms\n", now_ms() - tc0);
    {   // candidate capacity an earlier batch of this stream had to grow to
        const int f = pl->params.threshold > 0.0 ? cand_memo_factor(m, pl->params.threshold, device) : 1;
        if (f > 1) {
            sa_plan_grow_candidates(pl, f);
            b->cand_factor = f;
            if (b->dev_planned && pl->n_segs > 0)   // its segments are in HBM already: the copy is stream-ordered behind the planner
                TRY((*UPT).copy(b->d_segs, pl->segs, sizeof(sa_seg_t) * (size_t) pl->n_segs));
        }
    }
    const bool big_pinned = pl->pooled && pl->big_free == plan_pinned_free;   // the big arrays are pinned: no staging
    if (!b->dev_planned) {
        TRY(upload(&b->d_regions, pl->regions, pl->n_regions));
        TRY(upload(&b->d_rows, pl->rows, pl->n_rows, 192, big_pinned));   // (the ring kernels read row tiles up to 127 entries past a region)
        TRY(upload(&b->d_pk, pl->pk, pl->n_pk, 0, big_pinned));
        TRY(upload(&b->d_poff, pl->poff, pl->n_poff, 0, big_pinned));
        TRY(upload(&b->d_pid, pl->pid, pl->n_pid, 0, big_pinned));
        // per-path records: only batches that hold ring-kernel regions with several paths per cell have (and read) them
        bool need = false;
        for (long long r = 0; r < pl->n_regions && !need; r++) need = pl->regions[r].kind == SA_KIND_RING && pl->regions[r].max_p > 1;
        if (need && pl->prec) TRY(upload(&b->d_prec, pl->prec, pl->n_pid, 0, big_pinned));
    }
    std::vector<int> px;   // (alive until the uploader has drained)
    {   // cell-path -> reference position, for the memory-resident kernels (one lane per cell-path); register-kernel
        // regions never read it
        bool any_generic = false;
        for (long long r = 0; r < pl->n_regions && !any_generic && !b->dev_planned; r++) any_generic = pl->regions[r].kind == SA_KIND_GENERIC;
        if (any_generic) {
            px.assign((size_t) at_least_1(pl->n_pid), 0);
            for (long long r = 0; r < pl->n_regions; r++) {
                const sa_region_t *R = &pl->regions[r];
                if (R->kind != SA_KIND_GENERIC) continue;
                const int32_t *po = pl->poff + R->poff_off;
                for (long long x = 0; x <= R->lX; x++)
                    for (int g = po[x]; g < po[x + 1]; g++) px[(size_t) (R->pid_off + g)] = (int) x;
            }
            TRY(upload(&b->d_px, px.data(), pl->n_pid));
        } else {
            TRY(upload(&b->d_px, (const int *) nullptr, 0));
        }
    }
    // readable padding behind the events: the kernels clamp event indices to 0 even for reads without events
    if (!b->dev_planned) {
        TRY(upload(&b->d_ev, pl->ev, pl->n_ev, 8, big_pinned));
        TRY(upload(&b->d_segs, pl->segs, pl->n_segs));
        TRY(upload(&b->d_cks, pl->cks, pl->n_cks));
    }
    TRY(upload_model_tables(b, pl));
    if ((flags & SA_FLAG_VC_ROWS) && !b->expect) TRY(upload_vc_rows(b, pl));
    {   // emission constants, on the device (same stream as the uploads they read)
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &b->d_xc, sizeof(double) * 4 * (size_t) at_least_1(pl->n_pid), device) != hipSuccess)
            return SA_ENOMEM;
        if (pl->n_regions > 0)
            hipLaunchKernelGGL(k_fill_xc, dim3((unsigned) pl->n_regions), dim3(256), 0, (*UPT).stream, b->d_regions, b->d_poff,
                               b->d_pid, b->d_tab6, m->hdp ? b->d_hdp_slot : (const int *) nullptr,
                               m->hdp ? (long long) m->hdp->grid_length : 0ll, reinterpret_cast<double4 *>(b->d_xc), m->emission);
        if (hipGetLastError() != hipSuccess) return SA_ENODEVICE;
    }
    TRY((*UPT).drain());
    up_lock.unlock();
    if (trace_c) fprintf(stderr, "[trace] create: inputs uploaded at %.1f ms\n", now_ms() - tc0);
    TRY(batch_build_lists(b));
    if (trace_c) fprintf(stderr, "[trace] create: launch lists at %.1f ms\n", now_ms() - tc0);
    return SA_OK;
}

// The forward storage in passes of at most `budget` cell-paths; the kernels read chunk / f_base from the device copy of the regions
static int repack_forward(sa_batch *b, long long budget) {
    sa_plan_t *pl = b->plan;
    sa_plan_repack(pl, budget);
    TRY(batch_build_lists(b));
    if (pl->n_regions > 0 && hipMemcpy(b->d_regions, pl->regions, sizeof(sa_region_t) * (size_t) pl->n_regions, hipMemcpyHostToDevice) != hipSuccess) {
        (void) hipGetLastError();
        return SA_ENODEVICE;
    }
    return SA_OK;
}

static int batch_finish_body(sa_batch *b) {
    const sa_model_t *m = b->c_m;
    const unsigned flags = b->flags;
    const int device = b->device;
    const bool trace_c = getenv("SA_TRACE") != nullptr;
    const double tc0 = b->c_t0;
    HIPCHK(hipSetDevice(device));
    SaUploader *const UPT = batch_uploader(b);
    UseUploader use_upt_(UPT);
    sa_plan_t *pl = b->plan;
    // Working buffers and launch lists.  What does not fit is planned again: a deferred batch's storage budget dates from its first
    // half -- other batches may have taken the memory since --, SA_FLAG_DEVICE_TO_ITSELF is a promise the caller can break, and
    // candidate / result slots (HDP models, low thresholds) are sized after the budget was set.  When an allocation fails, what
    // this attempt took goes back, the forward storage is re-packed into more passes of half the size at most (regions keep
    // everything else of their plan: only regions[].chunk / f_base change) and the attempt is repeated; SA_ENOMEM only when a
    // single region's planes and the fixed buffers do not fit together.
    double working_bytes = 0.0;
    auto dalloc = [&](void **p_, long long bytes) -> int {
        const hipError_t e_ = g_sa_pool.get(SaPool::DEVICE, p_, (size_t) (bytes > 0 ? bytes : 8), device);
        if (e_ != hipSuccess) {
            (void) hipGetLastError();
            return e_ == hipErrorOutOfMemory ? SA_ENOMEM : SA_ENODEVICE;
        }
        working_bytes += (double) (bytes > 0 ? bytes : 8);
        return SA_OK;
    };
    // SA_TEST_FAIL_WORKING_ALLOC=n (test hook): an attempt fails as if out of memory while the plan has fewer than n passes
    const int test_min_passes = getenv("SA_TEST_FAIL_WORKING_ALLOC") ? atoi(getenv("SA_TEST_FAIL_WORKING_ALLOC")) : 0;
    auto build_working = [&]() -> int {
        working_bytes = b->d_blk ? (double) b->d_blk_bytes : 0.0;   // (the image of the caller's block stays until the batch goes)
        if (pl->n_chunks < test_min_passes && pl->n_regions > pl->n_chunks) return SA_ENOMEM;
        TRY(dalloc((void **) &b->d_F, 24 * pl->max_chunk_cellpaths));
        // HDP: the emission plane of the register-, ring- and strip-kernel regions (one value per cell-path, laid out like the match plane)
        if (m->hdp && pl->n_fast_regions + pl->n_ring_regions > 0) TRY(dalloc((void **) &b->d_E, 8 * pl->max_chunk_cellpaths));
        TRY(dalloc((void **) &b->d_vbuf, 8 * pl->n_vbuf));
        TRY(dalloc((void **) &b->d_cands, (long long) sizeof(sa_cand_t) * pl->n_cand));
        TRY(dalloc((void **) &b->d_prob, 8 * pl->n_cand));
        b->cand_alloc = pl->n_cand;
        TRY(dalloc((void **) &b->d_cand_count, 4 * pl->n_segs));
        TRY(dalloc((void **) &b->d_seg_pass, 4 * pl->n_segs));
        TRY(dalloc((void **) &b->d_seg_off, 8 * (2 * pl->n_segs + 8)));  // n+1 offsets per group
        TRY(dalloc((void **) &b->d_totals, 8 * pl->n_cks));
        TRY(dalloc((void **) &b->d_bscratch, 8 * pl->n_bscratch));
        if (b->expect) {
            TRY(dalloc((void **) &b->d_gsum, 64 * pl->n_cks));
            TRY(dalloc((void **) &b->d_gmc, 8 * pl->n_cks));
        }
        // launch lists (batch_build_lists: with the plan): seam storage, speculative totals, sort keys, events
        {
            const bool host_finalize = (flags & SA_FLAG_EXACT) || b->expect;
            const long long strip_max_n = b->lw_strip_max_n, strip_max_seg = b->lw_strip_max_seg;
            const long long strip_fwd_slots = b->lw_strip_fwd_slots, strip_bwd_slots = b->lw_strip_bwd_slots;
            if (strip_fwd_slots + strip_bwd_slots > 0) {
                // seam storage: per wave two arrays of (diagonals of the longest strip-kernel region / traceback segment + lead-in
                // + sentinels) records; the groups of a pass run side by side, every segment has its own slot behind the forward
                // launch's
                b->seam_cap = (unsigned) (strip_max_n + 16);
                b->seam_cap_bwd = (unsigned) (strip_max_seg + 16);
                b->seam_bwd_off = strip_fwd_slots * 32ll * (long long) b->seam_cap;
                TRY(dalloc((void **) &b->d_seam, b->seam_bwd_off + strip_bwd_slots * 32ll * (long long) b->seam_cap_bwd));
            }
            if ((pl->n_ring_regions + pl->n_fast_regions > 0 && !host_finalize) || (b->expect && pl->n_ring_regions > 0)) {
                // register, ring and strip kernels: candidates against the traceback's speculative total (one per segment)
                TRY(dalloc((void **) &b->d_spec, 8ll * at_least_1(pl->n_segs)));
            }
            // k_gather_sorted: sort keys per candidate slot.  A 64-bit key holds 24 bits of diagonals below a traceback's start (de << 40).
            if (strip_fwd_slots > 0 && !host_finalize) {
                TRY(dalloc((void **) &b->d_sortkey, 8ll * at_least_1(pl->n_cand)));
                TRY(dalloc((void **) &b->d_sortidx, 4ll * at_least_1(pl->n_cand)));
            }
            b->group_ev.resize(b->groups.size());
            b->chunk_ev.resize(b->chunks.size());
            for (sa_group_events &e : b->group_ev) TRY(events_make(e, device));
            for (sa_chunk_events &e : b->chunk_ev) TRY(events_make(e, device));
            if (g_sa_pool.get(SaPool::PINNED, (void **) &b->h_seg_off, 8 * (size_t) (pl->n_segs + (long long) b->groups.size() + 1),
                              device) != hipSuccess ||
                g_sa_pool.get(SaPool::PINNED, (void **) &b->h_overflow, 64, device) != hipSuccess) {
                return SA_ENOMEM;
            }
            if (!host_finalize) {
                TRY(dalloc((void **) &b->d_out, (long long) sizeof(sa_pair16_t) * pl->n_cand));
                b->out_alloc = pl->n_cand;
            }
        }
        return SA_OK;
    };
    auto release_working = [&]() {
        b->put_blocks(0, sa_batch::BLK_PLAN);
        if (b->h_seg_off) { g_sa_pool.put(SaPool::PINNED, b->h_seg_off); b->h_seg_off = nullptr; }
        if (b->h_overflow) { g_sa_pool.put(SaPool::PINNED, b->h_overflow); b->h_overflow = nullptr; }
        for (sa_group_events &e : b->group_ev) events_park(e, device);
        for (sa_chunk_events &e : b->chunk_ev) events_park(e, device);
        b->group_ev.clear(); b->chunk_ev.clear();
        b->seam_cap = 0; b->seam_cap_bwd = 0; b->seam_bwd_off = 0;
    };
    // A batch whose RESULTS take longer to cross PCIe than its kernels take to run (broad HDP densities at a low threshold: hundreds of
    // millions of pairs) ends when its last copy ends, and its first copy cannot start before the forward sweep of its first pass has
    // finished: such a batch sweeps in four passes instead of one, so that the first groups' pairs travel while the later passes
    // compute (5000 HDP reads at threshold 0.01, 8-byte records: 87 -> 76 ms per step; the kernels themselves lose 5 ms to the
    // smaller launches).  The estimate is the pairs-per-event of the last finished batch of this kind (g_pairs_memo).
    if (!(flags & SA_FLAG_EXACT) && !b->expect && pl->n_chunks == 1 && pl->n_regions >= 64 && !getenv("SA_F_BUDGET_CELLPATHS")) {
        const double est_bytes = g_pairs_memo.estimate(pl->model->uid, b->device, pl->params.threshold) * (double) pl->n_ev * (double) b->rec();
        if (est_bytes > 2.0e9) {
            long long total = 0, largest = 1;
            for (long long r = 0; r < pl->n_regions; r++) {
                total += pl->regions[r].f_cellpaths;
                largest = pl->regions[r].f_cellpaths > largest ? pl->regions[r].f_cellpaths : largest;
            }
            TRY(repack_forward(b, (total + 3) / 4 + largest));   // (a pass closes before the region that would overflow it: four at most)
            if (trace_c) fprintf(stderr, "[trace] create: %.1f GB of pairs expected: forward storage in %d passes\n", est_bytes / 1e9, (int) pl->n_chunks);
        }
    }
    {
        int rcw = SA_OK;
        for (int attempt = 0; attempt < 6; attempt++) {
            rcw = build_working();
            if (rcw != SA_ENOMEM) break;
            release_working();
            long long largest = 1;
            for (long long r = 0; r < pl->n_regions; r++) largest = pl->regions[r].f_cellpaths > largest ? pl->regions[r].f_cellpaths : largest;
            if (pl->max_chunk_cellpaths <= largest) break;   // one region per pass already: nothing left to give
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); free_b = 0; }
            free_b += g_sa_pool.idle_bytes(SaPool::DEVICE, device);
            long long budget2 = pl->max_chunk_cellpaths / 2;
            const long long by_free = (long long) (0.5 * (double) free_b / (m->hdp ? 32.0 : 24.0));
            if (by_free > 0 && by_free < budget2) budget2 = by_free;
            if (budget2 < largest) budget2 = largest;
            TRY(repack_forward(b, budget2));
            if (trace_c || !test_min_passes)
                fprintf(stderr, "[signalalign_hip] working storage did not fit: forward storage re-packed into %d passes of at most %.1f GB\n",
                        (int) pl->n_chunks, (m->hdp ? 32.0 : 24.0) * (double) pl->max_chunk_cellpaths / 1e9);
        }
        if (rcw == SA_ENOMEM) fprintf(stderr, "[signalalign_hip] working storage does not fit the device\n");
        if (rcw) return rcw;
    }
    {   // the launch lists (small)
        std::lock_guard<std::mutex> g_((*UPT).mu);
        TRY((*UPT).bind(device));
        TRY(upload(&b->d_ids, b->ids_flat.data(), (long long) b->ids_flat.size()));
        TRY((*UPT).drain());
    }
    if (trace_c) fprintf(stderr, "[trace] create: buffers allocated at %.1f ms\n", now_ms() - tc0);
    b->stats.cells_forward = pl->cells_fwd;
    b->stats.cells_backward = pl->cells_bwd;
    b->stats.n_regions = pl->n_regions;
    b->stats.n_segments = pl->n_segs;
    b->stats.n_checkpoints = pl->n_cks;
    b->stats.n_fast_regions = pl->n_fast_regions;
    b->stats.n_ring_regions = pl->n_ring_regions;
    b->stats.n_strip_regions = 0;
    for (const auto &C_ : b->chunks) b->stats.n_strip_regions += C_.ids[LC_STRIP].n;
    b->stats.n_chunks = pl->n_chunks;
    b->stats.n_groups = (int64_t) b->groups.size();
    double fb = 0;
    for (long long r = 0; r < pl->n_regions; r++)   // (HDP register-kernel regions: 8 B more per cell, the emission plane)
        fb += (m->hdp && pl->regions[r].kind != SA_KIND_GENERIC ? 32.0 : 24.0) * (double) pl->regions[r].f_cellpaths;
    b->stats.f_bytes = fb;
    b->stats.device_bytes = working_bytes;
    // The pinned result buffer, from an estimate of the result size (measured: 0.9 pairs per event at the default threshold): taken
    // here and not at the start of the run, so that a stream of batches asks the pinned cache for its blocks in the same order in
    // every step.  Taken by the runner thread, the third buffer of a three-deep pipeline was first needed whenever three runs
    // happened to overlap -- sometimes during the caller's warm-up, sometimes in the middle of its timed loop: a 100 ms
    // hipHostMalloc that also held up every other thread's HIP calls (12.5 against 16-19 ms per step, run to run).
    if (!(flags & SA_FLAG_EXACT) && !b->expect && b->h_pairs_cap == 0 && pl->params.threshold >= 0.005) {
        const long long cap = pairs_block_cap(expected_pairs(b));
        if (g_sa_pool.get(SaPool::PINNED, (void **) &b->h_pairs, b->rec() * (size_t) cap, device) == hipSuccess) b->h_pairs_cap = cap;
        else { (void) hipGetLastError(); b->h_pairs = nullptr; }   // (the run asks again)
    }
    if (trace_c) fprintf(stderr, "[trace] create: done at %.1f ms\n", now_ms() - tc0);
    return SA_OK;
}

// Second half of a batch's creation: the plan (the device planner's results, or the host planner), the remaining uploads, the
// working buffers and the launch lists.  Runs once, on the batch's first use (run, statistics, accessors) or at the end of
// sa_batch_create; a failure is remembered and returned to every later caller.
static int batch_finish(sa_batch *b) {
    std::lock_guard<std::mutex> g(b->fin_mu);
    if (!b->finished) {
        b->finish_rc = b->prepared ? b->prepare_rc : batch_prepare_body(b);
        if (b->finish_rc == SA_OK) b->finish_rc = batch_finish_body(b);
        b->finished = true;
        if (b->finish_rc != SA_OK) {
            // Memsets, uploads and k_fill_xc of this batch may still be queued on the upload stream it used; sa_batch_destroy
            // only waits for the batch's own streams before its blocks go back to the caching allocator, where a batch being
            // created on the other uploader could receive them while that work still writes.  Drain the stream here.
            SaUploader *const U = batch_uploader(b);
            if (U->stream && U->device == b->device) (void) sa_sync_stream(U->stream, b->device);
        }
    }
    return b->finish_rc;
}

// The event noise of a two-distribution model's jobs (a record's second value), read where the caller left it -- pageable memory or a
// page-locked block alike.  upload_model_tables stores n, log n, 1 / n and 1.5 log n of it for every event, and the register kernels
// evaluate the noise term in every lane, the ones without a k-mer / event pair included: a NaN there is not confined to the event's
// own row.  The reference gives such a read a NaN total and no pairs (NaN, +-inf, negative; zero without the 1e-9 replacement of
// impl/stateMachine.c:619-621, i.e. under SA_EMISSION_TWO_DIST_SCALED_MODEL: log 0 - log 0).  Such a batch is refused before anything
// is launched, in the wording of sa_batch_run's line for event means.  Finite positive values of any size are legal.
static int event_noise_check(const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs) {
    if (m->emission == SA_EMISSION_MEAN_ONLY || !jobs) return SA_OK;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_job_t *jb = &jobs[j];
        if (jb->n_events <= 0 || jb->event_stride < 2 || !jb->events) continue;   // (stride 1: refused where the noise is read)
        for (int64_t i = 0; i < jb->n_events; i++) {
            const double n = jb->events[i * jb->event_stride + 1];
            const bool legal = (n > 0.0 && n < INFINITY) || (n == 0.0 && m->emission == SA_EMISSION_TWO_DIST);
            if (!legal) {
                fprintf(stderr, "[signalalign_hip] an event noise (job %lld, event %lld) is not a finite number greater than zero: no result\n",
                        (long long) j, (long long) i);
                return SA_EINVAL;
            }
        }
    }
    return SA_OK;
}

static int batch_create_impl(sa_batch_t **out, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                             const char *const *ambig, int device, unsigned flags, bool deferred,
                             const sa_noise_scale_t *noise = nullptr, bool noise_scaled = false) {
    if (!out || !m || !p) return SA_EINVAL;
    if (const int rc = sa_device_check(device)) return rc;
    if (const int rc = event_noise_check(m, jobs, n_jobs)) return rc;
    // Threshold 0 keeps every band cell, the ones of posterior 0 included: the default kernels' candidate filter (forward +
    // backward >= checkpoint maximum + log threshold) has no lower bound then and would pass lanes that hold no cell.  Such a
    // batch takes the reference-ordered kernels with host finalisation, which list a diagonal's cells explicitly.
    if (!(p->threshold > 0.0)) flags |= SA_FLAG_EXACT;
    // The two-distribution emission (sa_model_set_emission) exists in the reference-ordered memory-resident kernels and, since round
    // 6, in the register kernels (k_fwd_fast_two / k_bwd_fast_two: one path per cell; wide stretches through their in-kernel
    // memory-resident path).  A batch whose regions are not ALL register-kernel regions (an ambiguity letter, a matrix that the
    // planner splits beyond their limits) is planned again as with SA_FLAG_EXACT (batch_prepare_body); the expectation pass keeps the
    // reference-ordered kernels.  (SA_TWO_DIST_FAST_OFF=1: always the reference-ordered kernels, as up to round 5.)
    if (m->emission != 0 && ((flags & (SA_FLAG_EXPECT_INTERNAL | SA_FLAG_FORCE_GENERIC)) || getenv("SA_TWO_DIST_FAST_OFF")))
        flags |= SA_FLAG_EXACT;
    // SA_FLAG_TWO_DIST_ALL_KERNELS: the ring and strip kernels' two-distribution instances (sa_plan.c plans such a batch's regions as a
    // MeanOnly model's); nothing to do for a MeanOnly model, no such instance for an HDP model
    if ((flags & SA_FLAG_TWO_DIST_ALL_KERNELS) && m->hdp) return SA_EUNSUPPORTED;
    if (noise_scaled) {   // sa_batch_create_noise_scaled: per-job factors on the noise columns (batch_prepare_body applies them)
        if (!(flags & SA_FLAG_TWO_DIST_ALL_KERNELS) || m->emission == 0 || n_jobs < 0 || (n_jobs > 0 && (!noise || !jobs))) return SA_EINVAL;
        for (int64_t j = 0; j < n_jobs; j++) {
            const double a_ = noise[j].scale_sd, b_ = noise[j].var_sd;
            if (!(a_ > 0.0) || !(b_ > 0.0) || a_ == INFINITY || b_ == INFINITY || jobs[j].event_stride < 2) return SA_EINVAL;
        }
        if (flags & SA_FLAG_EXACT) return SA_EUNSUPPORTED;   // (the reference-ordered kernels read the model's own noise columns)
    }
    if (flags & SA_FLAG_EXPECT_INTERNAL) flags &= ~(SA_FLAG_SITE_CALLS | SA_FLAG_POSITION_CALLS);
    if ((flags & (SA_FLAG_SITE_CALLS | SA_FLAG_POSITION_CALLS)) && (flags & SA_FLAG_VC_ROWS)) return SA_EINVAL;   // (that flag drops the rows the calls are made of)
    if ((flags & SA_FLAG_POSITION_CALLS) && (flags & SA_FLAG_PAIRS8)) return SA_EUNSUPPORTED;   // (an 8-byte record names no path k-mer)
    const bool trace_c = getenv("SA_TRACE") != nullptr;
    const double tc0 = now_ms();
    HIPCHK(hipSetDevice(device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (trace_c) fprintf(stderr, "[trace] create: memory queried at %.1f ms\n", now_ms() - tc0);
    free_b += g_sa_pool.idle_bytes(SaPool::DEVICE, device);   // what destroyed batches left parked is available to this one
    if (deferred && (flags & SA_FLAG_DEVICE_TO_ITSELF)) free_b += g_sa_pool.live_bytes(SaPool::DEVICE, device);   // ... and what the running ones hold
    // forward storage gets at most 60% of what is free; 24 B per cell-path (HDP models: 8 B more, the emission plane)
    long long budget = (long long) ((double) free_b * 0.60 / (m->hdp ? 32.0 : 24.0));
    const char *envb = getenv("SA_F_BUDGET_CELLPATHS");  // test hook: force several passes
    if (envb && atoll(envb) > 0) budget = atoll(envb);

    sa_batch *b = new sa_batch();
    std::unique_ptr<sa_batch, void (*)(sa_batch *)> owner(b, sa_batch_destroy);   // a failure below destroys the batch
    b->c_m = m; b->c_k = m->k; b->c_n_alpha = m->n_alpha; b->c_p = *p; b->c_jobs = jobs; b->c_n = n_jobs; b->c_ambig = ambig; b->c_budget = budget; b->c_t0 = tc0;
    if (noise_scaled) b->c_noise.assign(noise, noise + n_jobs);
    b->device = device;
    b->flags = flags;
    // the exact totals of a traceback drift away from its speculative total diagonal by diagonal (1.6e-4 per diagonal with the flat
    // HDP fixture: sa_strip.inc), so the slack is sized for the traceback's length -- the default 0.5 at the default 1100 diagonals --
    // and starts from what earlier batches of this model on this device had to grow to
    b->spec_slack = STRIP_SPEC_SLACK * std::max(1.0, (double) (p->min_diags_between_trace_back + p->trace_back_diagonals) / 1100.0);
    b->spec_slack = spec_memo_slack(m, device, b->spec_slack);
    if (const char *ets = getenv("SA_TEST_SPEC_SLACK")) {   // test hook: a slack the totals' drift exceeds, so that the repeat below is exercised
        const double v_ = atof(ets);
        if (v_ > 0.0) b->spec_slack = v_;
    }
    if (flags & (SA_FLAG_SITE_CALLS | SA_FLAG_POSITION_CALLS)) {   // every job's sites / ambiguous positions: one pass over its reference each
        TRY(n_jobs > 0 && !jobs ? SA_EINVAL : SA_OK);
        if (flags & SA_FLAG_SITE_CALLS) {
            TRY(sa_ambig_build(m, jobs, n_jobs, ambig, m->k - 1, &b->ambig_tab[SA_TAB_SITES]));
            // (an 8-byte record names no k-mer: such a batch may hold no site)
            if ((flags & SA_FLAG_PAIRS8) && sa_ambig_count(b->ambig_tab[SA_TAB_SITES]) > 0) return SA_EUNSUPPORTED;
        }
        if (flags & SA_FLAG_POSITION_CALLS)
            TRY(m->k > SA_POS_MAX_K ? SA_EUNSUPPORTED : sa_ambig_build(m, jobs, n_jobs, ambig, 0, &b->ambig_tab[SA_TAB_POSITIONS]));
    }
    if (!b->lanes.lane(0, device) || !b->lanes.lane(1, device) || g_handles.stream(&b->lanes.pair, device, 1) != hipSuccess) return SA_ENODEVICE;
    TRY(events_make(b->ev, device));
    // ---- the plan: on the device when the batch allows it (sa_dplan.inc: its first half here), else on the host ----
    {
        std::lock_guard<std::mutex> dp_lock(g_uploader.mu);
        TRY(g_uploader.bind(device));
        const int rcd = dplan_front(b, m, p, jobs, n_jobs, ambig, flags, budget, &b->pending);
        if (rcd < 0) return rcd;
    }
    b->c_deferred = deferred && b->pending != nullptr;
    if (!b->c_deferred) TRY(batch_finish(b));   // (a batch the device planner does not take is planned on the host right away)
    *out = owner.release();
    return SA_OK;
}

int sa_batch_create(sa_batch_t **out, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                    const char *const *ambig, int device, unsigned flags) {
    return batch_create_impl(out, m, p, jobs, n_jobs, ambig, device, flags, false);
}
int sa_batch_create_noise_scaled(sa_batch_t **out, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs,
                                 const sa_noise_scale_t *noise, int64_t n_jobs, const char *const *ambig, int device, unsigned flags) {
    return batch_create_impl(out, m, p, jobs, n_jobs, ambig, device, flags, false, noise, true);
}
int sa_batch_create_deferred(sa_batch_t **out, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                             const char *const *ambig, int device, unsigned flags) {
    return batch_create_impl(out, m, p, jobs, n_jobs, ambig, device, flags, true);
}

// Test hook: plans the batch twice -- on the device (sa_dplan.inc) and with sa_plan.c -- and compares every array the kernels
// read, byte for byte.  Returns 0 when all agree, a bit mask of the arrays that differ (1 regions, 2 rows, 4 packed words,
// 8 path offsets, 16 k-mer ids, 32 events, 64 segments, 128 checkpoints, 256 totals, 512 per-path records), 1 << 30 when the batch is not one the
// device planner takes, or a negative SA_E* code.
int sa_dplan_compare(const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs, const char *const *ambig,
                     int device, unsigned flags) {
    if (!m || !p) return SA_EINVAL;
    HIPCHK(hipSetDevice(device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    free_b += g_sa_pool.idle_bytes(SaPool::DEVICE, device);
    long long budget = (long long) ((double) free_b * 0.60 / 24.0);
    const char *envb = getenv("SA_F_BUDGET_CELLPATHS");
    if (envb && atoll(envb) > 0) budget = atoll(envb);
    sa_batch *b = new sa_batch();
    b->device = device;
    int rcd;
    {
        std::unique_lock<std::mutex> lk(g_uploader.mu);
        rcd = g_uploader.bind(device);
        if (rcd == SA_OK) rcd = dplan_build(b, m, p, jobs, n_jobs, ambig, flags, budget);
    }
    if (rcd != SA_OK) {
        sa_batch_destroy(b);
        return rcd < 0 ? rcd : (1 << 30);
    }
    sa_plan_t *hp = nullptr;
    int rc = sa_plan_build(&hp, m, p, jobs, n_jobs, ambig, flags | SA_FLAG_DEVICE_XC_INTERNAL, budget);
    if (rc) { sa_batch_destroy(b); return rc; }
    const sa_plan_t *dp = b->plan;
    int mask = 0;
    auto differs = [&](const void *dev, const void *host, size_t bytes) -> bool {
        if (bytes == 0) return false;
        std::vector<char> tmp(bytes);
        if (hipMemcpy(tmp.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return true;
        return memcmp(tmp.data(), host, bytes) != 0;
    };
    if (dp->n_regions != hp->n_regions || dp->n_segs != hp->n_segs || dp->n_cks != hp->n_cks || dp->n_rows != hp->n_rows ||
        dp->n_pk != hp->n_pk || dp->n_poff != hp->n_poff || dp->n_pid != hp->n_pid || dp->n_ev != hp->n_ev ||
        dp->n_vbuf != hp->n_vbuf || dp->n_cand != hp->n_cand || dp->n_bscratch != hp->n_bscratch ||
        dp->n_chunks != hp->n_chunks || dp->max_chunk_cellpaths != hp->max_chunk_cellpaths ||
        dp->n_fast_regions != hp->n_fast_regions || dp->n_ring_regions != hp->n_ring_regions || dp->cells_fwd != hp->cells_fwd ||
        dp->cells_bwd != hp->cells_bwd)
        mask |= 256;
    if (!(mask & 256)) {
        if (differs(b->d_regions, hp->regions, sizeof(sa_region_t) * (size_t) hp->n_regions) ||
            memcmp(dp->regions, hp->regions, sizeof(sa_region_t) * (size_t) hp->n_regions) != 0)
            mask |= 1;
        if (differs(b->d_rows, hp->rows, sizeof(sa_row_t) * (size_t) hp->n_rows)) mask |= 2;
        if (differs(b->d_pk, hp->pk, 4 * (size_t) hp->n_pk)) mask |= 4;
        if (differs(b->d_poff, hp->poff, 4 * (size_t) hp->n_poff)) mask |= 8;
        if (differs(b->d_pid, hp->pid, 4 * (size_t) hp->n_pid)) mask |= 16;
        if (differs(b->d_ev, hp->ev, 8 * (size_t) hp->n_ev)) mask |= 32;
        if (differs(b->d_segs, hp->segs, sizeof(sa_seg_t) * (size_t) hp->n_segs) ||
            memcmp(dp->segs, hp->segs, sizeof(sa_seg_t) * (size_t) hp->n_segs) != 0)
            mask |= 64;
        if (differs(b->d_cks, hp->cks, sizeof(sa_ck_t) * (size_t) hp->n_cks)) mask |= 128;
        for (int64_t r = 0; r < hp->n_regions; r++) {   // per-path records: they exist for these regions only
            const sa_region_t *R = &hp->regions[r];
            if (R->kind != SA_KIND_RING || R->max_p <= 1) continue;
            if (!b->d_prec || !hp->prec ||
                differs(b->d_prec + R->pid_off, hp->prec + R->pid_off, sizeof(sa_prec_t) * (size_t) hp->poff[R->poff_off + R->lX + 1]))
                mask |= 512;
        }
        for (int64_t j = 0; j < hp->n_jobs; j++)
            if (memcmp(&dp->jobs[j], &hp->jobs[j], sizeof(sa_jobinfo_t)) != 0) mask |= 256;
    }
    sa_plan_free(hp);
    sa_batch_destroy(b);
    return mask;
}
