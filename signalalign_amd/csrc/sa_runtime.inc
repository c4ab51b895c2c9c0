// sa_runtime.inc -- the process-wide host runtime under the batches (no device code): parked streams and events, the two upload
// rings, the pinned and host-block allocators, the pool API, and what one batch leaves for the next of its kind (candidate
// capacity, speculative slack, pairs per event).  Included by sa_hip.hip ahead of sa_batch.
// HIPCHK(call): a failed HIP call is reported and returned as an SA_E* code; TRY(x): a non-zero SA_E* code is returned as it is
#define HIPCHK(call)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "[signalalign_hip] %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                                 \
            return e_ == hipErrorOutOfMemory ? SA_ENOMEM : SA_ENODEVICE;                       \
        }                                                                                      \
    } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
static long long at_least_1(long long n) { return n > 0 ? n : 1; }   // elements of a block or vector that may not be empty

static double now_ms() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// Streams and events of destroyed batches, kept per device for the next batch (creating three streams and ~50 events is
// 10 ms per batch).  Handles are only parked after the batch has drained them.
struct SaHandles {
    std::mutex mu;
    struct S { hipStream_t s; int dev; int kind; };   // kind 0: compute, 1: high priority
    struct E { hipEvent_t e; int dev; };
    std::vector<S> streams;
    std::vector<E> events;
    hipError_t stream(hipStream_t *out, int dev, int kind) {
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < streams.size(); i++)
                if (streams[i].dev == dev && streams[i].kind == kind) {
                    *out = streams[i].s;
                    streams.erase(streams.begin() + (long) i);
                    return hipSuccess;
                }
        }
        if (kind == 0) return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
        int lo = 0, hi = 0;
        (void) hipDeviceGetStreamPriorityRange(&lo, &hi);
        return hipStreamCreateWithPriority(out, hipStreamNonBlocking, hi);
    }
    hipError_t event(hipEvent_t *out, int dev) {
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = events.size(); i-- > 0;)
                if (events[i].dev == dev) {
                    *out = events[i].e;
                    events.erase(events.begin() + (long) i);
                    return hipSuccess;
                }
        }
        // blocking: a host thread that waits on one of these sleeps instead of spinning (see sa_sync_stream)
        return hipEventCreateWithFlags(out, hipEventBlockingSync);
    }
    void park(hipStream_t s, int dev, int kind) {
        if (!s) return;
        if (!SaPool::enabled()) { (void) hipStreamDestroy(s); return; }
        std::lock_guard<std::mutex> g(mu);
        streams.push_back(S{s, dev, kind});
    }
    void park(hipEvent_t e, int dev) {
        if (!e) return;
        if (SaPool::enabled()) {
            std::lock_guard<std::mutex> g(mu);   // events.size() is read under the lock: batches may be destroyed from several threads
            if (events.size() <= 4096) {
                events.push_back(E{e, dev});
                return;
            }
        }
        (void) hipEventDestroy(e);
    }
    void release() {
        std::lock_guard<std::mutex> g(mu);
        for (S &x : streams) (void) hipStreamDestroy(x.s);
        for (E &x : events) (void) hipEventDestroy(x.e);
        streams.clear();
        events.clear();
    }
};
static SaHandles g_handles;

// Waits for a stream without spinning: hipStreamSynchronize busy-waits by default, and a pipeline with several batches in
// flight then burns one CPU per waiting thread -- inside a container with a CPU quota that pushes the process over its
// share and the kernel throttles ALL its threads for the rest of the accounting period (measured: 40 ms stalls in
// sa_batch_create).  An event created with hipEventBlockingSync sleeps on an interrupt instead.
static hipError_t sa_sync_stream(hipStream_t s, int dev) {
    hipEvent_t e = nullptr;
    if (g_handles.event(&e, dev) != hipSuccess) { (void) hipGetLastError(); return hipStreamSynchronize(s); }
    hipError_t r = hipEventRecord(e, s);
    if (r == hipSuccess) r = hipEventSynchronize(e);
    g_handles.park(e, dev);
    return r;
}

// Host -> device copies of the plan (several hundred MB per batch) through a persistent ring of pinned buffers: the
// runtime's own staging of pageable memory moves about 3 GB/s; here the CPU copy into a pinned slot (all host threads)
// overlaps the DMA of the previous slots.  One ring per process and device, calls serialise on it.
struct SaUploader {
    std::mutex mu;
    int device = -1;
    static const int SLOTS = 4;
    static const size_t SLOT_BYTES = (size_t) 16 << 20;
    void *slot[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t done[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t stream = nullptr;
    int next = 0;
    int bind(int dev) {
        if (device == dev && stream) return SA_OK;
        // (a process normally drives one GPU; a change of device rebuilds the ring)
        for (int i = 0; i < SLOTS; i++) {
            if (slot[i]) (void) hipHostFree(slot[i]);
            if (done[i]) (void) hipEventDestroy(done[i]);
            slot[i] = nullptr; done[i] = nullptr;
        }
        if (stream) (void) hipStreamDestroy(stream);
        stream = nullptr;
        device = dev;
        // highest priority: the uploads and the device planner of the NEXT batch run while the current batch's sweeps fill the
        // chip; at normal priority their (short) kernels wait for wave slots behind thousands of long-running waves and
        // sa_batch_create takes 18 ms instead of 8
        int prio_lo = 0, prio_hi = 0;
        (void) hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        if (hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio_hi) != hipSuccess) return SA_ENODEVICE;
        for (int i = 0; i < SLOTS; i++) {
            if (hipHostMalloc(&slot[i], SLOT_BYTES, hipHostMallocDefault) != hipSuccess) return SA_ENOMEM;
            if (hipEventCreateWithFlags(&done[i], hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) return SA_ENODEVICE;
        }
        return SA_OK;
    }
    int copy_pinned(void *dst, const void *src, size_t bytes) {   // the source is pinned: plain DMA
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
        return SA_OK;
    }
    int copy(void *dst, const void *src, size_t bytes) {
        const char *s = (const char *) src;
        char *d = (char *) dst;
        while (bytes > 0) {
            const size_t n = bytes < SLOT_BYTES ? bytes : SLOT_BYTES;
            const int k = next;
            next = (next + 1) % SLOTS;
            HIPCHK(hipEventSynchronize(done[k]));            // the slot's previous DMA has left it
            char *buf = (char *) slot[k];
            const size_t piece = (size_t) 1 << 20;
            sa_parallel_for((n + piece - 1) / piece, [&](size_t q) {
                const size_t a = q * piece, len = a + piece < n ? piece : n - a;
                memcpy(buf + a, s + a, len);
            });
            HIPCHK(hipMemcpyAsync(d, buf, n, hipMemcpyHostToDevice, stream));
            HIPCHK(hipEventRecord(done[k], stream));
            s += n; d += n; bytes -= n;
        }
        return SA_OK;
    }
    int drain() {
        HIPCHK(sa_sync_stream(stream, device));
        return SA_OK;
    }
};
static SaUploader g_uploader;
// A second one for the second half of a batch's creation (batch_finish_body): with sa_batch_create_deferred that half runs on the
// batch's runner thread while the caller's thread is inside the NEXT batch's first half, which holds g_uploader for as long as it
// packs and uploads the reads (60 ms for a 10k-event slice) -- the batch that is ready to run would wait for it.
static SaUploader g_uploader_tail;
static thread_local SaUploader *tl_uploader = &g_uploader;   // the one upload() uses on this thread
struct UseUploader {   // ... for the lifetime of one of these
    SaUploader *prev;
    explicit UseUploader(SaUploader *u) : prev(tl_uploader) { tl_uploader = u; }
    ~UseUploader() { tl_uploader = prev; }
};
SaPool g_sa_pool;
SaWorkers g_sa_workers;

// the planner's big arrays as pinned memory of the caching allocator (the device then reads them by plain DMA)
static void *plan_pinned_alloc(size_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    void *p = nullptr;
    if (g_sa_pool.get(SaPool::PINNED, &p, bytes, dev) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
    return p;
}
static void plan_pinned_free(void *p, size_t bytes) { (void) bytes; g_sa_pool.put(SaPool::PINNED, p); }

extern "C" int sa_pool_configure(int64_t device_limit_bytes, int64_t pinned_limit_bytes) {
    if (device_limit_bytes >= 0) SaPool::configured(SaPool::DEVICE).store((long long) device_limit_bytes);
    if (pinned_limit_bytes >= 0) SaPool::configured(SaPool::PINNED).store((long long) pinned_limit_bytes);
    g_sa_pool.trim(SaPool::DEVICE);
    g_sa_pool.trim(SaPool::PINNED);
    return SA_OK;
}

// sa_host_alloc: page-locked blocks a caller fills with its reads' arrays (SA_FLAG_INPUTS_IN_HOST_BLOCK).  hipHostMalloc's default
// flags make them visible to every device of the process; the registry is what lets sa_batch_create check that a job's pointers
// really lie in such a block before a DMA is pointed at them.
static std::mutex g_host_blocks_mu;
static std::map<const char *, size_t> g_host_blocks;   // first byte -> bytes
extern "C" void *sa_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes > 0 ? bytes : 8, hipHostMallocDefault) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> g(g_host_blocks_mu);
    g_host_blocks[(const char *) p] = bytes > 0 ? bytes : 8;
    return p;
}
extern "C" void sa_host_free(void *block) {
    if (!block) return;
    {
        std::lock_guard<std::mutex> g(g_host_blocks_mu);
        auto it = g_host_blocks.find((const char *) block);
        if (it == g_host_blocks.end()) return;
        g_host_blocks.erase(it);
    }
    (void) hipHostFree(block);
}
// the block that holds `p`, if any
static bool sa_host_block_of(const char *p, const char **base, size_t *bytes) {
    std::lock_guard<std::mutex> g(g_host_blocks_mu);
    auto it = g_host_blocks.upper_bound(p);
    if (it == g_host_blocks.begin()) return false;
    --it;
    if (p >= it->first + it->second) return false;
    *base = it->first;
    *bytes = it->second;
    return true;
}

extern "C" void sa_pool_release_device(void) {
    g_sa_pool.release(SaPool::DEVICE);
}
extern "C" void sa_pool_release(void) {
    g_sa_pool.release(SaPool::DEVICE);
    g_sa_pool.release(SaPool::PINNED);
    sa_plan_pool_release();
    g_handles.release();
}

template <typename T>
static int upload(T **dst, const T *src, long long n, long long pad = 0, bool src_pinned = false) {
    // pad: extra zeroed elements behind the data (kernels that clamp an index may read one element past the end)
    size_t bytes = sizeof(T) * (size_t) at_least_1(n + pad);
    SaUploader &U = *tl_uploader;
    HIPCHK(g_sa_pool.get(SaPool::DEVICE, (void **) dst, bytes, U.device));
    if (pad > 0) HIPCHK(hipMemsetAsync((char *) *dst + sizeof(T) * (size_t) n, 0, sizeof(T) * (size_t) pad, U.stream));
    if (n > 0) return src_pinned ? U.copy_pinned(*dst, src, sizeof(T) * (size_t) n) : U.copy(*dst, src, sizeof(T) * (size_t) n);
    return SA_OK;
}

// What the last overflow taught: batches of one stream resemble each other, so the next batch of the same model and threshold
// starts with the candidate capacity the previous one had to grow to (a re-run of the whole pass costs a batch's kernel
// time again: the HDP workload at threshold 0.1 ran 73 instead of 37 ms per batch until it stopped overflowing every time).
// Keyed on the model OBJECT (its uid, not its address: the CLI clones and destroys a model per read and addresses come back), the
// threshold and the device; a few entries, least recently used out.  The factor is not for ever: after `patience` batches in a
// row without an overflow the next batch is planned one step (x4) lower; if that one overflows the old factor is back and the
// patience is four times longer -- one outlier batch no longer inflates every later batch's candidate, probability and result
// slots 4-16x.
struct SaCandMemo {
    struct Entry { uint64_t uid; double threshold; int device; int factor; int quiet; int patience; bool probing; uint64_t used; };
    std::mutex mu;
    std::vector<Entry> e;
    uint64_t clock = 0;
    Entry *find(uint64_t uid, double thr, int dev) {
        for (auto &x : e)
            if (x.uid == uid && x.threshold == thr && x.device == dev) { x.used = ++clock; return &x; }
        return nullptr;
    }
};
static SaCandMemo g_cand_memo;
static int cand_memo_factor(const sa_model_t *m, double threshold, int device) {   // once per batch created
    std::lock_guard<std::mutex> g(g_cand_memo.mu);
    SaCandMemo::Entry *x = g_cand_memo.find(m->uid, threshold, device);
    if (!x) return 1;
    if (x->probing && x->quiet >= 8) x->probing = false;   // the lower capacity held for eight batches
    if (x->factor > 1 && ++x->quiet >= x->patience) { x->factor /= 4; if (x->factor < 1) x->factor = 1; x->quiet = 0; x->probing = true; }
    return x->factor;
}
static void cand_memo_note(const sa_model_t *m, double threshold, int device, int factor) {   // a batch overflowed and grew to `factor`
    std::lock_guard<std::mutex> g(g_cand_memo.mu);
    SaCandMemo::Entry *x = g_cand_memo.find(m->uid, threshold, device);
    if (!x) {
        if (g_cand_memo.e.size() >= 32) {
            size_t lru = 0;
            for (size_t i = 1; i < g_cand_memo.e.size(); i++) if (g_cand_memo.e[i].used < g_cand_memo.e[lru].used) lru = i;
            g_cand_memo.e.erase(g_cand_memo.e.begin() + (long) lru);
        }
        g_cand_memo.e.push_back({m->uid, threshold, device, factor, 0, 64, false, ++g_cand_memo.clock});
        return;
    }
    if (factor > x->factor) x->factor = factor;
    if (x->probing && x->patience < (1 << 20)) x->patience *= 4;   // the lower capacity did not hold
    x->probing = false;
    x->quiet = 0;
}

// The slack of the speculative candidate bound (sa_strip.inc: STRIP_SPEC_SLACK) a model had to grow to on a device is remembered
// too: a stream of batches whose totals drift further than the default allows (longer tracebacks, densities broader than the
// bundled HDP's) would otherwise run every batch's pass twice.  Keyed like the candidate capacity; +inf is remembered as well.
struct SaSpecMemo {
    struct Entry { uint64_t uid; int device; double slack; uint64_t used; };
    std::mutex mu;
    std::vector<Entry> e;
    uint64_t clock = 0;
};
static SaSpecMemo g_spec_memo;
static double spec_memo_slack(const sa_model_t *m, int device, double dflt) {
    std::lock_guard<std::mutex> g(g_spec_memo.mu);
    for (auto &x : g_spec_memo.e)
        if (x.uid == m->uid && x.device == device) { x.used = ++g_spec_memo.clock; return x.slack > dflt ? x.slack : dflt; }
    return dflt;
}
static void spec_memo_note(const sa_model_t *m, int device, double slack) {
    std::lock_guard<std::mutex> g(g_spec_memo.mu);
    for (auto &x : g_spec_memo.e)
        if (x.uid == m->uid && x.device == device) { if (slack > x.slack) x.slack = slack; x.used = ++g_spec_memo.clock; return; }
    if (g_spec_memo.e.size() >= 32) {
        size_t lru = 0;
        for (size_t i = 1; i < g_spec_memo.e.size(); i++) if (g_spec_memo.e[i].used < g_spec_memo.e[lru].used) lru = i;
        g_spec_memo.e.erase(g_spec_memo.e.begin() + (long) lru);
    }
    g_spec_memo.e.push_back({m->uid, device, slack, ++g_spec_memo.clock});
}

// Pairs per event of the last finished batch of the same MODEL (its uid: a broad HDP at threshold 0.01 returns 17.8 pairs per event, a
// narrow model beside it 0.9), device and threshold, process-wide: the estimate the NEXT such batch's pinned result block is sized
// from (a batch whose estimate is short copies its pairs after its kernels instead of beside them).  Clamped to [1.5, 64] pairs per
// event; a pinned block that cannot be had at the estimated size is not an error (the run copies after its kernels, as without one).
struct SaPairsMemo {
    std::mutex mu;
    struct E { uint64_t uid; int device; double thr, ratio; };
    E e[8] = {};
    int next = 0;
    void note(uint64_t uid, int device, double threshold, double pairs, double events) {
        if (!(events > 0)) return;
        std::lock_guard<std::mutex> g(mu);
        for (int i = 0; i < 8; i++)
            if (e[i].uid == uid && e[i].device == device && e[i].thr == threshold && e[i].ratio > 0) { e[i].ratio = pairs / events > 1e-9 ? pairs / events : 1e-9; return; }
        e[next] = E{uid, device, threshold, pairs / events > 1e-9 ? pairs / events : 1e-9};
        next = (next + 1) & 7;
    }
    double estimate(uint64_t uid, int device, double threshold) {
        std::lock_guard<std::mutex> g(mu);
        for (int i = 0; i < 8; i++)
            if (e[i].uid == uid && e[i].device == device && e[i].thr == threshold && e[i].ratio > 0) {
                const double r = e[i].ratio * 1.1;
                return r < 1.5 ? 1.5 : (r > 64.0 ? 64.0 : r);
            }
        return 1.5;
    }
};
static SaPairsMemo g_pairs_memo;
