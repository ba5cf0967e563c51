// tbk_count.cpp — host side of the k-mer counter behind find-unique-kmers.
//
// The reference's find_unique_kmers.py is subprocess glue around KMC 3 (kmc, kmc_tools, kmc_dump;
// find_unique_kmers.py:62-233).  KMC is not part of the reference checkout, so what is restated
// here is its published behaviour at the call sites' settings:
//   kmc -k<k> -t<n> @files db tmp     canonical k-mers of all reads, both strands; k-mers holding
//                                     a symbol outside ACGT are skipped; defaults -ci2 (k-mers seen
//                                     once are not stored), -cs255 (counters saturate at 255)
//   kmc_tools transform db histogram  one row per counter value: value <tab> number of k-mers
//   kmc_tools simple A B kmers_subtract   k-mers of A that B does not hold
//   kmc_dump -ci<a> -cx<b> db out     k-mers with a <= counter <= b, in lexicographic order
// Parity with KMC itself is unpinned (no binary, no golden output in the reference); the tests
// check this code against a CPU restatement of the list above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_compact_host.h"
#include "tbk_lookup_host.h"

extern "C" void tbk_set_error_(int code, const char *msg);
extern "C" hipError_t tbk_launch_separate(const uint8_t *, const uint64_t *, uint64_t, uint8_t *, hipStream_t);
extern "C" hipError_t tbk_launch_count(const uint8_t *, uint64_t, uint64_t, uint64_t, int, uint64_t *, uint32_t, TbkMz, int *, unsigned long long *,
                                       hipStream_t);
extern "C" uint64_t tbk_probe_passes(uint64_t total);
extern "C" hipError_t tbk_launch_count_clamp(uint64_t *, uint32_t, TbkMz, hipStream_t);
extern "C" hipError_t tbk_launch_count_rehash(uint64_t *, uint32_t, TbkMz, uint64_t *, uint32_t, TbkMz, int *, hipStream_t);
extern "C" hipError_t tbk_launch_count_histogram(uint64_t *, uint32_t, TbkMz, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_count_unique(uint64_t *, uint32_t, TbkMz, uint64_t *, uint32_t, TbkMz, int, uint32_t, uint32_t,
                                              uint64_t *, uint64_t, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_sort_u64(const uint64_t *, uint64_t *, uint64_t, int, hipStream_t);
// pass mode
extern "C" hipError_t tbk_launch_retain(const uint8_t *, uint64_t, uint64_t *, uint64_t, hipStream_t);
extern "C" hipError_t tbk_launch_count_class(const uint64_t *, uint64_t, uint64_t, uint64_t, int, uint64_t *, uint32_t, TbkMz, int *, unsigned long long *,
                                             uint32_t, uint32_t, hipStream_t);
extern "C" hipError_t tbk_launch_count_distil(uint64_t *, uint32_t, TbkMz, uint32_t, uint64_t *, uint8_t *, uint64_t, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_db_solid_keys(const uint64_t *, const uint8_t *, uint64_t, uint64_t *, uint64_t, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_db_unique(const uint64_t *, const uint8_t *, uint64_t, const uint64_t *, uint64_t, int, uint32_t, uint32_t, uint64_t *,
                                           uint64_t, unsigned long long *, hipStream_t);

static int cfail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    tbk_set_error_(code, buf);
    return code;
}
#define CHIP(expr)                                                                                                      \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess)                                                                                           \
            return cfail(e_ == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct tbk_counter {
    int device = 0, k = 0;
    uint64_t *d_lines = nullptr;  // n_buckets lines of 128 B: 8 keys | 8 x 32-bit counters | 32 spare bytes
    uint32_t n_buckets = 0;
    TbkMz mz{0, 0, 0, 0};
    int *d_failed = nullptr;
    unsigned long long *d_used = nullptr;  // [0] slots taken so far (distinct k-mers met), [1 .. 1024] tallies of the 64-bit atomic adds issued: kept by the kernels
    uint64_t since_clamp = 0;              // window starts counted since the counters were last held below 2^31 (tbk_count_clamp_kernel)
    uint64_t used = 0;
    double load = 0.6;
    // staging of one batch: reads back to back, their offsets, and the separated upper-cased copy
    uint8_t *d_raw = nullptr, *d_sep = nullptr;
    uint64_t *d_off = nullptr;
    size_t cap_raw = 0, cap_sep = 0, cap_reads = 0;
    uint64_t bases_added = 0, reads_added = 0;
    // HIP-event timing of the counting kernel (every launch; read by tbk_counter_kernel_timing)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint64_t timed_launches = 0, timed_windows = 0;
    double timed_ms = 0.0;
    uint64_t peak_table_bytes = 0;  // the largest table this counter has held
    bool finished = false;          // no more batches (tbk_counter_finish)
    bool broken = false;            // finishing failed half way: nothing more can be asked of the counter
    // ---- pass mode (passes > 1) -----------------------------------------------------------------------
    // The canonical k-mers fall into `passes` classes (tbk_class_of).  Every batch is retained on the device in
    // packed form (tbk_retain_kernel) while class 0 is counted from it; finishing distils class 0 into its
    // database - the keys seen at least twice and their capped counters - counts class 1, 2, ... from the store
    // into the same table, distilling each, and then frees store and table.  The table only ever holds one class.
    int passes = 1;
    uint64_t store_limit = 0;  // bytes the store may take (0: what HBM gives)
    struct Segment { uint64_t *d = nullptr; uint64_t cap = 0, used = 0; };  // 64-bit words
    struct Piece { uint32_t segment; uint64_t first, words; };              // one batch: whole words of one segment
    std::vector<Segment> segments;
    std::vector<Piece> pieces;
    uint64_t store_bytes = 0, store_words = 0;  // allocated bytes; words in use
    struct ClassDb { uint64_t *d_keys = nullptr; uint8_t *d_counts = nullptr; uint64_t n = 0; };
    std::vector<ClassDb> db;                    // one per finished class
    uint64_t database_bytes = 0;
    unsigned long long *d_hist = nullptr;       // running histogram of the classes distilled so far
    uint64_t hist[256] = {0};                   // its host copy
    uint64_t distinct_done = 0;                 // distinct k-mers of the classes distilled so far
    bool compress = false;                      // tbk_counter_options.compress: the k-mers are those of the homopolymer-compressed reads
    tbk_hpc *hpc = nullptr;                     // its session: every batch goes through it (freed with the store when a counter in passes finishes)
    bool keep_singletons = false;               // tbk_counter_options.keep_singletons: the database (and every class's) holds the k-mers seen once too
    uint32_t floor() const { return keep_singletons ? 1u : 2u; }  // the lowest counter a database of this counter holds
};

static int counter_device(const tbk_counter *c) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return cfail(TBK_ERR_NO_DEVICE, "no HIP device visible; libtbk_hip has no CPU fallback");
    CHIP(hipSetDevice(c->device));
    return TBK_OK;
}

// lines for `capacity` distinct k-mers at the counter's target load; keys = all ones (free), counters = 0
static int alloc_lines(int k, uint64_t capacity, double load, uint64_t **d_lines, uint32_t *n_buckets, TbkMz *mz, uint64_t *peak) {
    uint64_t nb = (uint64_t)((double)capacity / (TBK_SLOTS_PER_BUCKET * load)) + 16;
    if (nb > 0x7FFFFFF0ull) return cfail(TBK_ERR_NOMEM, "%llu distinct k-mers are more than one table holds", (unsigned long long)capacity);
    const size_t bytes = (size_t)nb * 128;
    hipError_t e = hipMalloc((void **)d_lines, bytes);
    if (e == hipSuccess) e = hipMemset2D(*d_lines, 128, 0xFF, 64, nb);
    if (e == hipSuccess) e = hipMemset2D((uint8_t *)*d_lines + 64, 128, 0, 64, nb);
    if (e != hipSuccess) {
        if (*d_lines) (void)hipFree(*d_lines);
        *d_lines = nullptr;
        (void)hipGetLastError();
        return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "counting table for %llu k-mers (%zu bytes): %s",
                     (unsigned long long)capacity, bytes, hipGetErrorString(e));
    }
    *n_buckets = (uint32_t)nb;
    if (peak && bytes > *peak) *peak = bytes;
    const char *ew = getenv("TBK_COUNT_W"), *em = getenv("TBK_COUNT_M");
    *mz = tbk_mz_params(k, ew ? atoi(ew) : 6, capacity, em ? atoi(em) : 0, 0);
    return TBK_OK;
}

extern "C" void tbk_counter_options_init(tbk_counter_options *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->size = (uint32_t)sizeof *o;
    o->passes = 1;
}

extern "C" int tbk_counter_create(int k, uint64_t capacity_kmers, int device, tbk_counter **out) {
    return tbk_counter_create_opts(k, capacity_kmers, nullptr, device, out);
}

extern "C" int tbk_counter_create_opts(int k, uint64_t capacity_kmers, const tbk_counter_options *opts, int device, tbk_counter **out) {
    if (!out) return cfail(TBK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (k < 1 || k > 32) return cfail(TBK_ERR_INVALID, "k = %d out of range (1..32)", k);
    if (!capacity_kmers) return cfail(TBK_ERR_INVALID, "capacity is 0");
    tbk_counter_options o;
    tbk_counter_options_init(&o);
    if (opts) {
        if (opts->size < 8 || opts->size > sizeof o) return cfail(TBK_ERR_INVALID, "tbk_counter_options.size = %u (this library knows %zu bytes)", opts->size, sizeof o);
        memcpy(&o, opts, opts->size);
        o.size = (uint32_t)sizeof o;
    }
    if (o.passes < 1 || o.passes > TBK_COUNTER_MAX_PASSES)
        return cfail(TBK_ERR_INVALID, "passes = %d out of range (1..%d)", o.passes, TBK_COUNTER_MAX_PASSES);
    tbk_counter tmp;
    tmp.device = device;
    int rc = counter_device(&tmp);
    if (rc) return rc;
    // 8-slot lines at load <= 0.6.  A counting table meets every distinct k-mer of the reads,
    // sequencing errors included; the capacity is the caller's estimate, and the table is rebuilt
    // twice as large whenever the next batch could fill it.
    tbk_counter *c = new tbk_counter();
    c->device = device; c->k = k;
    c->passes = o.passes; c->store_limit = o.store_limit_bytes;
    c->compress = o.compress != 0;
    c->keep_singletons = o.keep_singletons != 0;
    if (c->compress) {
        const int made = tbk_hpc_create(device, &c->hpc);
        if (made) { delete c; return made; }
    }
    if (c->passes > 1) capacity_kmers = std::max<uint64_t>(1, capacity_kmers / (uint64_t)c->passes);  // the table holds one class
    const char *ev = getenv("TBK_COUNT_LOAD");
    c->load = ev ? atof(ev) : 0.6;
    if (c->load < 0.05) c->load = 0.05;
    if (c->load > 0.9) c->load = 0.9;
    rc = alloc_lines(k, capacity_kmers, c->load, &c->d_lines, &c->n_buckets, &c->mz, &c->peak_table_bytes);
    hipError_t e = hipSuccess;
    if (!rc && c->passes > 1) {
        e = hipMalloc((void **)&c->d_hist, 256 * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemset(c->d_hist, 0, 256 * sizeof(unsigned long long));
    }
    if (!rc) e = hipMalloc((void **)&c->d_failed, sizeof(int));
    if (!rc && e == hipSuccess) e = hipMalloc((void **)&c->d_used, 1025 * sizeof(unsigned long long));
    if (!rc && e == hipSuccess) e = hipMemset(c->d_failed, 0, sizeof(int));
    if (!rc && e == hipSuccess) e = hipMemset(c->d_used, 0, 1025 * sizeof(unsigned long long));
    if (!rc && e != hipSuccess) rc = cfail(TBK_ERR_HIP, "tbk_counter_create: %s", hipGetErrorString(e));
    if (rc) { tbk_counter_destroy(c); return rc; }
    *out = c;
    return TBK_OK;
}

// Rebuild the table for `capacity` distinct k-mers and move every (key, counter) over.
static int counter_grow(tbk_counter *c, uint64_t capacity) {
    uint64_t *d_new = nullptr;
    uint32_t nb = 0;
    TbkMz mz{0, 0, 0, 0};
    int rc = alloc_lines(c->k, capacity, c->load, &d_new, &nb, &mz, &c->peak_table_bytes);
    if (rc) return rc;
    hipError_t e = tbk_launch_count_rehash(c->d_lines, c->n_buckets, c->mz, d_new, nb, mz, c->d_failed, nullptr);
    int failed = 0;
    if (e == hipSuccess) e = hipMemcpy(&failed, c->d_failed, sizeof failed, hipMemcpyDeviceToHost);
    if (e != hipSuccess || failed) {
        (void)hipFree(d_new);
        return cfail(TBK_ERR_HIP, "counting table rebuild failed: %s", e != hipSuccess ? hipGetErrorString(e) : "new table full");
    }
    (void)hipFree(c->d_lines);
    c->d_lines = d_new; c->n_buckets = nb; c->mz = mz;
    return TBK_OK;
}

extern "C" void tbk_counter_destroy(tbk_counter *c) {
    if (!c) return;
    if (hipSetDevice(c->device) == hipSuccess) {
        (void)hipDeviceSynchronize();
        if (c->ev0) (void)hipEventDestroy(c->ev0);
        if (c->ev1) (void)hipEventDestroy(c->ev1);
        for (void *p : {(void *)c->d_lines, (void *)c->d_failed, (void *)c->d_used, (void *)c->d_raw, (void *)c->d_sep, (void *)c->d_off, (void *)c->d_hist})
            if (p) (void)hipFree(p);
        for (const tbk_counter::Segment &s : c->segments)
            if (s.d) (void)hipFree(s.d);
        for (const tbk_counter::ClassDb &d : c->db) {
            if (d.d_keys) (void)hipFree(d.d_keys);
            if (d.d_counts) (void)hipFree(d.d_counts);
        }
    }
    tbk_hpc_destroy(c->hpc);
    delete c;
}

// Count a stream of sep_total positions, the separated ASCII stream d_sep (cls < 0) or, in pass mode, the
// retained words of one batch for class cls.
static int count_stream(tbk_counter *c, const void *d_stream, uint64_t sep_total, int cls) {
    // The stream is counted in pieces of a quarter of the table's slots (at least 64 M window
    // starts).  Every window of a piece could be a k-mer never seen before, so before a piece that
    // could fill the table the table is rebuilt twice as large - a piece can then never run out of
    // room half way, and the table grows once its load passes 0.6.
    const uint64_t passes = tbk_probe_passes(sep_total);
    for (uint64_t p0 = 0; p0 < passes;) {
        uint64_t slots = (uint64_t)c->n_buckets * TBK_SLOTS_PER_BUCKET;
        // (at most 2^30 window starts however large the table: a piece on top of counters just set back to 2^31 must stay below 2^32 - see below)
        // A piece never exceeds the count launch's grid, so in product the kernel's pass loop takes one trip per block.
        constexpr uint64_t piece_cap = 1u << 19;
        static_assert(piece_cap <= TBK_COUNT_GRID_BLOCKS, "a piece of count_stream must fit the grid of one tbk_count_kernel launch");
        const uint64_t piece = std::min<uint64_t>(std::max<uint64_t>(32768, slots / 4 / 2048), piece_cap);
        const uint64_t np = std::min(piece, passes - p0), windows = np * 2048;
        if ((double)(c->used + windows) > 0.85 * (double)slots) {
            uint64_t want = (uint64_t)((double)slots * c->load) * 2;  // twice the present capacity
            while ((double)(c->used + windows) > 0.85 * ((double)want / c->load)) want *= 2;
            const int rc = counter_grow(c, want);
            if (rc) return rc;
            slots = (uint64_t)c->n_buckets * TBK_SLOTS_PER_BUCKET;
        }
        // no counter may pass 2^32 (it would carry into the neighbour it shares a 64-bit word with): one grows by at most a
        // piece's window starts, so before 2^31 of them have been added since the last clamp, every counter goes back to <= 2^31
        if (c->since_clamp + windows >= ((uint64_t)1 << 31)) {
            CHIP(tbk_launch_count_clamp(c->d_lines, c->n_buckets, c->mz, nullptr));
            c->since_clamp = 0;
        }
        c->since_clamp += windows;
        if (!c->ev0) { CHIP(hipEventCreate(&c->ev0)); CHIP(hipEventCreate(&c->ev1)); }
        CHIP(hipEventRecord(c->ev0, nullptr));
        if (cls < 0)
            CHIP(tbk_launch_count((const uint8_t *)d_stream, sep_total, p0, np, c->k, c->d_lines, c->n_buckets, c->mz, c->d_failed, c->d_used, nullptr));
        else
            CHIP(tbk_launch_count_class((const uint64_t *)d_stream, sep_total / 16, p0, np, c->k, c->d_lines, c->n_buckets, c->mz, c->d_failed, c->d_used,
                                        (uint32_t)c->passes, (uint32_t)cls, nullptr));
        CHIP(hipEventRecord(c->ev1, nullptr));
        int failed = 0;
        unsigned long long used = 0;
        CHIP(hipMemcpy(&failed, c->d_failed, sizeof failed, hipMemcpyDeviceToHost));
        {
            float ms = 0;
            CHIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            c->timed_ms += ms; c->timed_launches++; c->timed_windows += std::min<uint64_t>(windows, sep_total - p0 * 2048);
        }
        CHIP(hipMemcpy(&used, c->d_used, sizeof used, hipMemcpyDeviceToHost));
        c->used = used;
        if (failed) return cfail(TBK_ERR_NOMEM, "counting table is full (%llu slots, %llu taken)", (unsigned long long)slots, used);
        p0 += np;
    }
    return TBK_OK;
}

// Pack the separated stream of a batch (c->d_sep) into the store.  The store is a list of segments, each at least
// half as large as everything kept before it, so its growth never copies and costs O(log) allocations; a batch
// lies in one segment, on a word boundary, and is replayed from there.
static int store_append(tbk_counter *c, uint64_t sep_total, uint64_t **d_words, uint64_t *n_words) {
    const uint64_t words = (sep_total + 15) / 16;
    if (c->store_limit && (c->store_words + words) * 8 > c->store_limit)
        return cfail(TBK_ERR_NOMEM, "the retained store would pass its limit of %llu bytes: %llu bases are retained in %llu bytes, the next batch needs %llu more",
                     (unsigned long long)c->store_limit, (unsigned long long)c->bases_added, (unsigned long long)(c->store_words * 8),
                     (unsigned long long)(words * 8));
    if (c->segments.empty() || c->segments.back().cap - c->segments.back().used < words) {
        uint64_t cap = std::max<uint64_t>(words, std::max<uint64_t>((uint64_t)1 << 17, c->store_words / 2));
        if (c->store_limit) cap = std::max<uint64_t>(words, std::min<uint64_t>(cap, c->store_limit / 8 - c->store_words));
        tbk_counter::Segment seg;
        const hipError_t e = hipMalloc((void **)&seg.d, cap * 8);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "the retained store cannot grow by %llu bytes (%s): %llu bases are retained in %llu bytes",
                         (unsigned long long)(cap * 8), hipGetErrorString(e), (unsigned long long)c->bases_added, (unsigned long long)c->store_bytes);
        }
        seg.cap = cap;
        c->segments.push_back(seg);
        c->store_bytes += cap * 8;
    }
    tbk_counter::Segment &seg = c->segments.back();
    CHIP(tbk_launch_retain(c->d_sep, sep_total, seg.d + seg.used, words, nullptr));
    c->pieces.push_back({(uint32_t)(c->segments.size() - 1), seg.used, words});
    *d_words = seg.d + seg.used;
    *n_words = words;
    seg.used += words;
    c->store_words += words;
    return TBK_OK;
}

// The class just counted becomes its database; the table is empty afterwards.
static int distil_class(tbk_counter *c) {
    CHIP(tbk_launch_count_histogram(c->d_lines, c->n_buckets, c->mz, c->d_hist, nullptr));  // adds this class's rows to the running histogram
    unsigned long long h[256];
    CHIP(hipMemcpy(h, c->d_hist, sizeof h, hipMemcpyDeviceToHost));
    uint64_t keep = 0;
    for (int i = (int)c->floor(); i < 256; i++) keep += h[i] - c->hist[i];
    c->distinct_done += h[0] - c->hist[0];
    for (int i = 0; i < 256; i++) c->hist[i] = h[i];
    tbk_counter::ClassDb d;
    c->db.push_back(d);  // (owned by the counter from here on: freed with it whatever happens below)
    tbk_counter::ClassDb &db = c->db.back();
    if (keep) {
        CHIP(hipMalloc((void **)&db.d_keys, keep * sizeof(uint64_t)));
        CHIP(hipMalloc((void **)&db.d_counts, keep));
    }
    unsigned long long got = 0;
    CHIP(hipMemset(c->d_used, 0, sizeof got));  // [0] doubles as the append cursor: the class's slot count has been read
    CHIP(tbk_launch_count_distil(c->d_lines, c->n_buckets, c->mz, c->floor(), db.d_keys, db.d_counts, keep, c->d_used, nullptr));
    CHIP(hipMemcpy(&got, c->d_used, sizeof got, hipMemcpyDeviceToHost));
    CHIP(hipMemset(c->d_used, 0, sizeof got));
    if (got != keep) return cfail(TBK_ERR_HIP, "distilling a class: %llu k-mers to keep by the histogram, %llu in the table", (unsigned long long)keep, got);
    db.n = keep;
    c->database_bytes += keep * 9;
    c->used = 0;
    c->since_clamp = 0;
    return TBK_OK;
}

static int counter_finish(tbk_counter *c) {
    if (c->finished) return TBK_OK;
    if (c->broken) return cfail(TBK_ERR_INVALID, "the counter failed while it was being finished");
    if (c->passes == 1) { c->finished = true; return TBK_OK; }
    int rc = counter_device(c);
    if (rc) return rc;
    c->broken = true;  // until every class is through
    rc = distil_class(c);
    for (int cls = 1; !rc && cls < c->passes; cls++) {
        for (size_t i = 0; !rc && i < c->pieces.size(); i++) {
            const tbk_counter::Piece &pc = c->pieces[i];
            rc = count_stream(c, c->segments[pc.segment].d + pc.first, pc.words * 16, cls);
        }
        if (!rc) rc = distil_class(c);
    }
    if (rc) return rc;
    // only the databases and the histogram remain
    for (tbk_counter::Segment &sg : c->segments) (void)hipFree(sg.d);
    c->segments.clear(); c->pieces.clear();
    c->store_bytes = 0; c->store_words = 0;
    for (void **p : {(void **)&c->d_lines, (void **)&c->d_raw, (void **)&c->d_sep, (void **)&c->d_off}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    c->n_buckets = 0; c->cap_raw = 0; c->cap_sep = 0; c->cap_reads = 0;
    tbk_hpc_destroy(c->hpc);
    c->hpc = nullptr;
    c->broken = false;
    c->finished = true;
    return TBK_OK;
}

extern "C" int tbk_counter_finish(tbk_counter *c) {
    if (!c) return cfail(TBK_ERR_INVALID, "counter is NULL");
    return counter_finish(c);
}

static int counter_run(tbk_counter *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t total) {
    if (c->hpc) {
        // compressed space: the batch that is separated, counted and (in passes mode) kept is the compressed one
        void *d_cb = nullptr, *d_co = nullptr;
        const int rc = tbk_hpc_compress_device(c->hpc, d_bases, d_offsets, n_reads, total, 1, &d_cb, &d_co, &total);
        if (rc) return rc;
        d_bases = (const uint8_t *)d_cb;
        d_offsets = (const uint64_t *)d_co;
    }
    const size_t need_sep = (size_t)total + n_reads + 64;
    if (need_sep > c->cap_sep) {
        if (c->d_sep) CHIP(hipFree(c->d_sep));
        c->d_sep = nullptr; c->cap_sep = 0;
        CHIP(hipMalloc((void **)&c->d_sep, need_sep + need_sep / 8));
        c->cap_sep = need_sep + need_sep / 8;
    }
    CHIP(tbk_launch_separate(d_bases, d_offsets, n_reads, c->d_sep, nullptr));
    const uint64_t sep_total = total + n_reads;
    int rc;
    if (c->passes > 1) {
        // pass mode: keep the batch, and count class 0 from the kept words while they are at hand
        uint64_t *d_words = nullptr, n_words = 0;
        rc = store_append(c, sep_total, &d_words, &n_words);
        if (!rc) rc = count_stream(c, d_words, n_words * 16, 0);
    } else {
        rc = count_stream(c, c->d_sep, sep_total, -1);
    }
    if (rc) return rc;
    c->bases_added += total;
    c->reads_added += n_reads;
    return TBK_OK;
}

extern "C" int tbk_check_offsets_(const uint64_t *offsets, uint64_t n_reads);

extern "C" int tbk_counter_add_batch(tbk_counter *c, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads) {
    if (!c || (n_reads && (!bases || !offsets))) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (c->finished || c->broken) return cfail(TBK_ERR_INVALID, "the counter is finished: no more reads can be added");
    if (!n_reads) return TBK_OK;
    int rc = tbk_check_offsets_(offsets, n_reads);  // same rule as tbk_stream_submit
    if (rc) return rc;
    rc = counter_device(c);
    if (rc) return rc;
    const uint64_t total = offsets[n_reads];
    if (total + 16 > c->cap_raw) {
        if (c->d_raw) CHIP(hipFree(c->d_raw));
        c->d_raw = nullptr; c->cap_raw = 0;
        CHIP(hipMalloc((void **)&c->d_raw, total + total / 8 + 64));
        c->cap_raw = total + total / 8 + 64;
    }
    if (n_reads + 1 > c->cap_reads) {
        if (c->d_off) CHIP(hipFree(c->d_off));
        c->d_off = nullptr; c->cap_reads = 0;
        CHIP(hipMalloc((void **)&c->d_off, (n_reads + n_reads / 8 + 2) * sizeof(uint64_t)));
        c->cap_reads = n_reads + n_reads / 8 + 2;
    }
    CHIP(hipMemcpy(c->d_raw, bases, total, hipMemcpyHostToDevice));
    CHIP(hipMemcpy(c->d_off, offsets, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    return counter_run(c, c->d_raw, c->d_off, n_reads, total);
}

extern "C" int tbk_counter_add_device(tbk_counter *c, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t total_bases) {
    if (!c || (n_reads && (!d_bases || !d_offsets))) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (c->finished || c->broken) return cfail(TBK_ERR_INVALID, "the counter is finished: no more reads can be added");
    if (!n_reads) return TBK_OK;
    int rc = counter_device(c);
    if (rc) return rc;
    return counter_run(c, (const uint8_t *)d_bases, (const uint64_t *)d_offsets, n_reads, total_bases);
}

extern "C" int tbk_counter_kernel_timing(tbk_counter *c, uint64_t *launches, uint64_t *window_starts, double *total_ms, int reset) {
    if (!c) return cfail(TBK_ERR_INVALID, "counter is NULL");
    if (launches) *launches = c->timed_launches;
    if (window_starts) *window_starts = c->timed_windows;
    if (total_ms) *total_ms = c->timed_ms;
    if (reset) { c->timed_launches = 0; c->timed_windows = 0; c->timed_ms = 0.0; }
    return TBK_OK;
}

extern "C" int tbk_counter_adds_issued(tbk_counter *c, uint64_t *adds) {
    if (!c || !adds) return cfail(TBK_ERR_INVALID, "NULL argument");
    int rc = counter_device(c);
    if (rc) return rc;
    std::vector<unsigned long long> v(1024);
    CHIP(hipMemcpy(v.data(), c->d_used + 1, v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t sum = 0;
    for (unsigned long long x : v) sum += x;
    *adds = sum;
    return TBK_OK;
}

extern "C" int tbk_counter_histogram(tbk_counter *c, uint64_t hist[256]) {
    if (!c || !hist) return cfail(TBK_ERR_INVALID, "NULL argument");
    int rc = counter_device(c);
    if (rc) return rc;
    if (c->passes > 1) {
        rc = counter_finish(c);
        if (rc) return rc;
        for (int i = 0; i < 256; i++) hist[i] = c->hist[i];
        return TBK_OK;
    }
    unsigned long long *d_hist = nullptr;
    CHIP(hipMalloc((void **)&d_hist, 256 * sizeof(unsigned long long)));
    hipError_t e = hipMemset(d_hist, 0, 256 * sizeof(unsigned long long));
    if (e == hipSuccess) e = tbk_launch_count_histogram(c->d_lines, c->n_buckets, c->mz, d_hist, nullptr);
    unsigned long long h[256];
    if (e == hipSuccess) e = hipMemcpy(h, d_hist, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d_hist);
    if (e != hipSuccess) return cfail(TBK_ERR_HIP, "tbk_counter_histogram: %s", hipGetErrorString(e));
    for (int i = 0; i < 256; i++) hist[i] = h[i];
    return TBK_OK;
}

extern "C" int tbk_counter_distinct(const tbk_counter *c, uint64_t *distinct) {
    if (!c || !distinct) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (c->passes > 1) {  // the sum over the classes: known once all have been counted
        const int rc = counter_finish(const_cast<tbk_counter *>(c));
        if (rc) return rc;
        *distinct = c->distinct_done;
        return TBK_OK;
    }
    *distinct = c->used;
    return TBK_OK;
}

extern "C" int tbk_counter_stats(const tbk_counter *c, uint64_t *n_slots, uint64_t *table_bytes, uint64_t *bases_added, uint64_t *reads_added) {
    if (!c) return cfail(TBK_ERR_INVALID, "counter is NULL");
    if (n_slots) *n_slots = (uint64_t)c->n_buckets * TBK_SLOTS_PER_BUCKET;
    if (table_bytes) *table_bytes = (uint64_t)c->n_buckets * 128;
    if (bases_added) *bases_added = c->bases_added;
    if (reads_added) *reads_added = c->reads_added;
    return TBK_OK;
}

extern "C" int tbk_counter_params(const tbk_counter *c, int *w, int *m, int *o, int *t) {
    if (!c) return cfail(TBK_ERR_INVALID, "counter is NULL");
    if (w) *w = c->mz.w;
    if (m) *m = c->mz.m;
    if (o) *o = c->mz.o;
    if (t) *t = c->mz.t;
    return TBK_OK;
}

extern "C" int tbk_counter_stats_ex(const tbk_counter *c, tbk_counter_info *info) {
    if (!c || !info) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (info->size < 8 || info->size > sizeof(tbk_counter_info)) return cfail(TBK_ERR_INVALID, "tbk_counter_info.size = %u (this library knows %zu bytes)", info->size, sizeof(tbk_counter_info));
    tbk_counter_info v;
    memset(&v, 0, sizeof v);
    v.size = info->size;
    v.passes = c->passes;
    v.finished = c->finished ? 1 : 0;
    v.store_bytes = c->store_bytes;
    v.store_used_bytes = c->store_words * 8;
    v.peak_table_bytes = c->peak_table_bytes;
    v.database_bytes = c->database_bytes;
    v.distinct = c->distinct_done + c->used;  // classes distilled so far + the class in the table
    memcpy(info, &v, info->size);
    return TBK_OK;
}

// one k-mer per line, k characters + '\n', from lexicographic ranks (base 0 in the top bits)
static bool write_list(const char *path, const uint64_t *lex, uint64_t n, int k, std::string &err) {
    const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { err = std::string("cannot create ") + path + ": " + strerror(errno); return false; }
    const size_t line = (size_t)k + 1;
    const uint64_t per = (uint64_t)1 << 18;  // lines per piece
    const uint64_t pieces = (n + per - 1) / per;
    std::atomic<uint64_t> next{0};
    std::atomic<bool> ok{true};
    auto work = [&]() {
        std::vector<char> buf;
        for (uint64_t p; (p = next.fetch_add(1)) < pieces && ok.load();) {
            const uint64_t lo = p * per, hi = std::min(n, lo + per);
            buf.resize((size_t)(hi - lo) * line);
            char *w = buf.data();
            for (uint64_t i = lo; i < hi; i++) {
                const uint64_t v = lex[i];
                for (int b = 0; b < k; b++) *w++ = "ACGT"[(v >> (2 * (k - 1 - b))) & 3u];
                *w++ = '\n';
            }
            size_t done = 0;
            while (done < buf.size()) {
                const ssize_t r = ::pwrite(fd, buf.data() + done, buf.size() - done, (off_t)(lo * line + done));
                if (r <= 0) { ok.store(false); break; }
                done += (size_t)r;
            }
        }
    };
    const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)tbk_host_threads(), pieces));
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (std::thread &t : pool) t.join();
    const bool closed = ::close(fd) == 0;
    if (!ok.load() || !closed) { err = std::string("write failed: ") + path; return false; }
    return true;
}

extern "C" int tbk_counter_unique(tbk_counter *a, tbk_counter *b, uint32_t min_count, uint32_t max_count, const char *out_path,
                                  uint64_t *n_written) {
    if (!a || !b || !out_path || !n_written) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (a->k != b->k) return cfail(TBK_ERR_INVALID, "the counters have different k (%d and %d)", a->k, b->k);
    if (a->device != b->device) return cfail(TBK_ERR_INVALID, "the counters live on different devices");
    if (a->passes != b->passes)
        return cfail(TBK_ERR_INVALID, "the counters count in different numbers of passes (%d and %d): their classes do not match", a->passes, b->passes);
    if (a->compress != b->compress)
        return cfail(TBK_ERR_INVALID, "one counter counts homopolymer-compressed k-mers, the other plain ones: they cannot be subtracted");
    *n_written = 0;
    int rc = counter_device(a);
    if (rc) return rc;
    const bool by_class = a->passes > 1;
    if (by_class) {
        rc = counter_finish(a);
        if (!rc) rc = counter_finish(b);
        if (rc) return rc;
    }
    // upper bound of what can come out: k-mers of A with a counter in range
    uint64_t hist[256];
    rc = tbk_counter_histogram(a, hist);
    if (rc) return rc;
    uint64_t cap = 0;
    for (uint32_t cnt = std::max<uint32_t>(2, min_count); cnt <= std::min<uint32_t>(255, max_count); cnt++) cap += hist[cnt];
    uint64_t n = 0;
    std::vector<uint64_t> h_keys;
    if (cap) {
        uint64_t *d_out = nullptr, *d_sorted = nullptr;
        unsigned long long *d_n = nullptr, got = 0;
        hipError_t e = hipMalloc((void **)&d_out, cap * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&d_sorted, cap * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&d_n, sizeof got);
        if (e == hipSuccess) e = hipMemset(d_n, 0, sizeof got);
        if (e == hipSuccess && !by_class)
            e = tbk_launch_count_unique(a->d_lines, a->n_buckets, a->mz, b->d_lines, b->n_buckets, b->mz, a->k, min_count, max_count,
                                        d_out, cap, d_n, nullptr);
        if (e == hipSuccess && by_class) {
            // class by class: B's keys of the class sorted (keys alone), A's looked up among them
            // (a B that keeps its once-seen k-mers holds them in its classes: they are left out first - B "holds" what it saw twice)
            uint64_t most = 0, *d_bs = nullptr, *d_b2 = nullptr;
            unsigned long long *d_nb = nullptr;
            for (const tbk_counter::ClassDb &d : b->db) most = std::max(most, d.n);
            if (most) e = hipMalloc((void **)&d_bs, most * sizeof(uint64_t));
            if (e == hipSuccess && most && b->keep_singletons) e = hipMalloc((void **)&d_b2, most * sizeof(uint64_t));
            if (e == hipSuccess && most && b->keep_singletons) e = hipMalloc((void **)&d_nb, sizeof(unsigned long long));
            for (size_t p = 0; e == hipSuccess && p < a->db.size(); p++) {
                const tbk_counter::ClassDb &da = a->db[p], &db = b->db[p];
                if (!da.n) continue;
                const uint64_t *b_keys = db.d_keys;
                uint64_t b_n = db.n;
                if (db.n && b->keep_singletons) {
                    unsigned long long solid = 0;
                    e = hipMemset(d_nb, 0, sizeof solid);
                    if (e == hipSuccess) e = tbk_launch_db_solid_keys(db.d_keys, db.d_counts, db.n, d_b2, db.n, d_nb, nullptr);
                    if (e == hipSuccess) e = hipMemcpy(&solid, d_nb, sizeof solid, hipMemcpyDeviceToHost);
                    b_keys = d_b2;
                    b_n = std::min<uint64_t>(solid, db.n);
                }
                if (e == hipSuccess && b_n) e = tbk_launch_sort_u64(b_keys, d_bs, b_n, 2 * a->k, nullptr);
                if (e == hipSuccess)
                    e = tbk_launch_db_unique(da.d_keys, da.d_counts, da.n, d_bs, b_n, a->k, min_count, max_count, d_out, cap, d_n, nullptr);
            }
            if (e == hipSuccess) e = hipDeviceSynchronize();
            for (void *q : {(void *)d_bs, (void *)d_b2, (void *)d_nb})
                if (q) (void)hipFree(q);
        }
        if (e == hipSuccess) e = hipMemcpy(&got, d_n, sizeof got, hipMemcpyDeviceToHost);
        n = std::min<uint64_t>(got, cap);
        if (e == hipSuccess && n) e = tbk_launch_sort_u64(d_out, d_sorted, n, 2 * a->k, nullptr);
        if (e == hipSuccess && n) {
            h_keys.resize(n);
            e = hipMemcpy(h_keys.data(), d_sorted, n * sizeof(uint64_t), hipMemcpyDeviceToHost);
        }
        if (d_out) (void)hipFree(d_out);
        if (d_sorted) (void)hipFree(d_sorted);
        if (d_n) (void)hipFree(d_n);
        if (e != hipSuccess) return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_counter_unique: %s", hipGetErrorString(e));
    }
    std::string err;
    if (!write_list(out_path, h_keys.data(), n, a->k, err)) return cfail(TBK_ERR_IO, "%s", err.c_str());
    *n_written = n;
    return TBK_OK;
}

// =====================================================================================================================
// Count databases (tbk_kmerdb): what `kmc` leaves under --outpath in the reference (find_unique_kmers.py:247) - the
// k-mers seen at least twice with their capped counters - as an object that outlives its counter, goes to a file
// and comes back, and is subtracted from another at cut-offs the caller names.  Keys are lexicographic ranks in
// ascending order, so subtraction is a bisection and a dump needs no conversion.
// =====================================================================================================================
extern "C" hipError_t tbk_launch_count_export(uint64_t *, uint32_t, TbkMz, int, uint32_t, uint64_t *, uint8_t *, uint64_t, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_db_rank(const uint64_t *, const uint8_t *, uint64_t, int, uint64_t *, uint8_t *, hipStream_t);
extern "C" hipError_t tbk_launch_kmerdb_unique(const uint64_t *, const uint8_t *, uint64_t, const uint64_t *, uint64_t, uint32_t, uint32_t, uint64_t *,
                                               uint64_t, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_sort_u64_u8(const uint64_t *, uint64_t *, const uint8_t *, uint8_t *, uint64_t, int, hipStream_t);

struct tbk_kmerdb {
    int device = 0, k = 0;
    uint64_t n = 0;
    uint64_t *d_keys = nullptr;   // n ranks, strictly ascending
    uint8_t *d_counts = nullptr;  // their counters, floor..255
    uint64_t hist[256] = {0};     // the counter's whole histogram (tbk_counter_histogram)
    uint64_t reads_added = 0, bases_added = 0;
    bool compressed = false;      // counted in homopolymer-compressed space: another magic in the file, no mixing with plain ones
    uint32_t floor = 2;           // the lowest counter held: 2, or 1 for a FULL database (the k-mers seen once are entries too: n == hist[0])
};

// The subtractions test membership in `b` by key alone and the list builders select from counter 2 up: a full database
// among their arguments would silently count its once-seen k-mers as held.
static int kmerdb_not_full(const tbk_kmerdb *db, const char *which, const char *who) {
    if (db->floor >= 2) return TBK_OK;
    return cfail(TBK_ERR_INVALID, "%s: %s database is a full one (it holds the k-mers seen once): make its solid form with tbk_kmerdb_solid first", who, which);
}

// two databases in different spaces share no k-mer worth comparing
static int kmerdb_same_space(const tbk_kmerdb *a, const tbk_kmerdb *b, const char *what_b) {
    if (a->compressed == b->compressed) return TBK_OK;
    return cfail(TBK_ERR_INVALID, "the first database holds %s k-mers, %s %s ones: they cannot be compared",
                 a->compressed ? "homopolymer-compressed" : "plain", what_b, b->compressed ? "homopolymer-compressed" : "plain");
}

static int kmerdb_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return cfail(TBK_ERR_NO_DEVICE, "no HIP device visible; libtbk_hip has no CPU fallback");
    CHIP(hipSetDevice(device));
    return TBK_OK;
}

extern "C" void tbk_kmerdb_destroy(tbk_kmerdb *db) {
    if (!db) return;
    if ((db->d_keys || db->d_counts) && hipSetDevice(db->device) == hipSuccess) {
        if (db->d_keys) (void)hipFree(db->d_keys);
        if (db->d_counts) (void)hipFree(db->d_counts);
    }
    delete db;
}

extern "C" int tbk_counter_export(tbk_counter *c, tbk_kmerdb **out) {
    if (!c || !out) return cfail(TBK_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (c->broken) return cfail(TBK_ERR_INVALID, "the counter failed while it was being finished");
    int rc = counter_device(c);
    if (rc) return rc;
    if (c->passes > 1) {
        rc = counter_finish(c);
        if (rc) return rc;
    }
    uint64_t hist[256];
    rc = tbk_counter_histogram(c, hist);
    if (rc) return rc;
    uint64_t n = 0;
    for (int i = (int)c->floor(); i < 256; i++) n += hist[i];
    tbk_kmerdb *db = new tbk_kmerdb();
    db->device = c->device; db->k = c->k; db->n = n;
    db->floor = c->floor();
    db->reads_added = c->reads_added; db->bases_added = c->bases_added;
    db->compressed = c->compress;
    memcpy(db->hist, hist, sizeof hist);
    if (n) {
        // the pairs as they come out of the table or the classes, then ordered by rank into the database's own arrays
        uint64_t *d_rk = nullptr;
        uint8_t *d_rc = nullptr;
        unsigned long long *d_n = nullptr, got = 0;
        hipError_t e = hipMalloc((void **)&db->d_keys, n * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&db->d_counts, n);
        if (e == hipSuccess) e = hipMalloc((void **)&d_rk, n * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&d_rc, n);
        if (e == hipSuccess && c->passes == 1) {
            e = hipMalloc((void **)&d_n, sizeof got);  // (a cursor of its own: the counter's d_used stays as it is)
            if (e == hipSuccess) e = hipMemset(d_n, 0, sizeof got);
            if (e == hipSuccess) e = tbk_launch_count_export(c->d_lines, c->n_buckets, c->mz, c->k, c->floor(), d_rk, d_rc, n, d_n, nullptr);
            if (e == hipSuccess) e = hipMemcpy(&got, d_n, sizeof got, hipMemcpyDeviceToHost);
        } else if (e == hipSuccess) {
            for (const tbk_counter::ClassDb &d : c->db) {
                if (got + d.n > n) { got += d.n; continue; }  // (reported below; nothing is written past the arrays)
                if (e == hipSuccess) e = tbk_launch_db_rank(d.d_keys, d.d_counts, d.n, c->k, d_rk + got, d_rc + got, nullptr);
                got += d.n;
            }
        }
        const bool complete = got == n;
        if (e == hipSuccess && complete) e = tbk_launch_sort_u64_u8(d_rk, db->d_keys, d_rc, db->d_counts, n, 2 * c->k, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        for (void *p : {(void *)d_rk, (void *)d_rc, (void *)d_n})
            if (p) (void)hipFree(p);
        if (e != hipSuccess || !complete) {
            tbk_kmerdb_destroy(db);
            (void)hipGetLastError();
            if (e != hipSuccess) return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_counter_export (%llu k-mers): %s", (unsigned long long)n, hipGetErrorString(e));
            return cfail(TBK_ERR_HIP, "tbk_counter_export: %llu k-mers to keep by the histogram, %llu in the counter", (unsigned long long)n, got);
        }
    }
    c->finished = true;  // (a counter in passes is already)
    *out = db;
    return TBK_OK;
}

// ---- the file (*.tbkdb; INTEGRATION.md has the table) ---------------------------------------------------------------------
static const char TBK_KMERDB_MAGIC[8] = {'T', 'B', 'K', 'K', 'M', 'D', 'B', '1'};
static const char TBK_KMERDB_MAGIC_HPC[8] = {'T', 'B', 'K', 'K', 'M', 'D', 'H', '1'};  // a compressed database: the same layout under another name
// full databases (the k-mers seen once are entries): two more names for the same layout, which an older build refuses at the magic
static const char TBK_KMERDB_MAGIC_FULL[8] = {'T', 'B', 'K', 'K', 'M', 'F', 'B', '1'};
static const char TBK_KMERDB_MAGIC_FULL_HPC[8] = {'T', 'B', 'K', 'K', 'M', 'F', 'H', '1'};
constexpr size_t TBK_KMERDB_HEADER = 2096;

struct KmerdbHeader {
    int k = 0;
    uint64_t n = 0, reads = 0, bases = 0, hist[256] = {0};
    bool compressed = false;
    uint32_t floor = 2;
};

// little-endian hosts only (as the rest of the library: x86-64 beside the MI355X)
template <typename T> static void put_le(uint8_t *p, T v) { memcpy(p, &v, sizeof v); }
template <typename T> static T get_le(const uint8_t *p) { T v; memcpy(&v, p, sizeof v); return v; }

static bool write_all(int fd, const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    while (n) {
        const ssize_t r = ::write(fd, b, n);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        b += r; n -= (size_t)r;
    }
    return true;
}

static bool read_all(int fd, void *p, size_t n) {
    uint8_t *b = (uint8_t *)p;
    while (n) {
        const ssize_t r = ::read(fd, b, n);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        b += r; n -= (size_t)r;
    }
    return true;
}

// Header of an open file, checked against itself and the file's size: nothing of the content is trusted before this passes.
static int kmerdb_read_header(int fd, const char *path, KmerdbHeader *h) {
    const off_t end = ::lseek(fd, 0, SEEK_END);
    if (end < 0 || ::lseek(fd, 0, SEEK_SET) != 0) return cfail(TBK_ERR_IO, "%s: %s", path, strerror(errno));
    const uint64_t size = (uint64_t)end;
    if (size < TBK_KMERDB_HEADER) return cfail(TBK_ERR_FORMAT, "%s: %llu bytes are less than the header of a k-mer database (%zu)", path, (unsigned long long)size, TBK_KMERDB_HEADER);
    uint8_t b[TBK_KMERDB_HEADER];
    if (!read_all(fd, b, sizeof b)) return cfail(TBK_ERR_IO, "%s: cannot read the header: %s", path, strerror(errno));
    h->floor = (memcmp(b, TBK_KMERDB_MAGIC_FULL, 8) == 0 || memcmp(b, TBK_KMERDB_MAGIC_FULL_HPC, 8) == 0) ? 1 : 2;
    h->compressed = memcmp(b, h->floor == 1 ? TBK_KMERDB_MAGIC_FULL_HPC : TBK_KMERDB_MAGIC_HPC, 8) == 0;
    if (h->floor == 2 && !h->compressed && memcmp(b, TBK_KMERDB_MAGIC, 8) != 0) return cfail(TBK_ERR_FORMAT, "%s: not a k-mer database (magic)", path);
    if (get_le<uint32_t>(b + 8) != TBK_KMERDB_HEADER) return cfail(TBK_ERR_FORMAT, "%s: header size %u, expected %zu", path, get_le<uint32_t>(b + 8), TBK_KMERDB_HEADER);
    const uint32_t k = get_le<uint32_t>(b + 12);
    if (k < 1 || k > 32) return cfail(TBK_ERR_FORMAT, "%s: k = %u out of range (1..32)", path, k);
    const uint32_t crc = tbk_crc32_c(0, b, TBK_KMERDB_HEADER - 8);
    if (crc != get_le<uint32_t>(b + TBK_KMERDB_HEADER - 8)) return cfail(TBK_ERR_FORMAT, "%s: header checksum mismatch (damaged file)", path);
    if (get_le<uint32_t>(b + TBK_KMERDB_HEADER - 4) != 0) return cfail(TBK_ERR_FORMAT, "%s: header padding is not zero", path);
    h->k = (int)k;
    h->n = get_le<uint64_t>(b + 16);
    h->reads = get_le<uint64_t>(b + 24);
    h->bases = get_le<uint64_t>(b + 32);
    for (int i = 0; i < 256; i++) h->hist[i] = get_le<uint64_t>(b + 40 + 8 * i);
    const uint64_t body = size - TBK_KMERDB_HEADER;
    if (body % 9 != 0 || body / 9 != h->n)  // (compared by division: 9 * n is never formed from an unchecked n)
        return cfail(TBK_ERR_FORMAT, "%s: %llu bytes after the header do not hold the %llu k-mers it states (9 bytes each)", path, (unsigned long long)body, (unsigned long long)h->n);
    uint64_t kept = 0;
    for (int i = (int)h->floor; i < 256; i++) {
        if (h->hist[i] > h->n) return cfail(TBK_ERR_FORMAT, "%s: histogram row %d exceeds the number of k-mers", path, i);
        kept += h->hist[i];  // (256 terms of at most n < 2^61: no overflow)
    }
    if (h->floor == 1) {  // a full database: every distinct k-mer is an entry
        if (kept != h->n)
            return cfail(TBK_ERR_FORMAT, "%s: histogram rows 1..255 sum to %llu, the full database states %llu k-mers", path, (unsigned long long)kept, (unsigned long long)h->n);
        if (h->hist[0] != h->n)
            return cfail(TBK_ERR_FORMAT, "%s: histogram row 0 (all distinct k-mers) is %llu, the full database states %llu k-mers", path, (unsigned long long)h->hist[0], (unsigned long long)h->n);
        return TBK_OK;
    }
    if (kept != h->n) return cfail(TBK_ERR_FORMAT, "%s: histogram rows 2..255 sum to %llu, the file states %llu k-mers", path, (unsigned long long)kept, (unsigned long long)h->n);
    if (h->hist[0] < h->n || h->hist[0] - h->n < h->hist[1])
        return cfail(TBK_ERR_FORMAT, "%s: histogram row 0 (all distinct k-mers) is below rows 1..255 together", path);
    return TBK_OK;
}

extern "C" int tbk_kmerdb_file_info(const char *path, int *k, uint64_t *n, uint64_t hist[256], uint64_t *reads, uint64_t *bases) {
    if (!path) return cfail(TBK_ERR_INVALID, "path is NULL");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return cfail(TBK_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    KmerdbHeader h;
    const int rc = kmerdb_read_header(fd, path, &h);
    ::close(fd);
    if (rc) return rc;
    if (k) *k = h.k;
    if (n) *n = h.n;
    if (hist) memcpy(hist, h.hist, sizeof h.hist);
    if (reads) *reads = h.reads;
    if (bases) *bases = h.bases;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_file_compressed(const char *path, int *flag) {
    if (!path || !flag) return cfail(TBK_ERR_INVALID, "NULL argument");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return cfail(TBK_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    KmerdbHeader h;
    const int rc = kmerdb_read_header(fd, path, &h);
    ::close(fd);
    if (rc) return rc;
    *flag = h.compressed ? 1 : 0;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_file_floor(const char *path, int *floor) {
    if (!path || !floor) return cfail(TBK_ERR_INVALID, "NULL argument");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return cfail(TBK_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    KmerdbHeader h;
    const int rc = kmerdb_read_header(fd, path, &h);
    ::close(fd);
    if (rc) return rc;
    *floor = (int)h.floor;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_floor(const tbk_kmerdb *db, int *floor) {
    if (!db || !floor) return cfail(TBK_ERR_INVALID, "NULL argument");
    *floor = (int)db->floor;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_compressed(const tbk_kmerdb *db, int *flag) {
    if (!db || !flag) return cfail(TBK_ERR_INVALID, "NULL argument");
    *flag = db->compressed ? 1 : 0;
    return TBK_OK;
}

constexpr uint64_t TBK_KMERDB_PIECE = (uint64_t)1 << 22;  // k-mers per piece of a save or a load

extern "C" int tbk_kmerdb_save(const tbk_kmerdb *db, const char *path) {
    if (!db || !path) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (db->n) {
        const int rc = kmerdb_device(db->device);
        if (rc) return rc;
    }
    uint8_t b[TBK_KMERDB_HEADER];
    memset(b, 0, sizeof b);
    memcpy(b, db->floor == 1 ? (db->compressed ? TBK_KMERDB_MAGIC_FULL_HPC : TBK_KMERDB_MAGIC_FULL) : (db->compressed ? TBK_KMERDB_MAGIC_HPC : TBK_KMERDB_MAGIC), 8);
    put_le<uint32_t>(b + 8, (uint32_t)TBK_KMERDB_HEADER);
    put_le<uint32_t>(b + 12, (uint32_t)db->k);
    put_le<uint64_t>(b + 16, db->n);
    put_le<uint64_t>(b + 24, db->reads_added);
    put_le<uint64_t>(b + 32, db->bases_added);
    for (int i = 0; i < 256; i++) put_le<uint64_t>(b + 40 + 8 * i, db->hist[i]);
    put_le<uint32_t>(b + TBK_KMERDB_HEADER - 8, tbk_crc32_c(0, b, TBK_KMERDB_HEADER - 8));
    const std::string tmp = std::string(path) + ".tmp";
    const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return cfail(TBK_ERR_IO, "cannot create %s: %s", tmp.c_str(), strerror(errno));
    bool ok = write_all(fd, b, sizeof b);
    hipError_t e = hipSuccess;
    std::vector<uint64_t> buf((size_t)std::min(db->n, TBK_KMERDB_PIECE));
    for (uint64_t at = 0; ok && e == hipSuccess && at < db->n; at += TBK_KMERDB_PIECE) {
        const uint64_t m = std::min(TBK_KMERDB_PIECE, db->n - at);
        e = hipMemcpy(buf.data(), db->d_keys + at, m * sizeof(uint64_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) ok = write_all(fd, buf.data(), m * sizeof(uint64_t));
    }
    for (uint64_t at = 0; ok && e == hipSuccess && at < db->n; at += TBK_KMERDB_PIECE) {
        const uint64_t m = std::min(TBK_KMERDB_PIECE, db->n - at);
        e = hipMemcpy(buf.data(), db->d_counts + at, m, hipMemcpyDeviceToHost);
        if (e == hipSuccess) ok = write_all(fd, buf.data(), m);
    }
    const int werr = errno;
    const bool closed = ::close(fd) == 0;
    if (e != hipSuccess || !ok || !closed || ::rename(tmp.c_str(), path) != 0) {
        const int rerr = errno;
        (void)::unlink(tmp.c_str());
        if (e != hipSuccess) return cfail(TBK_ERR_HIP, "tbk_kmerdb_save: %s", hipGetErrorString(e));
        return cfail(TBK_ERR_IO, "cannot write %s: %s", path, strerror(!ok ? werr : rerr));
    }
    return TBK_OK;
}

extern "C" int tbk_kmerdb_load(const char *path, int device, tbk_kmerdb **out) {
    if (!path || !out) return cfail(TBK_ERR_INVALID, "NULL argument");
    *out = nullptr;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return cfail(TBK_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    KmerdbHeader h;
    int rc = kmerdb_read_header(fd, path, &h);
    if (!rc) rc = kmerdb_device(device);
    if (rc) { ::close(fd); return rc; }
    tbk_kmerdb *db = new tbk_kmerdb();
    db->device = device; db->k = h.k; db->n = h.n;
    db->reads_added = h.reads; db->bases_added = h.bases;
    db->compressed = h.compressed;
    db->floor = h.floor;
    memcpy(db->hist, h.hist, sizeof h.hist);
    if (h.n) {
        unsigned long long *d_tally = nullptr, tally[3 + 256];
        bool ok = true;
        hipError_t e = hipMalloc((void **)&db->d_keys, h.n * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&db->d_counts, h.n);
        if (e == hipSuccess) e = hipMalloc((void **)&d_tally, sizeof tally);
        if (e == hipSuccess) e = hipMemset(d_tally, 0, sizeof tally);
        std::vector<uint64_t> buf((size_t)std::min(h.n, TBK_KMERDB_PIECE));
        for (uint64_t at = 0; ok && e == hipSuccess && at < h.n; at += TBK_KMERDB_PIECE) {
            const uint64_t m = std::min(TBK_KMERDB_PIECE, h.n - at);
            ok = read_all(fd, buf.data(), m * sizeof(uint64_t));
            if (ok) e = hipMemcpy(db->d_keys + at, buf.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice);
        }
        for (uint64_t at = 0; ok && e == hipSuccess && at < h.n; at += TBK_KMERDB_PIECE) {
            const uint64_t m = std::min(TBK_KMERDB_PIECE, h.n - at);
            ok = read_all(fd, buf.data(), m);
            if (ok) e = hipMemcpy(db->d_counts + at, buf.data(), m, hipMemcpyHostToDevice);
        }
        // the content is only data so far: one pass tells whether it may be searched and tallied by
        if (ok && e == hipSuccess) e = tbk_launch_kmerdb_check(db->d_keys, db->d_counts, h.n, h.k, h.floor, d_tally, nullptr);
        if (ok && e == hipSuccess) e = hipMemcpy(tally, d_tally, sizeof tally, hipMemcpyDeviceToHost);
        if (d_tally) (void)hipFree(d_tally);
        ::close(fd);
        if (!ok || e != hipSuccess) {
            tbk_kmerdb_destroy(db);
            (void)hipGetLastError();
            if (!ok) return cfail(TBK_ERR_IO, "%s: cannot read the k-mers: %s", path, strerror(errno));
            return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_kmerdb_load (%llu k-mers): %s", (unsigned long long)h.n, hipGetErrorString(e));
        }
        int row = 0;
        for (int i = (int)h.floor; i < 256 && !row; i++)
            if (tally[3 + i] != h.hist[i]) row = i;
        if (tally[0] || tally[1] || tally[2] || row) {
            tbk_kmerdb_destroy(db);
            if (tally[0]) return cfail(TBK_ERR_FORMAT, "%s: the k-mers are not in strictly ascending order (%llu places)", path, tally[0]);
            if (tally[1]) return cfail(TBK_ERR_FORMAT, "%s: %llu k-mers have bits above 2k = %d", path, tally[1], 2 * h.k);
            if (tally[2]) return cfail(TBK_ERR_FORMAT, "%s: %llu counters are below %u", path, tally[2], h.floor);
            return cfail(TBK_ERR_FORMAT, "%s: %llu counters are %d, the header's histogram states %llu", path, tally[3 + row], row, (unsigned long long)h.hist[row]);
        }
    } else {
        ::close(fd);
    }
    *out = db;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_info(const tbk_kmerdb *db, int *k, uint64_t *n, int *device, uint64_t *bytes) {
    if (!db) return cfail(TBK_ERR_INVALID, "database is NULL");
    if (k) *k = db->k;
    if (n) *n = db->n;
    if (device) *device = db->device;
    if (bytes) *bytes = db->n * 9;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_stats(const tbk_kmerdb *db, uint64_t *reads_added, uint64_t *bases_added) {
    if (!db) return cfail(TBK_ERR_INVALID, "database is NULL");
    if (reads_added) *reads_added = db->reads_added;
    if (bases_added) *bases_added = db->bases_added;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_histogram(const tbk_kmerdb *db, uint64_t hist[256]) {
    if (!db || !hist) return cfail(TBK_ERR_INVALID, "NULL argument");
    memcpy(hist, db->hist, sizeof db->hist);
    return TBK_OK;
}

extern "C" int tbk_kmerdb_read(const tbk_kmerdb *db, uint64_t first, uint64_t count, uint64_t *keys, uint8_t *counts) {
    if (!db) return cfail(TBK_ERR_INVALID, "database is NULL");
    if (first > db->n || count > db->n - first)
        return cfail(TBK_ERR_INVALID, "entries %llu + %llu lie outside a database of %llu", (unsigned long long)first, (unsigned long long)count, (unsigned long long)db->n);
    if (!count) return TBK_OK;
    const int rc = kmerdb_device(db->device);
    if (rc) return rc;
    if (keys) CHIP(hipMemcpy(keys, db->d_keys + first, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (counts) CHIP(hipMemcpy(counts, db->d_counts + first, count, hipMemcpyDeviceToHost));
    return TBK_OK;
}

extern "C" int tbk_kmerdb_unique(const tbk_kmerdb *a, const tbk_kmerdb *b, uint32_t min_count, uint32_t max_count, const char *out_path,
                                 uint64_t *n_written) {
    if (!a || !b || !out_path || !n_written) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (a->k != b->k) return cfail(TBK_ERR_INVALID, "the databases have different k (%d and %d)", a->k, b->k);
    if (a->device != b->device) return cfail(TBK_ERR_INVALID, "the databases live on different devices");
    if (kmerdb_same_space(a, b, "the second")) return TBK_ERR_INVALID;
    if (kmerdb_not_full(a, "the first", "tbk_kmerdb_unique") || kmerdb_not_full(b, "the second", "tbk_kmerdb_unique")) return TBK_ERR_INVALID;
    *n_written = 0;
    // upper bound of what can come out: k-mers of A with a counter in range
    uint64_t cap = 0;
    for (uint32_t cnt = std::max<uint32_t>(2, min_count); cnt <= std::min<uint32_t>(255, max_count); cnt++) cap += a->hist[cnt];
    cap = std::min(cap, a->n);
    uint64_t n = 0;
    std::vector<uint64_t> h_keys;
    if (cap) {
        const int rc = kmerdb_device(a->device);
        if (rc) return rc;
        uint64_t *d_out = nullptr, *d_sorted = nullptr;
        unsigned long long *d_n = nullptr, got = 0;
        hipError_t e = hipMalloc((void **)&d_out, cap * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&d_sorted, cap * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&d_n, sizeof got);
        if (e == hipSuccess) e = hipMemset(d_n, 0, sizeof got);
        if (e == hipSuccess) e = tbk_launch_kmerdb_unique(a->d_keys, a->d_counts, a->n, b->d_keys, b->n, min_count, max_count, d_out, cap, d_n, nullptr);
        if (e == hipSuccess) e = hipMemcpy(&got, d_n, sizeof got, hipMemcpyDeviceToHost);
        n = std::min<uint64_t>(got, cap);
        // (waves append in the order they get there: the dump is ordered as tbk_counter_unique orders its own)
        if (e == hipSuccess && n) e = tbk_launch_sort_u64(d_out, d_sorted, n, 2 * a->k, nullptr);
        if (e == hipSuccess && n) {
            h_keys.resize(n);
            e = hipMemcpy(h_keys.data(), d_sorted, n * sizeof(uint64_t), hipMemcpyDeviceToHost);
        }
        if (d_out) (void)hipFree(d_out);
        if (d_sorted) (void)hipFree(d_sorted);
        if (d_n) (void)hipFree(d_n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_kmerdb_unique: %s", hipGetErrorString(e));
        }
    }
    std::string err;
    if (!write_list(out_path, h_keys.data(), n, a->k, err)) return cfail(TBK_ERR_IO, "%s", err.c_str());
    *n_written = n;
    return TBK_OK;
}

// ---- the same subtraction as a k-mer list in HBM -------------------------------------------------------------------------
extern "C" int tbk_table_adopt_device_keys_(uint64_t *, uint64_t, int, int, int, tbk_table **);

// What tbk_kmerdb_unique would write and tbk_table_create_from_file would read back, without the text in between: the
// selection is flagged (one bit per entry of A, one count per tile), the tile counts are scanned, the list's keys are
// allocated at their exact number and the flagged ranks go to their places as packed keys.  Beside the list this takes
// a bit per entry of A and 16 bytes per tile of 1024 entries, freed before it returns.
extern "C" int tbk_kmerdb_unique_table(const tbk_kmerdb *a, const tbk_kmerdb *b, uint32_t min_count, uint32_t max_count, tbk_table **out) {
    if (!a || !b || !out) return cfail(TBK_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (a->k != b->k) return cfail(TBK_ERR_INVALID, "the databases have different k (%d and %d)", a->k, b->k);
    if (a->device != b->device) return cfail(TBK_ERR_INVALID, "the databases live on different devices");
    if (kmerdb_same_space(a, b, "the second")) return TBK_ERR_INVALID;
    if (kmerdb_not_full(a, "the first", "tbk_kmerdb_unique_table") || kmerdb_not_full(b, "the second", "tbk_kmerdb_unique_table")) return TBK_ERR_INVALID;
    // upper bound of what can come out, as in tbk_kmerdb_unique: none in range means nothing to launch
    uint64_t cap = 0;
    for (uint32_t cnt = std::max<uint32_t>(2, min_count); cnt <= std::min<uint32_t>(255, max_count); cnt++) cap += a->hist[cnt];
    cap = std::min(cap, a->n);
    if (!cap) return cfail(TBK_ERR_FORMAT, "empty k-mer list");
    const int rc = kmerdb_device(a->device);
    if (rc) return rc;
    Compaction sel;
    uint64_t *d_keys = nullptr;
    unsigned long long total = 0;
    hipError_t e = sel.reserve(a->n, nullptr);
    if (e == hipSuccess) e = tbk_launch_kmerdb_flag(a->d_keys, a->d_counts, a->n, b->d_keys, b->n, min_count, max_count, sel.d_flags, sel.counts(), nullptr);
    if (e == hipSuccess) e = sel.total(&total);
    const uint64_t n = std::min<uint64_t>(total, cap);  // (never more than the histogram allows: a list is not written past)
    if (e == hipSuccess && n) e = hipMalloc((void **)&d_keys, n * sizeof(uint64_t));
    if (e == hipSuccess && n) e = tbk_launch_kmerdb_scatter(a->d_keys, a->n, sel.d_flags, sel.offsets(), a->k, d_keys, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    sel.release();
    if (e != hipSuccess) {
        if (d_keys) (void)hipFree(d_keys);
        (void)hipGetLastError();
        return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_kmerdb_unique_table (%llu k-mers): %s", (unsigned long long)a->n, hipGetErrorString(e));
    }
    if (total > cap) {
        if (d_keys) (void)hipFree(d_keys);
        return cfail(TBK_ERR_HIP, "tbk_kmerdb_unique_table: %llu k-mers selected, the histogram allows %llu", total, (unsigned long long)cap);
    }
    if (!n) return cfail(TBK_ERR_FORMAT, "empty k-mer list");
    const int made = tbk_table_adopt_device_keys_(d_keys, n, a->k, a->device, 3, out);
    if (made) (void)hipFree(d_keys);
    return made;
}

// ---- three databases: what the child inherited of A's own k-mers --------------------------------------------------------
static int inherited_check(const tbk_kmerdb *a, const tbk_kmerdb *b, const tbk_kmerdb *child) {
    if (a->k != b->k || a->k != child->k)
        return cfail(TBK_ERR_INVALID, "the databases have different k (%d, %d and the child's %d)", a->k, b->k, child->k);
    if (a->device != b->device || a->device != child->device) return cfail(TBK_ERR_INVALID, "the databases live on different devices");
    if (kmerdb_same_space(a, b, "the second") || kmerdb_same_space(a, child, "the child's")) return TBK_ERR_INVALID;
    if (kmerdb_not_full(a, "the first", "tbk_kmerdb_inherited") || kmerdb_not_full(b, "the second", "tbk_kmerdb_inherited") ||
        kmerdb_not_full(child, "the child's", "tbk_kmerdb_inherited"))
        return TBK_ERR_INVALID;
    return TBK_OK;
}

// The k-mers of `a` with a counter in range that `b` lacks and `child` holds with a counter in its range, compacted in
// A's order at their exact number: packed keys (as_keys) or ranks.  *n_out = 0 and *d_out = NULL when none is selected.
// Flag, scan and scatter as in tbk_kmerdb_unique_table, with the same n/8 + n/64 bytes beside the output.
static int inherited_select(const char *who, const tbk_kmerdb *a, const tbk_kmerdb *b, const tbk_kmerdb *child, uint32_t min_count,
                            uint32_t max_count, uint32_t child_min, uint32_t child_max, bool as_keys, uint64_t **d_out, uint64_t *n_out) {
    *d_out = nullptr;
    *n_out = 0;
    // upper bound of what can come out: A's k-mers in range, and no more than the child holds in its own
    uint64_t cap = 0, child_cap = 0;
    for (uint32_t cnt = std::max<uint32_t>(2, min_count); cnt <= std::min<uint32_t>(255, max_count); cnt++) cap += a->hist[cnt];
    for (uint32_t cnt = std::max<uint32_t>(2, child_min); cnt <= std::min<uint32_t>(255, child_max); cnt++) child_cap += child->hist[cnt];
    cap = std::min(std::min(cap, a->n), std::min(child_cap, child->n));
    if (!cap) return TBK_OK;
    const int rc = kmerdb_device(a->device);
    if (rc) return rc;
    Compaction sel;
    uint64_t *d_sel = nullptr;
    unsigned long long total = 0;
    hipError_t e = sel.reserve(a->n, nullptr);
    if (e == hipSuccess)
        e = tbk_launch_kmerdb_inherited_flag(a->d_keys, a->d_counts, a->n, b->d_keys, b->n, child->d_keys, child->d_counts, child->n, min_count,
                                             max_count, child_min, child_max, sel.d_flags, sel.counts(), nullptr);
    if (e == hipSuccess) e = sel.total(&total);
    const uint64_t n = std::min<uint64_t>(total, cap);  // (never more than the histograms allow: nothing is written past)
    if (e == hipSuccess && n) e = hipMalloc((void **)&d_sel, n * sizeof(uint64_t));
    if (e == hipSuccess && n)
        e = as_keys ? tbk_launch_kmerdb_scatter(a->d_keys, a->n, sel.d_flags, sel.offsets(), a->k, d_sel, n, nullptr)
                    : tbk_launch_kmerdb_scatter_ranks(a->d_keys, a->n, sel.d_flags, sel.offsets(), d_sel, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    sel.release();
    if (e != hipSuccess) {
        if (d_sel) (void)hipFree(d_sel);
        (void)hipGetLastError();
        return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "%s (%llu k-mers): %s", who, (unsigned long long)a->n, hipGetErrorString(e));
    }
    if (total > cap) {
        if (d_sel) (void)hipFree(d_sel);
        return cfail(TBK_ERR_HIP, "%s: %llu k-mers selected, the histograms allow %llu", who, total, (unsigned long long)cap);
    }
    *d_out = d_sel;
    *n_out = n;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_inherited(const tbk_kmerdb *a, const tbk_kmerdb *b, const tbk_kmerdb *child, uint32_t min_count, uint32_t max_count,
                                    uint32_t child_min, uint32_t child_max, const char *out_path, uint64_t *n_written) {
    if (!a || !b || !child || !out_path || !n_written) return cfail(TBK_ERR_INVALID, "NULL argument");
    *n_written = 0;
    int rc = inherited_check(a, b, child);
    if (rc) return rc;
    uint64_t *d_ranks = nullptr, n = 0;
    rc = inherited_select("tbk_kmerdb_inherited", a, b, child, min_count, max_count, child_min, child_max, false, &d_ranks, &n);
    if (rc) return rc;
    std::vector<uint64_t> h_keys;
    if (n) {
        // (in A's order already: nothing to sort, and no buffer larger than the list)
        h_keys.resize(n);
        const hipError_t e = hipMemcpy(h_keys.data(), d_ranks, n * sizeof(uint64_t), hipMemcpyDeviceToHost);
        (void)hipFree(d_ranks);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return cfail(TBK_ERR_HIP, "tbk_kmerdb_inherited: %s", hipGetErrorString(e));
        }
    }
    std::string err;
    if (!write_list(out_path, h_keys.data(), n, a->k, err)) return cfail(TBK_ERR_IO, "%s", err.c_str());
    *n_written = n;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_inherited_table(const tbk_kmerdb *a, const tbk_kmerdb *b, const tbk_kmerdb *child, uint32_t min_count,
                                          uint32_t max_count, uint32_t child_min, uint32_t child_max, tbk_table **out) {
    if (out) *out = nullptr;
    if (!a || !b || !child || !out) return cfail(TBK_ERR_INVALID, "NULL argument");
    int rc = inherited_check(a, b, child);
    if (rc) return rc;
    uint64_t *d_keys = nullptr, n = 0;
    rc = inherited_select("tbk_kmerdb_inherited_table", a, b, child, min_count, max_count, child_min, child_max, true, &d_keys, &n);
    if (rc) return rc;
    if (!n) return cfail(TBK_ERR_FORMAT, "empty k-mer list");
    const int made = tbk_table_adopt_device_keys_(d_keys, n, a->k, a->device, 3, out);
    if (made) {
        (void)hipFree(d_keys);
        *out = nullptr;
    }
    return made;
}

// ---- full databases: the union of two, and the way back to the solid form -------------------------------------------------
// db(X) united with db(Y) is db(X ++ Y) when both are full: min(255, min(255, x) + min(255, y)) == min(255, x + y).  A's
// entries are flagged where B holds the same key (one bit per entry of A, one count per tile of A), the tile counts are
// scanned, the output is allocated at n_a + n_b - duplicates and both inputs are scattered to their places (the kernels'
// comment has the rule); the histogram is tallied from the merged counters.  Beside the output: n_a / 8 + n_a / 64 bytes and
// 2 KiB, freed before the call returns.
extern "C" int tbk_kmerdb_union(const tbk_kmerdb *a, const tbk_kmerdb *b, tbk_kmerdb **out) {
    if (out) *out = nullptr;
    if (!a || !b || !out) return cfail(TBK_ERR_INVALID, "NULL argument");
    for (const tbk_kmerdb *d : {a, b})
        if (d->floor != 1)
            return cfail(TBK_ERR_INVALID, "tbk_kmerdb_union: the %s database was kept without the once-seen k-mers and cannot be united exactly "
                                          "(a k-mer seen once in each half is in neither); count with keep_singletons", d == a ? "first" : "second");
    if (a->k != b->k) return cfail(TBK_ERR_INVALID, "the databases have different k (%d and %d)", a->k, b->k);
    if (a->device != b->device) return cfail(TBK_ERR_INVALID, "the databases live on different devices");
    if (kmerdb_same_space(a, b, "the second")) return TBK_ERR_INVALID;
    if (a->n > (UINT64_MAX >> 4) || b->n > (UINT64_MAX >> 4)) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_union: too many k-mers");
    const int rc = kmerdb_device(a->device);
    if (rc) return rc;
    tbk_kmerdb *db = new tbk_kmerdb();
    db->device = a->device; db->k = a->k; db->floor = 1; db->compressed = a->compressed;
    db->reads_added = a->reads_added + b->reads_added;
    db->bases_added = a->bases_added + b->bases_added;
    Compaction both;  // (of A's entries, the ones B holds too)
    unsigned long long *d_hist = nullptr, dups = 0, hist[256];
    memset(hist, 0, sizeof hist);
    hipError_t e = both.reserve(a->n, nullptr);
    if (e == hipSuccess) e = hipMalloc((void **)&d_hist, sizeof hist);
    if (e == hipSuccess) e = hipMemset(d_hist, 0, sizeof hist);
    if (e == hipSuccess) e = tbk_launch_kmerdb_union_flag(a->d_keys, a->n, b->d_keys, b->n, both.d_flags, both.counts(), nullptr);
    if (e == hipSuccess) e = both.total(&dups);
    const bool sane = dups <= a->n && dups <= b->n;  // (nothing is allocated or written by a count that cannot be)
    const uint64_t n = sane ? a->n + b->n - dups : 0;
    if (e == hipSuccess && sane && n) e = hipMalloc((void **)&db->d_keys, n * sizeof(uint64_t));
    if (e == hipSuccess && sane && n) e = hipMalloc((void **)&db->d_counts, n);
    if (e == hipSuccess && sane && n)
        e = tbk_launch_kmerdb_union_scatter(a->d_keys, a->d_counts, a->n, b->d_keys, b->d_counts, b->n, both.d_flags, both.offsets(), db->d_keys,
                                            db->d_counts, n, nullptr);
    if (e == hipSuccess && sane && n) e = tbk_launch_kmerdb_tally(db->d_counts, n, d_hist, nullptr);
    if (e == hipSuccess) e = hipMemcpy(hist, d_hist, sizeof hist, hipMemcpyDeviceToHost);
    both.release();
    if (d_hist) (void)hipFree(d_hist);
    if (e != hipSuccess || !sane) {
        tbk_kmerdb_destroy(db);
        (void)hipGetLastError();
        if (e != hipSuccess)
            return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_kmerdb_union (%llu and %llu k-mers): %s", (unsigned long long)a->n, (unsigned long long)b->n, hipGetErrorString(e));
        return cfail(TBK_ERR_HIP, "tbk_kmerdb_union: %llu k-mers in both of %llu and %llu", dups, (unsigned long long)a->n, (unsigned long long)b->n);
    }
    db->n = n;
    uint64_t tallied = 0;
    for (int i = 1; i < 256; i++) { db->hist[i] = hist[i]; tallied += hist[i]; }
    db->hist[0] = n;
    if (hist[0] || tallied != n) {
        tbk_kmerdb_destroy(db);
        return cfail(TBK_ERR_HIP, "tbk_kmerdb_union: %llu of %llu merged counters tallied, %llu of them 0", (unsigned long long)tallied, (unsigned long long)n, hist[0]);
    }
    *out = db;
    return TBK_OK;
}

// ---- two or three databases held against each other: the joint and the origin spectrum (tbk_compare.hip) ---------------------
// Either floor in any position and nothing but reads of the inputs; beside them the spectrum itself on the device (512 KiB or
// 8 KiB), zeroed, tallied into and copied home.
static int compare_check(const char *who, const tbk_kmerdb *first, const tbk_kmerdb *other, const char *what_other) {
    if (first->k != other->k) return cfail(TBK_ERR_INVALID, "%s: the databases have different k (%d, and %s %d)", who, first->k, what_other, other->k);
    if (first->device != other->device) return cfail(TBK_ERR_INVALID, "%s: the databases live on different devices", who);
    return kmerdb_same_space(first, other, what_other);
}

// runs `launch` on a zeroed device array of `cells` words and copies it to spec
template <typename Launch>
static int compare_run(const char *who, int device, size_t cells, uint64_t *spec, Launch launch) {
    const int rc = kmerdb_device(device);
    if (rc) return rc;
    unsigned long long *d_spec = nullptr;
    hipError_t e = hipMalloc((void **)&d_spec, cells * sizeof *d_spec);
    if (e == hipSuccess) e = hipMemset(d_spec, 0, cells * sizeof *d_spec);
    if (e == hipSuccess) e = launch(d_spec);
    if (e == hipSuccess) e = hipMemcpy(spec, d_spec, cells * sizeof *d_spec, hipMemcpyDeviceToHost);
    if (d_spec) (void)hipFree(d_spec);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    return TBK_OK;
}

extern "C" int tbk_kmerdb_joint_spectrum(const tbk_kmerdb *x, const tbk_kmerdb *y, uint64_t spec[256 * 256]) {
    if (!x || !y || !spec) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_joint_spectrum: NULL argument");
    if (compare_check("tbk_kmerdb_joint_spectrum", x, y, "the second")) return TBK_ERR_INVALID;
    return compare_run("tbk_kmerdb_joint_spectrum", x->device, 256 * 256, spec, [&](unsigned long long *d_spec) {
        return tbk_launch_kmerdb_joint_spectrum(x->d_keys, x->d_counts, x->n, y->d_keys, y->d_counts, y->n, d_spec, nullptr);
    });
}

extern "C" int tbk_kmerdb_origin_spectrum(const tbk_kmerdb *base, const tbk_kmerdb *y, uint32_t y_min, uint32_t y_max, const tbk_kmerdb *z,
                                          uint32_t z_min, uint32_t z_max, uint64_t spec[4 * 256]) {
    if (!base || !y || !z || !spec) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_origin_spectrum: NULL argument");
    if (compare_check("tbk_kmerdb_origin_spectrum", base, y, "the second") || compare_check("tbk_kmerdb_origin_spectrum", base, z, "the third"))
        return TBK_ERR_INVALID;
    if (y_min < 1 || y_min > y_max || y_max > 255 || z_min < 1 || z_min > z_max || z_max > 255)
        return cfail(TBK_ERR_INVALID, "tbk_kmerdb_origin_spectrum: counter ranges [%u, %u] and [%u, %u]: need 1 <= min <= max <= 255", y_min, y_max, z_min, z_max);
    return compare_run("tbk_kmerdb_origin_spectrum", base->device, 4 * 256, spec, [&](unsigned long long *d_spec) {
        return tbk_launch_kmerdb_origin_spectrum(base->d_keys, base->d_counts, base->n, y->d_keys, y->d_counts, y->n, y_min, y_max, z->d_keys,
                                                 z->d_counts, z->n, z_min, z_max, 15u, d_spec, nullptr);
    });
}

// One database by the GC content of its keys (tbk_compare.hip): 33 x 256 words on the device (66 KiB) beside the input.
extern "C" int tbk_kmerdb_gc_spectrum(const tbk_kmerdb *db, uint64_t spec[33 * 256]) {
    if (!db || !spec) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_gc_spectrum: NULL argument");
    return compare_run("tbk_kmerdb_gc_spectrum", db->device, 33 * 256, spec, [&](unsigned long long *d_spec) {
        return tbk_launch_kmerdb_gc_spectrum(db->d_keys, db->d_counts, db->n, db->k, 0, d_spec, nullptr);
    });
}

// (measurement hook, not in tbk.h: tools/measure_union.py makes databases of 1e8 entries where they lie.  Takes over d_keys and
// d_counts - device memory of hipMalloc, freed with the database - once the pass that checks a loaded file has found them in
// order, within 2k bits and at or above the floor; the histogram is that pass's tally, row 0 = n.)
extern "C" int tbk_kmerdb_adopt_device_(uint64_t *d_keys, uint8_t *d_counts, uint64_t n, int k, int device, int floor, tbk_kmerdb **out) {
    if (out) *out = nullptr;
    if (!out || (n && (!d_keys || !d_counts))) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (k < 1 || k > 32 || floor < 1 || floor > 2) return cfail(TBK_ERR_INVALID, "k = %d, floor = %d", k, floor);
    const int rc = kmerdb_device(device);
    if (rc) return rc;
    unsigned long long *d_tally = nullptr, tally[3 + 256];
    memset(tally, 0, sizeof tally);
    hipError_t e = hipMalloc((void **)&d_tally, sizeof tally);
    if (e == hipSuccess) e = hipMemset(d_tally, 0, sizeof tally);
    if (e == hipSuccess) e = tbk_launch_kmerdb_check(d_keys, d_counts, n, k, (uint32_t)floor, d_tally, nullptr);
    if (e == hipSuccess) e = hipMemcpy(tally, d_tally, sizeof tally, hipMemcpyDeviceToHost);
    if (d_tally) (void)hipFree(d_tally);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return cfail(TBK_ERR_HIP, "tbk_kmerdb_adopt_device_: %s", hipGetErrorString(e));
    }
    if (tally[0] || tally[1] || tally[2])
        return cfail(TBK_ERR_FORMAT, "tbk_kmerdb_adopt_device_: %llu places out of order, %llu keys above 2k bits, %llu counters below %d", tally[0], tally[1], tally[2], floor);
    tbk_kmerdb *db = new tbk_kmerdb();
    db->device = device; db->k = k; db->n = n; db->floor = (uint32_t)floor;
    db->d_keys = d_keys; db->d_counts = d_counts;
    for (int i = 1; i < 256; i++) db->hist[i] = tally[3 + i];
    db->hist[0] = n;
    *out = db;
    return TBK_OK;
}

// (for tbk_dump_host.cpp, not in tbk.h: the importer of counted dumps has checked, ordered, folded and tallied its pairs on the
// device itself and states the header; this only makes the object.  Takes over d_keys and d_counts, both NULL when n is 0.)
extern "C" int tbk_kmerdb_make_(uint64_t *d_keys, uint8_t *d_counts, uint64_t n, int k, int device, int floor, int compressed, const uint64_t hist[256],
                                uint64_t reads, uint64_t bases, tbk_kmerdb **out) {
    if (out) *out = nullptr;
    if (!out || !hist || (n && (!d_keys || !d_counts))) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (k < 1 || k > 32 || floor < 1 || floor > 2) return cfail(TBK_ERR_INVALID, "k = %d, floor = %d", k, floor);
    tbk_kmerdb *db = new tbk_kmerdb();
    db->device = device; db->k = k; db->n = n; db->floor = (uint32_t)floor;
    db->compressed = compressed != 0;
    db->d_keys = d_keys; db->d_counts = d_counts;
    db->reads_added = reads; db->bases_added = bases;
    memcpy(db->hist, hist, sizeof db->hist);
    *out = db;
    return TBK_OK;
}

// (for tbk_dump_host.cpp: the arrays a dump selects from, where they lie)
extern "C" int tbk_kmerdb_arrays_(const tbk_kmerdb *db, const uint64_t **d_keys, const uint8_t **d_counts) {
    if (!db || !d_keys || !d_counts) return cfail(TBK_ERR_INVALID, "NULL argument");
    *d_keys = db->d_keys;
    *d_counts = db->d_counts;
    return TBK_OK;
}

// The database the same counter would have left without keep_singletons: the entries with a counter of 2 or more, in their
// places; the header's numbers as they are.  Flag (tbk_kmerdb_flag_kernel with no B and the range 2..255), scan, scatter
// of keys and counters; n / 8 + n / 64 bytes beside the output.
extern "C" int tbk_kmerdb_solid(const tbk_kmerdb *src, tbk_kmerdb **out) {
    if (out) *out = nullptr;
    if (!src || !out) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (src->floor != 1) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_solid: the database is not a full one: it is solid already");
    const int rc = kmerdb_device(src->device);
    if (rc) return rc;
    uint64_t want = 0;
    for (int i = 2; i < 256; i++) want += src->hist[i];
    tbk_kmerdb *db = new tbk_kmerdb();
    db->device = src->device; db->k = src->k; db->floor = 2; db->compressed = src->compressed;
    db->reads_added = src->reads_added; db->bases_added = src->bases_added;
    memcpy(db->hist, src->hist, sizeof src->hist);
    unsigned long long total = 0;
    if (src->n) {
        Compaction sel;
        hipError_t e = sel.reserve(src->n, nullptr);
        if (e == hipSuccess) e = tbk_launch_kmerdb_flag(src->d_keys, src->d_counts, src->n, nullptr, 0, 2, 255, sel.d_flags, sel.counts(), nullptr);
        if (e == hipSuccess) e = sel.total(&total);
        const bool agree = total == want;
        if (e == hipSuccess && agree && want) e = hipMalloc((void **)&db->d_keys, want * sizeof(uint64_t));
        if (e == hipSuccess && agree && want) e = hipMalloc((void **)&db->d_counts, want);
        if (e == hipSuccess && agree && want)
            e = tbk_launch_kmerdb_scatter_pairs(src->d_keys, src->d_counts, src->n, sel.d_flags, sel.offsets(), db->d_keys, db->d_counts, want, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        sel.release();
        if (e != hipSuccess) {
            tbk_kmerdb_destroy(db);
            (void)hipGetLastError();
            return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_kmerdb_solid (%llu k-mers): %s", (unsigned long long)src->n, hipGetErrorString(e));
        }
    }
    if (total != want) {
        tbk_kmerdb_destroy(db);
        return cfail(TBK_ERR_HIP, "tbk_kmerdb_solid: %llu counters of 2 or more, the histogram states %llu", total, (unsigned long long)want);
    }
    db->n = want;
    *out = db;
    return TBK_OK;
}

// ---- a selection that stays a database (tbk_kmerdb_select; kernels: tbk_select.hip) -----------------------------------------
extern "C" void tbk_select_options_init(tbk_select_options *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->size = sizeof *o;
    o->min_count = 1;
    o->max_count = 255;
    o->counter = TBK_SELECT_COUNTER_BASE;
    o->min_gc = 0;
    o->max_gc = 32;
}

static bool select_range_ok(uint32_t lo, uint32_t hi) { return lo >= 1 && lo <= hi && hi <= 255; }

// The entries of base in their range that the partners let pass, as a full database: flag (EXCLUDE partners asked first),
// scan, the output at its exact size, scatter (of base's pairs as they are when no REQUIRE partner's counter goes into the
// result), tally for the header.  Beside the output: n / 8 + n / 64 bytes and the 2 KiB of the tally, freed before the
// call returns.
extern "C" int tbk_kmerdb_select(const tbk_kmerdb *base, const tbk_select_partner *partners, int n_partners, const tbk_select_options *opts,
                                 tbk_kmerdb **out) {
    const char *who = "tbk_kmerdb_select";
    if (out) *out = nullptr;
    if (!base || !opts || !out) return cfail(TBK_ERR_INVALID, "%s: NULL argument", who);
    if (n_partners < 0 || n_partners > 2) return cfail(TBK_ERR_INVALID, "%s: %d partners: 0, 1 or 2 (chain calls for more)", who, n_partners);
    if (n_partners && !partners) return cfail(TBK_ERR_INVALID, "%s: NULL argument", who);
    tbk_select_options o;
    tbk_select_options_init(&o);
    // the struct as it was before the GC bounds ended with `counter` (20 bytes, 24 with its padding): a caller of that size,
    // or of any size that does not reach max_gc, states no GC bound, and what follows `counter` in its memory is not read
    const size_t without_gc = offsetof(tbk_select_options, counter) + sizeof(int), with_gc = offsetof(tbk_select_options, max_gc) + sizeof(uint32_t);
    if (opts->size < without_gc || opts->size > 4096)
        return cfail(TBK_ERR_INVALID, "tbk_select_options.size = %zu: set it with tbk_select_options_init", (size_t)opts->size);
    memcpy(&o, opts, opts->size < with_gc ? without_gc : std::min<size_t>(opts->size, sizeof o));
    if (o.counter != TBK_SELECT_COUNTER_BASE && o.counter != TBK_SELECT_COUNTER_MIN && o.counter != TBK_SELECT_COUNTER_SUM)
        return cfail(TBK_ERR_INVALID, "%s: counter rule %d: TBK_SELECT_COUNTER_BASE, _MIN or _SUM", who, o.counter);
    if (!select_range_ok(o.min_count, o.max_count))
        return cfail(TBK_ERR_INVALID, "%s: counter range [%u, %u] of the base: need 1 <= min <= max <= 255", who, o.min_count, o.max_count);
    if (o.min_gc > o.max_gc || o.max_gc > 32)
        return cfail(TBK_ERR_INVALID, "%s: GC range [%u, %u] of the base, in bases: need 0 <= min <= max <= 32", who, o.min_gc, o.max_gc);
    static const char *const place[2] = {"the first partner's", "the second partner's"};
    for (int i = 0; i < n_partners; i++) {
        const tbk_select_partner &p = partners[i];
        if (!p.db) return cfail(TBK_ERR_INVALID, "%s: NULL argument (%s database)", who, place[i]);
        if (p.mode != TBK_SELECT_REQUIRE && p.mode != TBK_SELECT_EXCLUDE)
            return cfail(TBK_ERR_INVALID, "%s: mode %d of %s database: TBK_SELECT_REQUIRE or TBK_SELECT_EXCLUDE", who, p.mode, place[i]);
        if (!select_range_ok(p.min_count, p.max_count))
            return cfail(TBK_ERR_INVALID, "%s: counter range [%u, %u] of %s database: need 1 <= min <= max <= 255", who, p.min_count, p.max_count, place[i]);
        if (compare_check(who, base, p.db, place[i])) return TBK_ERR_INVALID;
    }
    const int rc = kmerdb_device(base->device);
    if (rc) return rc;
    // EXCLUDE partners first, REQUIRE ones behind them: `ask` in the flag kernel's order, `join` the REQUIRE ones alone
    const TbkSelectPartner none = {nullptr, nullptr, 0, 1, 255, 0};
    TbkSelectPartner ask[2] = {none, none}, join[2] = {none, none};
    int n_ask = 0, n_join = 0;
    for (int mode : {TBK_SELECT_EXCLUDE, TBK_SELECT_REQUIRE})
        for (int i = 0; i < n_partners; i++) {
            const tbk_select_partner &p = partners[i];
            if (p.mode != mode) continue;
            const TbkSelectPartner t = {p.db->d_keys, p.db->d_counts, p.db->n, p.min_count, p.max_count, mode == TBK_SELECT_REQUIRE ? 1u : 0u};
            ask[n_ask++] = t;
            if (mode == TBK_SELECT_REQUIRE) join[n_join++] = t;
        }
    tbk_kmerdb *db = new tbk_kmerdb();
    db->device = base->device; db->k = base->k; db->floor = 1; db->compressed = base->compressed;
    unsigned long long total = 0, hist[256];
    memset(hist, 0, sizeof hist);
    if (base->n) {
        Compaction sel;
        unsigned long long *d_hist = nullptr;
        hipError_t e = sel.reserve(base->n, nullptr);
        if (e == hipSuccess) e = hipMalloc((void **)&d_hist, sizeof hist);
        if (e == hipSuccess) e = hipMemset(d_hist, 0, sizeof hist);
        if (e == hipSuccess)
            e = tbk_launch_kmerdb_select_flag(base->d_keys, base->d_counts, base->n, o.min_count, o.max_count, o.min_gc, o.max_gc, &ask[0], &ask[1],
                                              sel.d_flags, sel.counts(), nullptr);
        if (e == hipSuccess) e = sel.total(&total);
        const bool sane = total <= base->n;  // (nothing is allocated or written by a count that cannot be)
        const bool some = sane && total;
        if (e == hipSuccess && some) e = hipMalloc((void **)&db->d_keys, total * sizeof(uint64_t));
        if (e == hipSuccess && some) e = hipMalloc((void **)&db->d_counts, total);
        if (e == hipSuccess && some) {
            if (o.counter == TBK_SELECT_COUNTER_BASE || !n_join)
                e = tbk_launch_kmerdb_scatter_pairs(base->d_keys, base->d_counts, base->n, sel.d_flags, sel.offsets(), db->d_keys, db->d_counts, total, nullptr);
            else
                e = tbk_launch_kmerdb_select_scatter(o.counter, base->d_keys, base->d_counts, base->n, &join[0], &join[1], sel.d_flags, sel.offsets(),
                                                     db->d_keys, db->d_counts, total, nullptr);
        }
        if (e == hipSuccess && some) e = tbk_launch_kmerdb_tally(db->d_counts, total, d_hist, nullptr);
        if (e == hipSuccess) e = hipMemcpy(hist, d_hist, sizeof hist, hipMemcpyDeviceToHost);
        sel.release();
        if (d_hist) (void)hipFree(d_hist);
        if (e != hipSuccess || !sane) {
            tbk_kmerdb_destroy(db);
            (void)hipGetLastError();
            if (e != hipSuccess)
                return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "%s (%llu k-mers): %s", who, (unsigned long long)base->n, hipGetErrorString(e));
            return cfail(TBK_ERR_HIP, "%s: %llu of %llu k-mers flagged", who, total, (unsigned long long)base->n);
        }
    }
    uint64_t tallied = 0;
    for (int i = 1; i < 256; i++) { db->hist[i] = hist[i]; tallied += hist[i]; }
    db->hist[0] = total;
    db->n = total;
    if (hist[0] || tallied != total) {
        tbk_kmerdb_destroy(db);
        return cfail(TBK_ERR_HIP, "%s: %llu of %llu selected counters tallied, %llu of them 0", who, (unsigned long long)tallied, total, hist[0]);
    }
    *out = db;
    return TBK_OK;
}

// ---- the het-mer pairs of one database (tbk_kmerdb_hetmers; kernels: tbk_hetmer.hip) ---------------------------------------------
static int query_prefix_bits(uint64_t n, int k);  // (the query session's choice of directory, below)

extern "C" void tbk_hetmer_options_init(tbk_hetmer_options *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->size = sizeof *o;
    o->min_count = o->y_min = o->z_min = 1;
    o->max_count = o->y_max = o->z_max = 255;
}

extern "C" void tbk_hetmer_result_init(tbk_hetmer_result *r) {
    if (!r) return;
    memset(r, 0, sizeof *r);
    r->size = sizeof *r;
}

constexpr size_t TBK_HETMER_SUMS = 6 + 16;  // candidates, by partners 0..3, pairs, origin[16] (tbk_launch_hetmer_tally)

// Directory, tally and, for the pairs themselves, flag, scan and scatter at the exact size.  Beside the inputs: the directory,
// the spectrum and the sums on the device, n / 8 + n / 64 bytes and the records when pairs are asked for; all freed before
// the call returns.
extern "C" int tbk_kmerdb_hetmers(const tbk_kmerdb *db, const tbk_hetmer_options *opts, tbk_hetmer_result *result, uint64_t spec[256 * 256],
                                  tbk_hetmer_pair **out_pairs) {
    const char *who = "tbk_kmerdb_hetmers";
    if (out_pairs) *out_pairs = nullptr;
    if (!db || !opts || !result || !spec) return cfail(TBK_ERR_INVALID, "%s: NULL argument", who);
    tbk_hetmer_options o;
    tbk_hetmer_options_init(&o);
    if (opts->size < offsetof(tbk_hetmer_options, want_pairs) + sizeof(int) || opts->size > 4096)
        return cfail(TBK_ERR_INVALID, "tbk_hetmer_options.size = %zu: set it with tbk_hetmer_options_init", (size_t)opts->size);
    memcpy(&o, opts, std::min<size_t>(opts->size, sizeof o));
    if (result->size < sizeof(tbk_hetmer_result) || result->size > 4096)
        return cfail(TBK_ERR_INVALID, "tbk_hetmer_result.size = %zu: set it with tbk_hetmer_result_init", (size_t)result->size);
    if (o.want_pairs && !out_pairs) return cfail(TBK_ERR_INVALID, "%s: pairs are asked for and out_pairs is NULL", who);
    if (!(db->k & 1))
        return cfail(TBK_ERR_INVALID, "%s: k = %d is even: the middle base must be its own mirror under reverse complement, and only an odd k has "
                     "such a position", who, db->k);
    if (!select_range_ok(o.min_count, o.max_count))
        return cfail(TBK_ERR_INVALID, "%s: counter range [%u, %u]: need 1 <= min <= max <= 255", who, o.min_count, o.max_count);
    if (!select_range_ok(o.y_min, o.y_max) || !select_range_ok(o.z_min, o.z_max))
        return cfail(TBK_ERR_INVALID, "%s: counter ranges [%u, %u] and [%u, %u] of the partners: need 1 <= min <= max <= 255", who, o.y_min, o.y_max,
                     o.z_min, o.z_max);
    if (o.y && compare_check(who, db, o.y, "the first partner")) return TBK_ERR_INVALID;
    if (o.z && compare_check(who, db, o.z, "the second partner")) return TBK_ERR_INVALID;
    if (db->n > 0xFFFFFFFFull)
        return cfail(TBK_ERR_INVALID, "%s: the directory holds 32-bit offsets: a database of %llu k-mers (2^32 or more) cannot be searched", who,
                     (unsigned long long)db->n);
    const int rc = kmerdb_device(db->device);
    if (rc) return rc;
    const size_t size = result->size;
    memset(result, 0, sizeof(tbk_hetmer_result));
    result->size = size;
    memset(spec, 0, 256 * 256 * sizeof(uint64_t));
    if (!db->n) return TBK_OK;
    const TbkHetmerPartner y = {o.y ? o.y->d_keys : nullptr, o.y ? o.y->d_counts : nullptr, o.y ? o.y->n : 0, o.y_min, o.y_max};
    const TbkHetmerPartner z = {o.z ? o.z->d_keys : nullptr, o.z ? o.z->d_counts : nullptr, o.z ? o.z->n : 0, o.z_min, o.z_max};
    const int prefix_bits = query_prefix_bits(db->n, db->k);
    uint32_t *d_dir = nullptr;
    unsigned long long *d_sums = nullptr, sums[TBK_HETMER_SUMS], total = 0;  // d_sums: the sums, then the spectrum
    tbk_hetmer_pair *d_pairs = nullptr, *home = nullptr;
    const size_t sums_bytes = TBK_HETMER_SUMS * sizeof(unsigned long long), spec_bytes = 256 * 256 * sizeof(unsigned long long);
    memset(sums, 0, sizeof sums);
    Compaction sel;
    hipError_t e = hipMalloc((void **)&d_dir, (((size_t)1 << prefix_bits) + 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_sums, sums_bytes + spec_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_sums, 0, sums_bytes + spec_bytes, nullptr);
    if (e == hipSuccess && o.want_pairs) e = sel.reserve(db->n, nullptr);
    if (e == hipSuccess) e = tbk_launch_query_directory(db->d_keys, db->n, db->k, prefix_bits, d_dir, nullptr);
    if (e == hipSuccess)
        e = tbk_launch_hetmer_tally(db->d_keys, db->d_counts, db->n, db->k, d_dir, prefix_bits, o.min_count, o.max_count, &y, &z, d_sums,
                                    d_sums + TBK_HETMER_SUMS, nullptr);
    if (e == hipSuccess && o.want_pairs)
        e = tbk_launch_hetmer_flag(db->d_keys, db->d_counts, db->n, db->k, d_dir, prefix_bits, o.min_count, o.max_count, sel.d_flags, sel.counts(), nullptr);
    if (e == hipSuccess && o.want_pairs) e = sel.total(&total);
    const bool sane = total <= db->n / 2;  // (nothing is allocated or written by a count that cannot be)
    const bool some = o.want_pairs && sane && total;
    bool host_nomem = false;
    if (e == hipSuccess && some) e = hipMalloc((void **)&d_pairs, total * sizeof(tbk_hetmer_pair));
    if (e == hipSuccess && some)
        e = tbk_launch_hetmer_scatter(db->d_keys, db->d_counts, db->n, db->k, d_dir, prefix_bits, o.min_count, o.max_count, &y, &z, sel.d_flags,
                                      sel.offsets(), d_pairs, total, nullptr);
    if (e == hipSuccess && some) {
        home = (tbk_hetmer_pair *)tbk_host_alloc(total * sizeof(tbk_hetmer_pair));
        host_nomem = !home;
    }
    if (e == hipSuccess && some && home) e = hipMemcpy(home, d_pairs, total * sizeof(tbk_hetmer_pair), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sums, d_sums, sums_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(spec, d_sums + TBK_HETMER_SUMS, spec_bytes, hipMemcpyDeviceToHost);
    sel.release();
    for (void *p : {(void *)d_dir, (void *)d_sums, (void *)d_pairs})
        if (p) (void)hipFree(p);
    const bool agree = e != hipSuccess || !sane || host_nomem || !o.want_pairs || total == sums[5];
    if (e != hipSuccess || !sane || host_nomem || !agree) {
        tbk_host_free(home);
        (void)hipGetLastError();
        memset(spec, 0, 256 * 256 * sizeof(uint64_t));
        if (host_nomem) return TBK_ERR_NOMEM;  // (tbk_host_alloc has left the reason)
        if (e != hipSuccess)
            return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "%s (%llu k-mers): %s", who, (unsigned long long)db->n, hipGetErrorString(e));
        return cfail(TBK_ERR_HIP, "%s: %llu pairs flagged among %llu k-mers, %llu tallied", who, total, (unsigned long long)db->n, sane ? sums[5] : 0ull);
    }
    result->candidates = sums[0];
    for (int j = 0; j < 4; j++) result->partners[j] = sums[1 + j];
    result->pairs = sums[5];
    for (int j = 0; j < 16; j++) result->origin[j] = sums[6 + j];
    if (out_pairs) *out_pairs = home;
    return TBK_OK;
}

// =====================================================================================================================
// Database query (tbk_kmerdb_query; kernels: tbk_query.hip): the counter the database holds for every window of a
// batch of sequences - per-sequence totals, a histogram, the entries seen, their copies.  include/tbk.h has the rules.
// =====================================================================================================================
// (the launchers of its kernel files - tbk_query.hip, tbk_depth.hip, tbk_repair.hip, tbk_screen.hip, tbk_read_depth.hip, tbk_pieces.hip: tbk_lookup_host.h)
constexpr uint64_t TBK_QUERY_MAX_WINDOWS = 0xFFFFFFFFull;  // window starts of a session: a 32-bit copy counter cannot wrap
constexpr int TBK_QUERY_MAX_PREFIX_BITS = 28;              // a directory of at most 1 GiB + 4 bytes

// a device buffer that only ever grows
struct QueryBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct tbk_kmerdb_query {
    const tbk_kmerdb *db = nullptr;  // borrowed
    int device = 0, k = 0, prefix_bits = 0;
    bool with_copies = false;
    uint64_t wave_slots = 0;  // waves the device holds at once: the grid of the launches that stride over reads or passes
    uint64_t windows = 0;     // window starts added since creation or the last reset
    uint32_t *d_dir = nullptr, *d_seen = nullptr, *d_copies = nullptr;
    unsigned long long *d_sums = nullptr;  // 256 histogram rows, then 2 + 6 x 256 for the per-entry tallies
    void *d_pad = nullptr;                 // one zero entry that stands for the arrays of an empty database
    QueryBuf bases, offsets, sep, clean_bits, found_bits, bytes, totals, counts;
    QueryBuf copy_bytes, saturated_bits, collapsed_bits, expanded_bits, bin_prefix, bins;  // (the copy-number track's own)
    QueryBuf repairs;                                                                      // (the repair candidates' records)
    double repair_ms[2] = {0, 0};  // (tbk_kmerdb_query_repair_times_)
    QueryBuf evidence;                                                                     // (the read evidence's records)
    hipEvent_t evidence_marks[3] = {nullptr, nullptr, nullptr};  // around the evidence's two kernels, made by its first call
    double evidence_ms[2] = {0, 0};                              // (tbk_kmerdb_query_evidence_times_)
    QueryBuf read_depth;                                                                   // (the read depth's records)
    hipEvent_t read_depth_marks[3] = {nullptr, nullptr, nullptr};  // around the read depth's two kernels, made by its first call
    double read_depth_ms[2] = {0, 0};                              // (tbk_kmerdb_query_read_depth_times_)
    QueryBuf side, pieces, kept_pieces, piece_keys;                // (the read pieces' side bitmap, records and per-read keys)
    hipEvent_t pieces_marks[4] = {nullptr, nullptr, nullptr, nullptr};  // around the lookup, the evidence and the piece kernels, made by the first call
    double pieces_ms[3] = {0, 0, 0};                                    // (tbk_kmerdb_query_pieces_times_)
    size_t seen_bytes() const { return (size_t)((db->n + 31) / 32 + 1) * 4; }
    // what the kernels search; an empty database's arrays are the one entry of padding
    TbkDbView view() const {
        return TbkDbView{db->n ? db->d_keys : (const uint64_t *)d_pad, db->n ? db->d_counts : (const uint8_t *)d_pad, d_dir, (uint32_t)db->n, prefix_bits};
    }
};

static int query_reserve(QueryBuf &b, size_t need) {
    need = (need + 255) & ~(size_t)255;
    if (need <= b.cap) return TBK_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const hipError_t e = hipMalloc(&b.p, need);
    if (e != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();
        return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "database query buffer (%zu bytes): %s", need, hipGetErrorString(e));
    }
    b.cap = need;
    return TBK_OK;
}

// P = floor(log2 n) - 1: a mean bucket of 2 to 4 entries; no more bits than a rank has, nor than the directory's cap
static int query_prefix_bits(uint64_t n, int k) {
    int log2n = 0;
    while ((n >> (log2n + 1)) != 0) log2n++;
    return std::max(0, std::min(std::min(log2n - 1, 2 * k), TBK_QUERY_MAX_PREFIX_BITS));
}

extern "C" void tbk_kmerdb_query_destroy(tbk_kmerdb_query *q) {
    if (!q) return;
    if (hipSetDevice(q->device) == hipSuccess) {
        for (void *p : {(void *)q->d_dir, (void *)q->d_seen, (void *)q->d_copies, (void *)q->d_sums, q->d_pad})
            if (p) (void)hipFree(p);
        for (QueryBuf *b : {&q->bases, &q->offsets, &q->sep, &q->clean_bits, &q->found_bits, &q->bytes, &q->totals, &q->counts, &q->copy_bytes,
                            &q->saturated_bits, &q->collapsed_bits, &q->expanded_bits, &q->bin_prefix, &q->bins, &q->repairs, &q->evidence,
                            &q->read_depth, &q->side, &q->pieces, &q->kept_pieces, &q->piece_keys})
            if (b->p) (void)hipFree(b->p);
        for (hipEvent_t mark : q->evidence_marks)
            if (mark) (void)hipEventDestroy(mark);
        for (hipEvent_t mark : q->read_depth_marks)
            if (mark) (void)hipEventDestroy(mark);
        for (hipEvent_t mark : q->pieces_marks)
            if (mark) (void)hipEventDestroy(mark);
    }
    delete q;
}

constexpr size_t TBK_QUERY_SUMS = 256 + 2 + 6 * 256;

extern "C" int tbk_kmerdb_query_reset(tbk_kmerdb_query *q) {
    if (!q) return cfail(TBK_ERR_INVALID, "query is NULL");
    const int rc = kmerdb_device(q->device);
    if (rc) return rc;
    CHIP(hipMemsetAsync(q->d_seen, 0, q->seen_bytes(), nullptr));
    if (q->with_copies) CHIP(hipMemsetAsync(q->d_copies, 0, (size_t)(q->db->n + 1) * 4, nullptr));
    CHIP(hipMemsetAsync(q->d_sums, 0, TBK_QUERY_SUMS * sizeof(unsigned long long), nullptr));
    q->windows = 0;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_query_create(const tbk_kmerdb *db, int copies, tbk_kmerdb_query **out) {
    if (!out) return cfail(TBK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!db) return cfail(TBK_ERR_INVALID, "database is NULL");
    if (db->n > 0xFFFFFFFFull)
        return cfail(TBK_ERR_INVALID, "a query's directory holds 32-bit offsets: a database of %llu k-mers (2^32 or more) cannot be queried", (unsigned long long)db->n);
    int rc = kmerdb_device(db->device);
    if (rc) return rc;
    int cus = 0;
    CHIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, db->device));
    tbk_kmerdb_query *q = new tbk_kmerdb_query();
    q->db = db; q->device = db->device; q->k = db->k;
    q->with_copies = copies != 0;
    q->prefix_bits = query_prefix_bits(db->n, db->k);
    q->wave_slots = (uint64_t)std::max(cus, 1) * 32;  // 4 SIMDs x 8 waves per compute unit
    hipError_t e = hipMalloc((void **)&q->d_dir, (((size_t)1 << q->prefix_bits) + 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&q->d_seen, q->seen_bytes());
    if (e == hipSuccess && q->with_copies) e = hipMalloc((void **)&q->d_copies, (size_t)(db->n + 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&q->d_sums, TBK_QUERY_SUMS * sizeof(unsigned long long));
    if (e == hipSuccess && !db->n) e = hipMalloc(&q->d_pad, 16);
    if (e == hipSuccess && !db->n) e = hipMemsetAsync(q->d_pad, 0, 16, nullptr);
    if (e == hipSuccess && db->n) e = tbk_launch_query_directory(db->d_keys, db->n, db->k, q->prefix_bits, q->d_dir, nullptr);
    if (e == hipSuccess && !db->n) e = hipMemsetAsync(q->d_dir, 0, 2 * 4, nullptr);  // (P = 0: both offsets 0)
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        tbk_kmerdb_query_destroy(q);
        (void)hipGetLastError();
        return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_kmerdb_query_create (%llu k-mers): %s", (unsigned long long)db->n, hipGetErrorString(e));
    }
    rc = tbk_kmerdb_query_reset(q);
    if (rc) { tbk_kmerdb_query_destroy(q); return rc; }
    *out = q;
    return TBK_OK;
}

// (test hook, not in tbk.h: the running total of window starts, so that the cap can be met without 4 G windows)
extern "C" int tbk_kmerdb_query_set_windows_(tbk_kmerdb_query *q, uint64_t windows) {
    if (!q) return cfail(TBK_ERR_INVALID, "query is NULL");
    q->windows = windows;
    return TBK_OK;
}

// (test hook, not in tbk.h: the grid of the launches that stride over passes or reads, so that a small batch takes a
// second trip of their loops)
extern "C" int tbk_kmerdb_query_set_wave_slots_(tbk_kmerdb_query *q, uint64_t wave_slots) {
    if (!q) return cfail(TBK_ERR_INVALID, "query is NULL");
    if (!wave_slots) return cfail(TBK_ERR_INVALID, "wave_slots is 0");
    q->wave_slots = wave_slots;
    return TBK_OK;
}

// the window starts of a batch: every sequence of k bases or more has len - k + 1
static uint64_t query_count_windows(const uint64_t *offsets, uint64_t n_reads, int k) {
    uint64_t windows = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t len = offsets[r + 1] - offsets[r];
        if (len >= (uint64_t)k) windows += len - (uint64_t)k + 1;
    }
    return windows;
}

// What the four calls that look a batch up begin with, on the session's device: the buffers of the batch, of its separated
// stream (one 'N' behind every read: sep_total bytes, `passes` wave passes) and of the two bitmaps every lookup kernel
// leaves, 64 words per pass each; the batch copied in and separated.  All of it in the stream when this returns.
static int query_stage_batch(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint64_t *sep_total_out,
                             uint64_t *passes_out) {
    const uint64_t total = offsets[n_reads], sep_total = total + n_reads, passes = tbk_probe_passes(sep_total);
    int rc;
    if ((rc = query_reserve(q->bases, total + 16)) || (rc = query_reserve(q->offsets, (n_reads + 1) * 8)) || (rc = query_reserve(q->sep, sep_total + 16)) ||
        (rc = query_reserve(q->clean_bits, passes * 64 * 4)) || (rc = query_reserve(q->found_bits, passes * 64 * 4)))
        return rc;
    CHIP(hipMemcpyAsync(q->bases.p, bases, total, hipMemcpyHostToDevice, nullptr));
    CHIP(hipMemcpyAsync(q->offsets.p, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, nullptr));
    CHIP(tbk_launch_separate(q->bases.as<uint8_t>(), q->offsets.as<uint64_t>(), n_reads, q->sep.as<uint8_t>(), nullptr));
    *sep_total_out = sep_total;
    *passes_out = passes;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_query_add(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t min_count,
                                    uint64_t *per_read, uint8_t *counts) {
    if (!q) return cfail(TBK_ERR_INVALID, "query is NULL");
    if (!n_reads) return TBK_OK;
    int rc = tbk_check_offsets_(offsets, n_reads);
    if (rc) return rc;
    const uint64_t total = offsets[n_reads];
    if (total && !bases) return cfail(TBK_ERR_INVALID, "bases is NULL");
    const uint64_t windows = query_count_windows(offsets, n_reads, q->k);
    if (windows > TBK_QUERY_MAX_WINDOWS || q->windows > TBK_QUERY_MAX_WINDOWS - windows)
        return cfail(TBK_ERR_INVALID, "a query session takes at most 2^32 - 1 window starts: %llu so far, %llu in this batch (reset the session, or make another)",
                     (unsigned long long)q->windows, (unsigned long long)windows);
    if (per_read) memset(per_read, 0, n_reads * 2 * sizeof(uint64_t));
    if (counts && total) memset(counts, 0, total);
    if (!windows) return TBK_OK;
    if ((rc = kmerdb_device(q->device))) return rc;
    uint64_t sep_total, passes;
    if ((rc = query_stage_batch(q, bases, offsets, n_reads, &sep_total, &passes)) || (rc = query_reserve(q->totals, n_reads * 2 * 8))) return rc;
    if (counts && ((rc = query_reserve(q->bytes, passes * 2048)) || (rc = query_reserve(q->counts, total)))) return rc;
    CHIP(tbk_launch_query_lookup(q->sep.as<uint8_t>(), sep_total, passes, q->k, q->view(), std::max<uint32_t>(q->db->floor, min_count),
                                 q->clean_bits.as<uint32_t>(), q->found_bits.as<uint32_t>(), counts ? q->bytes.as<uint8_t>() : nullptr, q->d_sums, q->d_seen,
                                 q->with_copies ? q->d_copies : nullptr, q->wave_slots, nullptr));
    q->windows += windows;  // (the launch is in the stream: what follows can only fail to bring the answers home)
    CHIP(tbk_launch_query_totals(q->clean_bits.as<uint32_t>(), q->found_bits.as<uint32_t>(), q->offsets.as<uint64_t>(), n_reads,
                                 q->totals.as<unsigned long long>(), q->wave_slots, nullptr));
    if (counts)
        CHIP(tbk_launch_query_counts(q->bytes.as<uint8_t>(), q->offsets.as<uint64_t>(), n_reads, q->counts.as<uint8_t>(), q->wave_slots, nullptr));
    if (per_read) CHIP(hipMemcpy(per_read, q->totals.p, n_reads * 2 * 8, hipMemcpyDeviceToHost));
    if (counts) CHIP(hipMemcpy(counts, q->counts.p, total, hipMemcpyDeviceToHost));
    if (!per_read && !counts) CHIP(hipStreamSynchronize(nullptr));  // (the caller's arrays are free to go)
    return TBK_OK;
}

extern "C" int tbk_kmerdb_query_histogram(tbk_kmerdb_query *q, uint64_t hist[256]) {
    if (!q || !hist) return cfail(TBK_ERR_INVALID, "NULL argument");
    const int rc = kmerdb_device(q->device);
    if (rc) return rc;
    CHIP(hipMemcpy(hist, q->d_sums, 256 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return TBK_OK;
}

extern "C" int tbk_kmerdb_query_completeness(tbk_kmerdb_query *q, uint32_t min_count, uint32_t max_count, uint64_t *seen, uint64_t *solid) {
    if (!q || !seen || !solid) return cfail(TBK_ERR_INVALID, "NULL argument");
    *seen = *solid = 0;
    const uint32_t ci = std::max<uint32_t>(q->db->floor, min_count), cx = std::min<uint32_t>(255, max_count);
    if (!q->db->n || ci > cx) return TBK_OK;
    const int rc = kmerdb_device(q->device);
    if (rc) return rc;
    unsigned long long *d_out = q->d_sums + 256, got[2] = {0, 0};
    CHIP(hipMemsetAsync(d_out, 0, sizeof got, nullptr));
    CHIP(tbk_launch_query_completeness(q->db->d_counts, q->d_seen, q->db->n, ci, cx, d_out, nullptr));
    CHIP(hipMemcpy(got, d_out, sizeof got, hipMemcpyDeviceToHost));
    *seen = got[0];
    *solid = got[1];
    return TBK_OK;
}

extern "C" int tbk_kmerdb_query_copy_spectrum(tbk_kmerdb_query *q, uint64_t spec[6][256]) {
    if (!q || !spec) return cfail(TBK_ERR_INVALID, "NULL argument");
    if (!q->with_copies) return cfail(TBK_ERR_INVALID, "the query session was made without copies: it keeps no copy spectrum");
    memset(spec, 0, 6 * 256 * sizeof(uint64_t));
    if (!q->db->n) return TBK_OK;
    const int rc = kmerdb_device(q->device);
    if (rc) return rc;
    unsigned long long *d_spec = q->d_sums + 256 + 2;
    CHIP(hipMemsetAsync(d_spec, 0, 6 * 256 * sizeof(unsigned long long), nullptr));
    CHIP(tbk_launch_query_spectrum(q->db->d_counts, q->d_copies, q->db->n, d_spec, nullptr));
    CHIP(hipMemcpy(spec, d_spec, 6 * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return TBK_OK;
}

// The copy-number track (include/tbk.h has the rule; kernels: tbk_depth.hip): the batch is separated and looked up
// again, this time without a write to the session, and reduced per bin.  The lookup's bitmaps and counter bytes reuse the
// buffers of tbk_kmerdb_query_add; the copy bytes, three more bitmaps, the bin prefix and the bins are the call's own.
extern "C" int tbk_kmerdb_query_track(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t window,
                                      uint32_t peak, tbk_depth_bin *bins, uint64_t n_bins) {
    if (!q) return cfail(TBK_ERR_INVALID, "query is NULL");
    if (!q->with_copies) return cfail(TBK_ERR_INVALID, "the query session was made without copies: it has no copy-number track");
    if (!window) return cfail(TBK_ERR_INVALID, "a track's window is 0: need 1 or more window starts per bin");
    if (!peak) return cfail(TBK_ERR_INVALID, "a track's peak is 0: need the one-copy read depth, 1 or more");
    int rc = n_reads ? tbk_check_offsets_(offsets, n_reads) : TBK_OK;
    if (rc) return rc;
    std::vector<uint64_t> prefix(n_reads + 1, 0);
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t len = offsets[r + 1] - offsets[r];
        const uint64_t nw = len >= (uint64_t)q->k ? len - (uint64_t)q->k + 1 : 0;
        prefix[r + 1] = prefix[r] + nw / window + (nw % window != 0);
    }
    if (prefix[n_reads] != n_bins)
        return cfail(TBK_ERR_INVALID, "a track of these %llu sequences at window %u has %llu bins, not %llu", (unsigned long long)n_reads, window,
                     (unsigned long long)prefix[n_reads], (unsigned long long)n_bins);
    if (!n_bins) return TBK_OK;
    if (!bins) return cfail(TBK_ERR_INVALID, "bins is NULL");
    if (!bases) return cfail(TBK_ERR_INVALID, "bases is NULL");
    if ((rc = kmerdb_device(q->device))) return rc;
    uint64_t sep_total, passes;
    if ((rc = query_stage_batch(q, bases, offsets, n_reads, &sep_total, &passes)) || (rc = query_reserve(q->saturated_bits, passes * 64 * 4)) ||
        (rc = query_reserve(q->collapsed_bits, passes * 64 * 4)) || (rc = query_reserve(q->expanded_bits, passes * 64 * 4)) ||
        (rc = query_reserve(q->bytes, passes * 2048)) || (rc = query_reserve(q->copy_bytes, passes * 2048)) ||
        (rc = query_reserve(q->bin_prefix, (n_reads + 1) * 8)) || (rc = query_reserve(q->bins, n_bins * sizeof(tbk_depth_bin))))
        return rc;
    CHIP(hipMemcpy(q->bin_prefix.p, prefix.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice));  // (prefix is pageable and local: a copy that has left it on return)
    CHIP(tbk_launch_depth_lookup(q->sep.as<uint8_t>(), sep_total, passes, q->k, q->view(), q->d_copies, std::min<uint32_t>(peak, 509),
                                 q->clean_bits.as<uint32_t>(), q->found_bits.as<uint32_t>(),
                                 q->saturated_bits.as<uint32_t>(), q->collapsed_bits.as<uint32_t>(), q->expanded_bits.as<uint32_t>(), q->bytes.as<uint8_t>(),
                                 q->copy_bytes.as<uint8_t>(), q->wave_slots, nullptr));
    CHIP(tbk_launch_depth_bins(q->clean_bits.as<uint32_t>(), q->found_bits.as<uint32_t>(), q->saturated_bits.as<uint32_t>(), q->collapsed_bits.as<uint32_t>(),
                               q->expanded_bits.as<uint32_t>(), q->bytes.as<uint8_t>(), q->copy_bytes.as<uint8_t>(), q->offsets.as<uint64_t>(),
                               q->bin_prefix.as<uint64_t>(), n_reads, n_bins, q->k, window, q->bins.as<tbk_depth_bin>(), q->wave_slots, nullptr));
    CHIP(hipMemcpy(bins, q->bins.p, n_bins * sizeof(tbk_depth_bin), hipMemcpyDeviceToHost));
    return TBK_OK;
}

// The repair candidates (include/tbk.h has the rule; kernels: tbk_repair.hip): the batch is separated and looked up
// again without a write to the session, the heads of the broken stretches are compacted into records at their exact
// number, and the repair kernel completes the records in place.  The two bitmaps reuse the buffers of
// tbk_kmerdb_query_add; the compaction's flags are the call's own and freed on return, the records stay with the session.
extern "C" int tbk_kmerdb_query_repairs(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t min_count,
                                        uint32_t min_support, tbk_repair **repairs, uint64_t *n_repairs) {
    if (!q || !repairs || !n_repairs) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_query_repairs: NULL argument");
    if (min_count < 1 || min_count > 255) return cfail(TBK_ERR_INVALID, "repairs: min_count %u: need 1 <= min_count <= 255", min_count);
    if (min_support < 1 || min_support > 32) return cfail(TBK_ERR_INVALID, "repairs: min_support %u: need 1 <= min_support <= 32", min_support);
    *repairs = nullptr;
    *n_repairs = 0;
    if (!n_reads) return TBK_OK;
    int rc = tbk_check_offsets_(offsets, n_reads);
    if (rc) return rc;
    const uint64_t total = offsets[n_reads];
    if (total && !bases) return cfail(TBK_ERR_INVALID, "bases is NULL");
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t len = offsets[r + 1] - offsets[r];
        if (len >= (1ull << 32))
            return cfail(TBK_ERR_INVALID, "repairs: sequence %llu has %llu bases: a record counts a stretch's windows in 32 bits", (unsigned long long)r,
                         (unsigned long long)len);
    }
    const uint64_t windows = query_count_windows(offsets, n_reads, q->k);
    if (!windows) return TBK_OK;
    if ((rc = kmerdb_device(q->device))) return rc;
    const TbkDbView db = q->view();
    const uint32_t m = std::max<uint32_t>(q->db->floor, min_count);
    uint64_t sep_total, passes;
    const auto t0 = std::chrono::steady_clock::now();  // (the buffers are there after the first call: the clock runs over the copy in)
    if ((rc = query_stage_batch(q, bases, offsets, n_reads, &sep_total, &passes))) return rc;
    uint32_t *d_broken = q->found_bits.as<uint32_t>();
    CHIP(tbk_launch_repair_lookup(q->sep.as<uint8_t>(), sep_total, passes, q->k, db, m, q->clean_bits.as<uint32_t>(), d_broken, q->wave_slots, nullptr));
    Compaction sel;
    unsigned long long found = 0;
    hipError_t e = sel.reserve(passes * 2048, nullptr);
    if (e == hipSuccess) e = tbk_launch_repair_heads(d_broken, passes, sel.d_flags, sel.counts(), nullptr);
    if (e == hipSuccess) e = sel.total(&found);
    const auto t1 = std::chrono::steady_clock::now();
    const bool sane = found <= windows;  // (nothing is allocated or written by a count that cannot be)
    tbk_repair *home = nullptr;
    if (e == hipSuccess && sane && found) {
        if ((rc = query_reserve(q->repairs, found * sizeof(tbk_repair)))) return rc;
        e = tbk_launch_repair_stretches(d_broken, passes, q->offsets.as<uint64_t>(), n_reads, sel.d_flags, sel.offsets(), q->repairs.as<tbk_repair>(),
                                        found, nullptr);
        if (e == hipSuccess)
            e = tbk_launch_repair(q->sep.as<uint8_t>(), q->offsets.as<uint64_t>(), q->k, db, m, min_support, q->repairs.as<tbk_repair>(), found,
                                  q->wave_slots, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        q->repair_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        q->repair_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        if (e == hipSuccess && !(home = (tbk_repair *)tbk_host_alloc(found * sizeof(tbk_repair)))) return TBK_ERR_NOMEM;  // (tbk_host_alloc has left the reason)
        if (e == hipSuccess) e = hipMemcpy(home, q->repairs.p, found * sizeof(tbk_repair), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess || !sane) {
        tbk_host_free(home);
        (void)hipGetLastError();
        if (e != hipSuccess)
            return cfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "tbk_kmerdb_query_repairs (%llu bases): %s", (unsigned long long)total,
                         hipGetErrorString(e));
        return cfail(TBK_ERR_HIP, "tbk_kmerdb_query_repairs: %llu stretches among %llu windows", found, (unsigned long long)windows);
    }
    *repairs = home;
    *n_repairs = found;
    return TBK_OK;
}

// (measuring hook, not in tbk.h: the host's clock over the last call that found a stretch - the copy in, the lookup and the
// compaction up to the stretch count, then the records and the repair kernel up to the stream's end; tools/measure_repairs.py)
extern "C" int tbk_kmerdb_query_repair_times_(tbk_kmerdb_query *q, double ms[2]) {
    if (!q || !ms) return cfail(TBK_ERR_INVALID, "NULL argument");
    ms[0] = q->repair_ms[0];
    ms[1] = q->repair_ms[1];
    return TBK_OK;
}

// The read evidence (include/tbk.h has the rule; kernels: tbk_screen.hip): the batch is separated and looked up again
// without a write to the session, and the two bitmaps are reduced to one record per sequence.  The bitmaps reuse the buffers
// of tbk_kmerdb_query_add; the records are the call's own and stay with the session.
extern "C" int tbk_kmerdb_query_evidence(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t min_count,
                                         uint32_t max_count, tbk_read_evidence *out) {
    if (!q) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_query_evidence: query is NULL");
    if (min_count < 1 || min_count > 255) return cfail(TBK_ERR_INVALID, "evidence: min_count %u: need 1 <= min_count <= 255", min_count);
    if (max_count < min_count || max_count > 255)
        return cfail(TBK_ERR_INVALID, "evidence: max_count %u: need min_count (%u) <= max_count <= 255", max_count, min_count);
    if (!n_reads) return TBK_OK;
    if (!out) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_query_evidence: out is NULL");
    int rc = tbk_check_offsets_(offsets, n_reads);
    if (rc) return rc;
    const uint64_t total = offsets[n_reads];
    if (total && !bases) return cfail(TBK_ERR_INVALID, "bases is NULL");
    memset(out, 0, n_reads * sizeof(tbk_read_evidence));
    if (!query_count_windows(offsets, n_reads, q->k)) return TBK_OK;
    if ((rc = kmerdb_device(q->device))) return rc;
    if ((rc = query_reserve(q->evidence, n_reads * sizeof(tbk_read_evidence)))) return rc;
    for (hipEvent_t &mark : q->evidence_marks)
        if (!mark) CHIP(hipEventCreate(&mark));
    uint64_t sep_total, passes;
    if ((rc = query_stage_batch(q, bases, offsets, n_reads, &sep_total, &passes))) return rc;
    CHIP(hipEventRecord(q->evidence_marks[0], nullptr));
    CHIP(tbk_launch_screen_lookup(q->sep.as<uint8_t>(), sep_total, passes, q->k, q->view(), std::max<uint32_t>(q->db->floor, min_count), max_count,
                                  q->clean_bits.as<uint32_t>(), q->found_bits.as<uint32_t>(), q->wave_slots, nullptr));
    CHIP(hipEventRecord(q->evidence_marks[1], nullptr));
    CHIP(tbk_launch_screen_evidence(q->clean_bits.as<uint32_t>(), q->found_bits.as<uint32_t>(), q->offsets.as<uint64_t>(), n_reads, q->k,
                                    q->evidence.as<tbk_read_evidence>(), q->wave_slots, nullptr));
    CHIP(hipEventRecord(q->evidence_marks[2], nullptr));
    CHIP(hipMemcpy(out, q->evidence.p, n_reads * sizeof(tbk_read_evidence), hipMemcpyDeviceToHost));
    float ms[2] = {0, 0};
    CHIP(hipEventElapsedTime(&ms[0], q->evidence_marks[0], q->evidence_marks[1]));
    CHIP(hipEventElapsedTime(&ms[1], q->evidence_marks[1], q->evidence_marks[2]));
    q->evidence_ms[0] = ms[0];
    q->evidence_ms[1] = ms[1];
    return TBK_OK;
}

// (measuring hook, not in tbk.h: the device's clock over the two kernels of the last call that had a window - the lookup pass,
// then the evidence kernel; tools/measure_screen.py)
extern "C" int tbk_kmerdb_query_evidence_times_(tbk_kmerdb_query *q, double ms[2]) {
    if (!q || !ms) return cfail(TBK_ERR_INVALID, "NULL argument");
    ms[0] = q->evidence_ms[0];
    ms[1] = q->evidence_ms[1];
    return TBK_OK;
}

// The read depth (include/tbk.h has the rule; kernels: tbk_read_depth.hip): the batch is separated and looked up again without a
// write to the session, and the clean bitmap and the depth bytes are reduced to one record per sequence.  The bitmap and the
// bytes reuse the buffers of tbk_kmerdb_query_add; the records are the call's own and stay with the session.
extern "C" int tbk_kmerdb_query_read_depth(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t min_count,
                                           tbk_read_depth *out) {
    if (!q) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_query_read_depth: query is NULL");
    if (min_count < 1 || min_count > 255) return cfail(TBK_ERR_INVALID, "read depth: min_count %u: need 1 <= min_count <= 255", min_count);
    if (!n_reads) return TBK_OK;
    if (!out) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_query_read_depth: out is NULL");
    int rc = tbk_check_offsets_(offsets, n_reads);
    if (rc) return rc;
    const uint64_t total = offsets[n_reads];
    if (total && !bases) return cfail(TBK_ERR_INVALID, "bases is NULL");
    for (uint64_t r = 0; r < n_reads; r++)
        if (offsets[r + 1] - offsets[r] >= (uint64_t)q->k + 0xFFFFFFFFull)
            return cfail(TBK_ERR_INVALID, "read depth: sequence %llu has %llu window starts: the per-read kernel counts in 32-bit rows, need fewer than 2^32",
                         (unsigned long long)r, (unsigned long long)(offsets[r + 1] - offsets[r] - (uint64_t)q->k + 1));
    memset(out, 0, n_reads * sizeof(tbk_read_depth));
    if (!query_count_windows(offsets, n_reads, q->k)) return TBK_OK;
    if ((rc = kmerdb_device(q->device))) return rc;
    if ((rc = query_reserve(q->read_depth, n_reads * sizeof(tbk_read_depth)))) return rc;
    for (hipEvent_t &mark : q->read_depth_marks)
        if (!mark) CHIP(hipEventCreate(&mark));
    uint64_t sep_total, passes;
    if ((rc = query_stage_batch(q, bases, offsets, n_reads, &sep_total, &passes)) || (rc = query_reserve(q->bytes, passes * 2048))) return rc;
    CHIP(hipEventRecord(q->read_depth_marks[0], nullptr));
    CHIP(tbk_launch_read_depth_lookup(q->sep.as<uint8_t>(), sep_total, passes, q->k, q->view(), std::max<uint32_t>(q->db->floor, min_count),
                                      q->clean_bits.as<uint32_t>(), q->bytes.as<uint8_t>(), q->wave_slots, nullptr));
    CHIP(hipEventRecord(q->read_depth_marks[1], nullptr));
    CHIP(tbk_launch_read_depth(q->clean_bits.as<uint32_t>(), q->bytes.as<uint8_t>(), q->offsets.as<uint64_t>(), n_reads,
                               q->read_depth.as<tbk_read_depth>(), q->wave_slots, nullptr));
    CHIP(hipEventRecord(q->read_depth_marks[2], nullptr));
    CHIP(hipMemcpy(out, q->read_depth.p, n_reads * sizeof(tbk_read_depth), hipMemcpyDeviceToHost));
    float ms[2] = {0, 0};
    CHIP(hipEventElapsedTime(&ms[0], q->read_depth_marks[0], q->read_depth_marks[1]));
    CHIP(hipEventElapsedTime(&ms[1], q->read_depth_marks[1], q->read_depth_marks[2]));
    q->read_depth_ms[0] = ms[0];
    q->read_depth_ms[1] = ms[1];
    return TBK_OK;
}

// (measuring hook, not in tbk.h: the device's clock over the two kernels of the last call that had a window - the lookup pass,
// then the per-read kernel; tools/measure_read_depth.py)
extern "C" int tbk_kmerdb_query_read_depth_times_(tbk_kmerdb_query *q, double ms[2]) {
    if (!q || !ms) return cfail(TBK_ERR_INVALID, "NULL argument");
    ms[0] = q->read_depth_ms[0];
    ms[1] = q->read_depth_ms[1];
    return TBK_OK;
}

// The read pieces (include/tbk.h has the rule; kernels: tbk_pieces.hip, and tbk_screen.hip for the lookup and the evidence):
// the batch is separated and looked up again without a write to the session; the held bitmap becomes the side bitmap, the
// starts and the ends of its runs are compacted into records at their exact number, and min_length and TBK_PIECES_LONGEST
// filter the records in a third compaction.  The two bitmaps reuse the buffers of tbk_kmerdb_query_add; the compactions' flags
// are the call's own and freed on return; the side bitmap, the records and the keys stay with the session.
extern "C" int tbk_kmerdb_query_pieces(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t min_count,
                                       uint32_t max_count, uint32_t side, uint32_t which, uint64_t min_length, tbk_read_evidence *evidence,
                                       tbk_read_piece **pieces, uint64_t *n_pieces) {
    if (!q || !pieces || !n_pieces) return cfail(TBK_ERR_INVALID, "tbk_kmerdb_query_pieces: NULL argument");
    if (min_count < 1 || min_count > 255) return cfail(TBK_ERR_INVALID, "pieces: min_count %u: need 1 <= min_count <= 255", min_count);
    if (max_count < min_count || max_count > 255)
        return cfail(TBK_ERR_INVALID, "pieces: max_count %u: need min_count (%u) <= max_count <= 255", max_count, min_count);
    if (side > 1) return cfail(TBK_ERR_INVALID, "pieces: side %u: need TBK_PIECES_COVERED (0) or TBK_PIECES_UNCOVERED (1)", side);
    if (which > 1) return cfail(TBK_ERR_INVALID, "pieces: which %u: need TBK_PIECES_ALL (0) or TBK_PIECES_LONGEST (1)", which);
    int rc = n_reads ? tbk_check_offsets_(offsets, n_reads) : TBK_OK;
    if (rc) return rc;
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    if (total && !bases) return cfail(TBK_ERR_INVALID, "bases is NULL");
    for (uint64_t r = 0; r < n_reads; r++)
        if (offsets[r + 1] - offsets[r] >= (1ull << 32))
            return cfail(TBK_ERR_INVALID, "pieces: sequence %llu has %llu bases: a read's longest piece is chosen by 32 bits of length and 32 of position, need fewer than 2^32",
                         (unsigned long long)r, (unsigned long long)(offsets[r + 1] - offsets[r]));
    *pieces = nullptr;
    *n_pieces = 0;
    if (evidence && n_reads) memset(evidence, 0, n_reads * sizeof(tbk_read_evidence));
    if (!total) return TBK_OK;  // (no read, or empty ones only)
    if ((rc = kmerdb_device(q->device))) return rc;
    for (hipEvent_t &mark : q->pieces_marks)
        if (!mark) CHIP(hipEventCreate(&mark));
    uint64_t sep_total, passes;
    if ((rc = query_stage_batch(q, bases, offsets, n_reads, &sep_total, &passes)) || (rc = query_reserve(q->side, passes * 64 * 4)) ||
        (evidence && (rc = query_reserve(q->evidence, n_reads * sizeof(tbk_read_evidence)))))
        return rc;
    const uint32_t *d_held = q->found_bits.as<uint32_t>();
    uint32_t *d_side = q->side.as<uint32_t>();
    CHIP(hipEventRecord(q->pieces_marks[0], nullptr));
    CHIP(tbk_launch_screen_lookup(q->sep.as<uint8_t>(), sep_total, passes, q->k, q->view(), std::max<uint32_t>(q->db->floor, min_count), max_count,
                                  q->clean_bits.as<uint32_t>(), q->found_bits.as<uint32_t>(), q->wave_slots, nullptr));
    CHIP(hipEventRecord(q->pieces_marks[1], nullptr));
    if (evidence)
        CHIP(tbk_launch_screen_evidence(q->clean_bits.as<uint32_t>(), d_held, q->offsets.as<uint64_t>(), n_reads, q->k, q->evidence.as<tbk_read_evidence>(),
                                        q->wave_slots, nullptr));
    CHIP(hipEventRecord(q->pieces_marks[2], nullptr));
    if (side == TBK_PIECES_UNCOVERED) CHIP(hipMemsetAsync(d_side, 0, passes * 64 * 4, nullptr));
    CHIP(tbk_launch_pieces_side(d_held, q->offsets.as<uint64_t>(), n_reads, sep_total, passes, q->k, side == TBK_PIECES_UNCOVERED, d_side, q->wave_slots, nullptr));
    Compaction starts, ends, keep;
    unsigned long long found = 0, found_ends = 0, kept = 0;
    CHIP(starts.reserve(passes * 2048, nullptr));
    CHIP(ends.reserve(passes * 2048, nullptr));
    CHIP(tbk_launch_pieces_flag(d_side, passes, 0, starts.d_flags, starts.counts(), nullptr));
    CHIP(tbk_launch_pieces_flag(d_side, passes, 1, ends.d_flags, ends.counts(), nullptr));
    CHIP(starts.total(&found));
    CHIP(ends.total(&found_ends));
    if (found != found_ends || found > sep_total / 2)  // (nothing is allocated or written by a count that cannot be)
        return cfail(TBK_ERR_HIP, "tbk_kmerdb_query_pieces: %llu starts and %llu ends among %llu positions", found, found_ends, (unsigned long long)sep_total);
    const tbk_read_piece *d_result = nullptr;
    if (found) {
        if ((rc = query_reserve(q->pieces, found * sizeof(tbk_read_piece)))) return rc;
        CHIP(tbk_launch_pieces_ends(passes, ends.d_flags, ends.offsets(), q->pieces.as<tbk_read_piece>(), found, nullptr));
        CHIP(tbk_launch_pieces_starts(passes, q->offsets.as<uint64_t>(), n_reads, starts.d_flags, starts.offsets(), q->pieces.as<tbk_read_piece>(), found,
                                      nullptr));
        d_result = q->pieces.as<tbk_read_piece>();
        kept = found;
    }
    if (found && (min_length > 1 || which == TBK_PIECES_LONGEST)) {
        const unsigned long long *d_keys = nullptr;
        if (which == TBK_PIECES_LONGEST) {
            if ((rc = query_reserve(q->piece_keys, n_reads * 8))) return rc;
            CHIP(hipMemsetAsync(q->piece_keys.p, 0, n_reads * 8, nullptr));
            CHIP(tbk_launch_pieces_best(q->pieces.as<tbk_read_piece>(), found, min_length, q->piece_keys.as<unsigned long long>(), q->wave_slots, nullptr));
            d_keys = q->piece_keys.as<unsigned long long>();
        }
        CHIP(keep.reserve(found, nullptr));
        CHIP(tbk_launch_pieces_keep_flag(q->pieces.as<tbk_read_piece>(), found, min_length, d_keys, keep.d_flags, keep.counts(), nullptr));
        CHIP(keep.total(&kept));
        if (kept > found) return cfail(TBK_ERR_HIP, "tbk_kmerdb_query_pieces: %llu of %llu pieces kept", kept, found);
        if (kept) {
            if ((rc = query_reserve(q->kept_pieces, kept * sizeof(tbk_read_piece)))) return rc;
            CHIP(tbk_launch_pieces_keep(q->pieces.as<tbk_read_piece>(), found, keep.d_flags, keep.offsets(), q->kept_pieces.as<tbk_read_piece>(), kept, nullptr));
        }
        d_result = q->kept_pieces.as<tbk_read_piece>();
    }
    CHIP(hipEventRecord(q->pieces_marks[3], nullptr));
    tbk_read_piece *home = nullptr;
    if (kept) {
        if (!(home = (tbk_read_piece *)tbk_host_alloc(kept * sizeof(tbk_read_piece)))) return TBK_ERR_NOMEM;  // (tbk_host_alloc has left the reason)
        const hipError_t e = hipMemcpy(home, d_result, kept * sizeof(tbk_read_piece), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            tbk_host_free(home);
            (void)hipGetLastError();
            return cfail(TBK_ERR_HIP, "tbk_kmerdb_query_pieces (%llu pieces): %s", kept, hipGetErrorString(e));
        }
    }
    hipError_t e = evidence ? hipMemcpy(evidence, q->evidence.p, n_reads * sizeof(tbk_read_evidence), hipMemcpyDeviceToHost) : hipStreamSynchronize(nullptr);
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipEventElapsedTime(&ms[i], q->pieces_marks[i], q->pieces_marks[i + 1]);
    if (e != hipSuccess) {
        tbk_host_free(home);
        (void)hipGetLastError();
        return cfail(TBK_ERR_HIP, "tbk_kmerdb_query_pieces (%llu bases): %s", (unsigned long long)total, hipGetErrorString(e));
    }
    for (int i = 0; i < 3; i++) q->pieces_ms[i] = ms[i];
    *pieces = home;
    *n_pieces = kept;
    return TBK_OK;
}

// (measuring hook, not in tbk.h: the device's clock over the last call that had a base - the lookup pass, the evidence kernel
// (next to nothing when no evidence was asked for), then everything between the evidence and the last piece kernel, the
// host's waits for the compactions' totals included; tools/measure_pieces.py)
extern "C" int tbk_kmerdb_query_pieces_times_(tbk_kmerdb_query *q, double ms[3]) {
    if (!q || !ms) return cfail(TBK_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 3; i++) ms[i] = q->pieces_ms[i];
    return TBK_OK;
}
