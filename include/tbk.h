/*
 * tbk.h — C-ABI of libtbk_hip.so: the MI355X-native classify-by-kmers hot path.
 *
 * This is the drop-in boundary.  The reference crosses from Python into native code
 * through ctypes (src/trio_binning/kmers.py:30-86) into the symbols of c/kmers.c; every
 * entry point below names the reference interface it replaces.  Plain C types only:
 * pointers, sizes, opaque handles.  No torch types, no C++ in the signatures.
 *
 * Conventions
 *   - Functions returning int return TBK_OK (0) or a negative tbk_status; the message for
 *     the calling thread's last failure is tbk_last_error().
 *   - Handles are opaque, created/destroyed explicitly (the reference leaks its tables:
 *     c/kmers.c:164-172 has no destroy).
 *   - "Host" pointers are ordinary process memory; "device" pointers are HIP device
 *     memory on the handle's device.  The library never keeps a caller pointer after the
 *     call returns, except between tbk_stream_submit and the matching tbk_stream_wait.
 *   - A read batch is `bases` = the reads' ASCII bytes back to back, and
 *     `offsets[n_reads+1]`: read i is bases[offsets[i] .. offsets[i+1]).  No separators,
 *     no terminators.  Counts come back as int32 counts[n_reads][2] = {hapA, hapB}.
 *   - Any byte outside {A,C,G,T} (upper case) invalidates every window that contains it:
 *     such a window scores no hit (the reference is undefined there — c/kmers.c:78-91,279;
 *     its docstring restricts reads to [ACGT], kmers.py:134-135).
 *   - Everything that computes on the GPU fails with TBK_ERR_NO_DEVICE when no MI355X is
 *     visible.  There is no CPU fallback in this library.
 *   - Threading: a tbk_table is read-only after creation and may be shared by threads; a
 *     tbk_classifier (its streams, ticket ring and scratch) belongs to one thread at a time,
 *     like the reference's per-call scratch buffers (c/kmers.c:278-279).  tbk_last_error() is
 *     per thread.  Calls block the calling thread only where stated; the Python bindings
 *     release the GIL for the duration of every call (ctypes), as the reference's do.
 */
#ifndef TBK_H
#define TBK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TBK_ABI_VERSION 1

typedef enum tbk_status {
    TBK_OK = 0,
    TBK_ERR_INVALID = -1,   /* bad argument (k out of 1..32, NULL, mismatched k, ...)       */
    TBK_ERR_IO = -2,        /* file missing / unreadable (Python side raises IOError,       */
                            /*   as kmers.py:117-118 does)                                  */
    TBK_ERR_FORMAT = -3,    /* malformed k-mer list (empty file, first line gives k > 32)    */
    TBK_ERR_NO_DEVICE = -4, /* no usable HIP device                                         */
    TBK_ERR_HIP = -5,       /* a HIP runtime call failed                                    */
    TBK_ERR_NOMEM = -6,
    TBK_ERR_STATE = -7,     /* call sequence error (wait without submit, ...)               */
    TBK_ERR_INTERNAL = -8   /* the library found its own state inconsistent (never the caller's doing) */
} tbk_status;

typedef struct tbk_table tbk_table;           /* one k-mer list resident in HBM           */
typedef struct tbk_classifier tbk_classifier; /* (hapA, hapB) + streams + staging buffers */

/* ---- library ---------------------------------------------------------------------- */
int tbk_abi_version(void);
const char *tbk_last_error(void);
int tbk_device_count(int *count);
/* Short description of device `device` ("gfx950 AMD Instinct MI355X, 256 CUs, 288 GB"). */
int tbk_device_name(int device, char *buf, size_t buflen);
int tbk_device_identity(int device, char *buf, size_t buflen);  /* "<pci bus id> <uuid>" */
/* NUMA placement (pinned, NUMA-local buffers, one feeder thread per GPU; the reference is one thread on one
 * socket, c/kmers.c:270-299).  *node = the host NUMA node the device's PCIe root belongs to
 * (/sys/bus/pci/devices/<bdf>/numa_node), -1 when the kernel does not say.  tbk_numa_bind_to_device restricts the
 * CALLING thread - and the threads it starts afterwards - to that node's CPUs inside its current affinity mask
 * (*cpus = how many; 0 = left alone: unknown node, nothing in common, TBK_NUMA=0); a pipeline's feeder threads do
 * this for their device by themselves (tbk_pipeline_numa reports it), and a one-process-per-GPU launcher calls it
 * once per rank before the library starts its worker threads.  Pinned buffers the thread allocates afterwards are
 * local: hipHostMalloc places host memory on the node nearest to the current device. */
int tbk_device_numa_node(int device, int *node);
int tbk_numa_bind_to_device(int device, int *node, int *cpus);
/* (library-internal, exported for the CPU tests: sysfs lookups under TBK_SYSFS_ROOT, and the binding itself) */
int tbk_numa_node_of_pci_(const char *pci_bus_id);
int tbk_numa_node_cpus_(int node, int *cpus, int cap);
int tbk_numa_bind_thread_(int node);

/* ---- unit-level API kept for parity with the reference's ctypes surface ------------ */
/* Replaces kmer_to_int (c/kmers.c:50-72; bound kmers.py:75-82): base i -> bits 2i..2i+1,
 * A=0 C=1 G=2 T=3, any other byte contributes 0.  Host code. */
uint64_t tbk_kmer_to_int(const char *kmer, unsigned char k);
/* Replaces reverse_complement (c/kmers.c:74-93; bound kmers.py:85-93): out[k-1-i] =
 * complement(in[i]); a non-ACGT byte leaves out[k-1-i] untouched.  Host code. */
void tbk_reverse_complement(const char *kmer_in, char *kmer_out, unsigned char k);

/* ---- k-mer lists ------------------------------------------------------------------- */
/* Replaces create_kmer_hash_set (c/kmers.c:185-229; bound kmers.py:62-64,104-122) with
 * peek_at_file's rules (c/kmers.c:124-146): k = length of the first line as getline()
 * returns it, minus one; every line is one k-mer (duplicates counted, a last line without
 * '\n' counted); each line contributes its first k bytes, verbatim (no canonicalisation).
 * The packed keys are placed in HBM on `device`; tbk_classifier_create hashes two such lists
 * into the paired open-addressing table the probe kernel reads.
 * Where the keys come from, in this order: (1) the binary key cache `<path>.tbk` when it was made from this
 * very file (same size and modification time; a stale or damaged cache is ignored; TBK_LIST_CACHE=0: never
 * read one, TBK_LIST_CACHE=1: write one after parsing the text); (2) the GPU parser, for lists in the shape
 * every tool writes them - each line k bytes and a newline - whose text is staged through pinned memory and
 * packed one line per thread (TBK_LIST_GPU_PARSE=0: off); (3) the general host parser (the reference's getline
 * rules line by line) for anything else.  All three give the same keys.  tbk_table_origin says which it was
 * (0 keys from the caller / the host parser, 1 the GPU parser, 2 the cache, 3 no file at all: two count databases,
 * tbk_kmerdb_unique_table); tbk_table_keys copies the keys out. */
int tbk_table_create_from_file(const char *path, int device, tbk_table **out);
int tbk_table_origin(const tbk_table *t);
/* The list's packed keys where they lie in HBM on the list's device (num_kmers of them; read-only, valid until the list is
 * destroyed): what the full-membership sweep reads. */
const void *tbk_table_device_keys(const tbk_table *t);
int tbk_table_keys(const tbk_table *t, uint64_t *keys, uint64_t capacity);
/* Host-only half of the above: parse the list (all host threads when every line is k bytes +
 * newline, the sequential general parser otherwise) into malloc'd packed keys; free with
 * tbk_list_free. */
int tbk_list_parse_file(const char *path, uint64_t **keys, uint64_t *n, int *k);
void tbk_list_free(uint64_t *keys);
/* Same from already-packed keys (one per list line) in host memory. */
int tbk_table_create_from_keys(const uint64_t *keys, uint64_t n, int k, int device, tbk_table **out);
/* Same, keys already in device memory on `device` (bench generator).  The keys are copied. */
int tbk_table_create_from_device_keys(const void *d_keys, uint64_t n, int k, int device, tbk_table **out);
void tbk_table_destroy(tbk_table *t);
/* Replaces the field read hash_set->num_kmers (kmers.py:157-159): number of list LINES. */
uint64_t tbk_table_num_kmers(const tbk_table *t);
int tbk_table_k(const tbk_table *t);
int tbk_table_device(const tbk_table *t);
/* Bytes of HBM this list holds (keys + its standalone hashed form once built). */
uint64_t tbk_table_bytes(const tbk_table *t);
/* Distinct keys in the list (builds the standalone hashed form on first use). */
int tbk_table_distinct(tbk_table *t, uint64_t *distinct);
/* Membership of raw packed keys (no canonicalisation): out[i] = 1/0.  Host pointers.
 * Builds the standalone hashed form of the list on first use. */
int tbk_table_contains(tbk_table *t, const uint64_t *keys, uint64_t n, uint8_t *out);

/* ---- the hot path ------------------------------------------------------------------- */
/* Replaces count_kmers_in_read (c/kmers.c:270-299; bound kmers.py:66-73,125-154) for one
 * read: `read` is `len` bytes (len < 0: NUL-terminated).  hapA wins when a k-mer is in both
 * lists.  Both lists must have the same k (TBK_ERR_INVALID otherwise; the reference mixes
 * hapA's window length with hapB's packing there, c/kmers.c:251-253,278-290). */
int tbk_count_kmers_in_read(const char *read, int64_t len, const tbk_table *hap_a,
                            const tbk_table *hap_b, int *count_a, int *count_b);
/* The same call on a classifier of the caller's (tbk_count_kmers_in_read keeps one for the last pair of lists it saw).  The
 * reference's driver calls count_kmers_in_read once per read (classify_by_kmers.py:99-102); a call here is one memcpy into
 * pinned memory, ONE kernel launch that reads the read over PCIe, 8 bytes back and one stream synchronisation (reads of up
 * to 8 Mi bases; longer ones go through tbk_classify_batch). */
int tbk_classifier_count_read(tbk_classifier *c, const char *read, int64_t len, int *count_a, int *count_b);

/* Batch path (what the per-read Python loop classify_by_kmers.py:99-102 becomes).  Creating
 * the classifier builds the two open-addressing tables in HBM on the lists' device: 64-bit
 * slots, 8 per bucket per list, hapA's and hapB's bucket i interleaved in one 128-byte line
 * (initialize_hash_set + add_to_hash, c/kmers.c:112-122,160-180).  The lists may be
 * destroyed afterwards. */
int tbk_classifier_create(const tbk_table *hap_a, const tbk_table *hap_b, tbk_classifier **out);
void tbk_classifier_destroy(tbk_classifier *c);
/* How a classifier is built, as arguments (the reference configures itself through argparse alone,
 * classify_by_kmers.py:14-54): nothing under tbk_classifier_create* / tbk_pipeline_create* reads the environment, and two
 * classifiers of one process may be built with different options at the same time.  tbk_options_init writes the defaults;
 * tbk_classifier_create(a, b, out) = tbk_classifier_create_opts(a, b, NULL, out) = the defaults.  No option changes any
 * result (c/kmers.c:245-299: only membership is observable); they pin what the lists would decide, move the decisions'
 * thresholds and size the table.  tbk_options_from_env overlays the TBK_* variables of the process environment
 * (TBK_SHORT, TBK_ENTRY, TBK_ENTRY_WIDE, TBK_FRONT, TBK_MOD_SAMPLING, TBK_SPAN3, TBK_GUESTS, TBK_MINIMIZER_W/_M,
 * TBK_TABLE_LOAD, TBK_ENTRY_LOAD, TBK_WENTRY_LOAD, TBK_SHORT_LOAD, TBK_CLUSTERED, TBK_BEHIND_FRONT, TBK_PLAINLY_CLUSTERED,
 * TBK_ENTRY_MIN_RATIO, TBK_MEMORY_BUDGET, ...): the command-line tools' fallback, called by THEM (the Python bindings do
 * when no options are given) - never by the library's constructors. */
typedef struct tbk_options {
    uint32_t size;            /* sizeof(tbk_options) of the caller (tbk_options_init sets it): the struct may grow */
    /* the layout of the paired table: -1 the lists decide (short keys -> key layout front-first -> entries -> whole lines,
     * csrc/tbk_common.h), 0 never this one, 1 this one whatever the lists look like */
    int32_t short_keys, entries, wide_entries, front;
    int32_t mod_sampling;     /* -1 / 1: mod-sampling picks the bucket; 0: the random minimizer */
    int32_t span3;            /* -1 / 1: narrow entries and short keys rank 3w t-mer positions; 0: 2w */
    int32_t guests;           /* -1 / 1: key layouts keep a full half's surplus in the other half of its line (k < 32); 0: not */
    int32_t minimizer_w;      /* m-mers per span; -1: as many as k leaves room for (6 .. 8); 0: plain hashing of the key */
    int32_t minimizer_m;      /* m-mer length; 0: by k and the lists' size */
    int32_t two_read_kernel;  /* 0: passes that touch two reads go to the multi-read kernel */
    double table_load;        /* key layouts: keys per slot; 0: 0.08, denser only where the memory budget says so */
    double entry_load, wentry_load, short_load;  /* entries per list and bucket (0.5 / wide 0.25), short keys per line (2.3) */
    double clustered, behind_front, plainly_clustered, entry_min_ratio;  /* the policy's thresholds (0.003, 0.05, 0.12, 1.5) */
    uint64_t memory_budget_bytes;  /* what the paired table may take; 0: 60 % of the device's TOTAL memory (the same lists give
                                      the same table whatever else lives on the device) */
    uint64_t table_align;     /* alignment of the table's first byte (0: the allocator's) */
    uint32_t short_line_cap;  /* slots of a line the short-key inserts use (32; tests lower it to fill the overflow table) */
    int32_t probe_max_blocks; /* cap of the multi-read kernel's grid (0: none; tests) */
    int32_t packed_h2d;       /* 1: host batches cross PCIe in the packed transfer format; 0: as ASCII */
    uint64_t slice_bases;     /* an empty ring takes a host batch in slices of at least this many bases (384 Mi) */
    int32_t build_timing;     /* 1: every build of the paired table with its duration, on stderr */
    int32_t force_replica;    /* 1: a further ring on the table's own device gets a full replica (how one GPU runs the replica path) */
    int32_t ring_streams, copy_priority, h2d_streams, zero_copy;  /* experiments of EXPERIMENTS.md (0, 0, 1, 0) */
    int32_t full_keys;        /* the full-key layout (csrc/tbk_common.h "full keys"): -1 the lists decide, 0 never, 1 pinned */
    double full_load;         /* full keys per line of sixteen slots (2.0: 64 bytes of device memory per key) */
    int32_t replica_copy;     /* 0: the other devices of tbk_classifier_create_multi get the lists' keys and build the table themselves, all at
                                 once; 1: they get a copy of the finished table (asynchronous peer copies, one stream per destination) */
    int32_t verify_build;     /* -1: a table built by inserts that MERGE keys (entries, wide entries) is asked for every line of both lists
                                 before it is handed out (c/kmers.c:112-122: every line is stored); 1: every table; 0: none */
} tbk_options;
void tbk_options_init(tbk_options *o);
int tbk_options_from_env(tbk_options *o);
int tbk_classifier_create_opts(const tbk_table *hap_a, const tbk_table *hap_b, const tbk_options *options, tbk_classifier **out);
/* Several devices (the reference's per-read loop, classify_by_kmers.py:99-102, has no
 * cross-read state, so reads shard over devices and the tables are replicated).  The two lists are
 * hashed once, on their own device; out[i] is a classifier on devices[i] holding a copy of the
 * finished paired table (device-to-device copy, xGMI between peers) with its own streams and
 * ticket ring.  A device may appear more than once (two rings on one GPU).  There is no
 * collective and no cross-device traffic after this call: the caller deals batches to the
 * classifiers and writes results in input order (trio_binning_amd.kmers.MultiClassifier does;
 * tickets of one classifier complete in submission order).  On failure nothing is left behind. */
int tbk_classifier_create_multi(const tbk_table *hap_a, const tbk_table *hap_b, const int *devices, int n_devices,
                                tbk_classifier **out /* [n_devices] */);
int tbk_classifier_create_multi_opts(const tbk_table *hap_a, const tbk_table *hap_b, const int *devices, int n_devices,
                                     const tbk_options *options, tbk_classifier **out /* [n_devices] */);
/* One more classifier over a finished classifier's table, on `device`.  On another device the table is replicated
 * (peer access where the devices are peers, hipMemcpyPeer); on src's own device the read-only table is shared - unless
 * src was created with tbk_options.force_replica, which makes a full replica there too through the same calls (how a one-GPU box executes the
 * replica path).  tbk_classifier_table_id: where a classifier's table lies (equal ids = one shared table) and whether
 * it is such a copy. */
int tbk_classifier_replicate(const tbk_classifier *src, int device, tbk_classifier **out);
int tbk_classifier_table_id(const tbk_classifier *c, uint64_t *table_id, int *is_replica);
int tbk_classifier_device(const tbk_classifier *c);
/* Distinct keys stored per list, bucket lines, bytes of HBM the paired table holds. */
int tbk_classifier_stats(const tbk_classifier *c, uint64_t *distinct_a, uint64_t *distinct_b,
                         uint64_t *n_buckets, uint64_t *table_bytes);
/* Lines of hapB's list whose key hapA's list holds too (0 for lists made by find-unique-kmers).
 * hapA is asked first (c/kmers.c:291-294), so such a key can never count for hapB: it is left out
 * of hapB's half of the table (distinct_b above does not include it), the two halves are disjoint
 * and the probe kernel never arbitrates between them.  get_number_kmers_in_set is unaffected. */
int tbk_classifier_shared_keys(const tbk_classifier *c, uint64_t *n_shared);
/* How a key picks its bucket: the minimizer (w m-mers of length m, starting at base
 * span_offset of the k-mer) of the k-mer's central span, or the whole key when w = 0.
 * tbk_options.minimizer_w and .table_load tune it; neither changes any result. */
int tbk_classifier_layout(const tbk_classifier *c, int *minimizer_w, int *minimizer_m, int *span_offset);
/* 0: the span's m-mer with the smallest hash picks the bucket (random minimizer); t > 0: mod-sampling
 * over the span's t-mers (15 % fewer bucket switches between consecutive windows, more arithmetic per
 * window, longer runs of keys per bucket).  The lists decide: the table is built with mod-sampling
 * and, if more than 0.3 % (TBK_CLUSTERED) of the keys found their own half of their home line full
 * - lists that cluster, as real find-unique-kmers output does - built again with the random
 * minimizer and at half the load (0.04 instead of 0.08 keys per slot: such lists are the ones a
 * roomier table helps).  tbk_options.mod_sampling pins the rule, .table_load the load.  No result
 * depends on either. */
int tbk_classifier_sampling_t(const tbk_classifier *c);
/* How many times the table was built (1 or 2, see above) and how many keys found their own half of
 * their home line full in the layout that was kept. */
int tbk_classifier_build_info(const tbk_classifier *c, int *layout_builds, uint64_t *keys_past_half);
/* Layout of the paired table that stands: front = 1 when the probe kernel fetches the first 64 bytes of a
 * line only (the first four slots of each list; csrc/tbk_common.h "front layout"), and how many keys lie
 * behind that front (settled by the deferred walk).  tbk_options.front pins the layout. */
int tbk_classifier_front(const tbk_classifier *c, int *front, uint64_t *keys_behind_front);
/* Entry layout (csrc/tbk_common.h "entry layout"): lists whose keys come in runs of overlapping k-mers - what
 * find-unique-kmers writes (find_unique_kmers.py:200-233): the k windows over every variant - store a run once per
 * sampled m-mer: the m-mer, up to o + w - 1 bases on either side and one bit per window that is in the list, compared
 * under the window's mask (replaces kmer_in_hash_set's compare, c/kmers.c:245-268; membership is the same).
 * entry_layout = 1 when the table that stands is laid out so (2: WIDE entries of 16 bytes, for k-mers whose context
 * does not fit a slot - k = 26 .. 32); entries_a/_b = entries the lists' keys take.  Chosen for clustered lists whose
 * keys merge (>= tbk_options.entry_min_ratio, default 1.5, keys per entry); .entries = 1 / 0 pins it, .wide_entries the
 * wide form, .entry_load / .wentry_load set the entries per list and bucket (defaults 0.5 / 0.25).
 * entry_layout = 3: SHORT KEYS (csrc/tbk_common.h "short keys") - lists whose keys do not merge (uniform k-mers), each key
 * stored as the 32 bits its bucket does not say already, 32 to a line, plus an overflow table of full keys behind the lines
 * (tbk_classifier_stats' table_bytes counts it); entries_a/_b = words the lists' keys take.  Tried first where k (17 .. ~25,
 * m-mers of at most 16 bases) and the table's size allow; tbk_options.short_keys pins it, .short_load sets the keys per line
 * (default 2.3: 56 bytes of device memory per key; 2.6: 49).  Like the entry layouts it leaves out list lines that are not
 * canonical (no window ever asks for them, c/kmers.c:255): distinct_a/_b count the keys stored.
 * entry_layout = 4: FULL KEYS (csrc/tbk_common.h "full keys") - lists that do not merge and do not fit short keys (uniform 26- to
 * 31-mers): 64-bit keys in the same line shape, three keys and the line's summary in the 32-byte front, twelve more behind it;
 * entries_a/_b = slots the lists' keys take.  tbk_options.full_keys pins it, .full_load sets the keys per line (default 2.0). */
int tbk_classifier_entries(const tbk_classifier *c, int *entry_layout, uint64_t *entries_a, uint64_t *entries_b);
/* Random 64-byte reads, a quad of lanes per line as the probe asks for a front, over this table where it lies
 * in HBM: lines per second (a diagnostic: the same table measures up to 15 % differently from one placement in
 * the device's memory to another). */
int tbk_classifier_calibrate(tbk_classifier *c, double *lines_per_sec);
/* The same in the entry kernels' own request shape - one-wave blocks, waves_per_simd (4..8) of them resident per SIMD, two lanes x
 * 16 bytes of a line's first 32, inflight (1..8) lines per pair before any is used - over n_lines random lines of this table: the
 * ceiling bench.py prices the window loop's line rate against (same table, same box, same process). */
int tbk_classifier_calibrate_pairs(tbk_classifier *c, int inflight, int waves_per_simd, uint64_t n_lines, double *lines_per_sec);

/* Synchronous: host batch in, host counts out (pinned staging + H2D + kernel + D2H). */
int tbk_classify_batch(tbk_classifier *c, const uint8_t *bases, const uint64_t *offsets,
                       uint64_t n_reads, int32_t *counts);

/* Streaming: up to tbk_stream_depth() batches in flight; H2D of batch i+1 runs on a side
 * stream while the kernel of batch i runs.  submit returns a ticket; wait blocks until
 * that batch's counts are in `counts` (the pointer given at submit).  Tickets complete in
 * submission order.  `bases`/`offsets`/`counts` must stay valid until wait returns; buffers
 * from tbk_host_alloc are pinned and are copied without an intermediate staging copy. */
int tbk_stream_depth(const tbk_classifier *c);
int tbk_stream_submit(tbk_classifier *c, const uint8_t *bases, const uint64_t *offsets,
                      uint64_t n_reads, int32_t *counts, uint64_t *ticket);
int tbk_stream_wait(tbk_classifier *c, uint64_t ticket);
/* 1 when that ticket's batch is complete (tbk_stream_wait will not block), 0 when not yet, below -1 on error. */
int tbk_stream_query(tbk_classifier *c, uint64_t ticket);
/* The packed transfer format.  ASCII reads cost a byte per base over PCIe (Gen5 x16: ~56 GB/s, a
 * third of what the probe kernel consumes); the kernel's first step on a 16-base chunk is to turn it
 * into a 32-bit word of 2-bit codes (c/kmers.c:50-72's encoding) and a 16-bit not-ACGT mask, and that
 * step can run on the host instead.  A packed batch is
 *     codes[tbk_packed_chunks(total)]     chunk j = stream positions 16j..16j+15, base i at bits 2i..2i+1
 *     exc_chunk[n_exc], exc_mask[n_exc]   the chunks holding a byte outside ACGT, or positions at or
 *                                         past the end of the stream: chunk index and 16-bit mask
 * = 0.25 bytes per base for clean reads.  Counts are identical to the ASCII path's by construction.
 * The library ORs the exceptions into its dense mask array (an index listed twice is harmless) and marks
 * the positions at or past the end of the stream in the last, partial chunk itself, so a caller's own
 * packer, or a batch re-sliced after packing, need not list that tail.  Code bits of masked positions are
 * ignored.
 * tbk_stream_submit itself packs a host batch this way before the copy (all host threads, straight
 * from the caller's memory into pinned staging) unless TBK_PACKED_H2D=0 / tbk_classifier_set_transfer
 * (c, 0); tbk_pack_bases + tbk_stream_submit_packed let a caller pack ahead of time (a reader thread). */
uint64_t tbk_packed_chunks(uint64_t total_bases);
/* TBK_ERR_NOMEM with *n_exc set when exc_capacity is too small (tbk_packed_chunks(total) always suffices). */
int tbk_pack_bases(const uint8_t *bases, uint64_t total_bases, uint32_t *codes, uint32_t *exc_chunk, uint16_t *exc_mask,
                   uint64_t exc_capacity, uint64_t *n_exc);
int tbk_stream_submit_packed(tbk_classifier *c, const uint32_t *codes, const uint32_t *exc_chunk, const uint16_t *exc_mask,
                             uint64_t n_exc, const uint64_t *offsets, uint64_t n_reads, int32_t *counts, uint64_t *ticket);
/* packed != 0: tbk_stream_submit / tbk_classify_batch pack on the host before the copy (default). */
int tbk_classifier_set_transfer(tbk_classifier *c, int packed);
int tbk_classifier_transfer(const tbk_classifier *c);
void *tbk_host_alloc(size_t bytes);  /* pinned host memory (hipHostMalloc) */
void tbk_host_free(void *p);

/* Device-resident form (inputs already in HBM: bench.py's timed region, and callers that
 * produce reads on the GPU).  d_bases must be 16-byte aligned, d_offsets[0] must be 0 and
 * d_offsets[n_reads] must equal total_bases.  Asynchronous on the classifier's compute stream;
 * tbk_classifier_sync waits for it. */
int tbk_classify_device(tbk_classifier *c, const void *d_bases, const void *d_offsets,
                        uint64_t n_reads, uint64_t total_bases, void *d_counts);
int tbk_classifier_sync(tbk_classifier *c);
/* Device-resident batch through the same ticket ring as tbk_stream_submit: the kernel runs
 * on the compute stream and the counts are copied to `counts` (host; pinned memory from
 * tbk_host_alloc avoids a staging copy) behind it; tbk_stream_wait(ticket) returns when
 * they have arrived.  Lets the host bin batch i while the GPU probes batch i+1. */
int tbk_stream_submit_device(tbk_classifier *c, const void *d_bases, const void *d_offsets,
                             uint64_t n_reads, uint64_t total_bases, int32_t *counts, uint64_t *ticket);

/* ---- one handle over several devices ("one host feeder thread + pinned ring + 2-3 streams per
 * device", tables replicated, reads dealt in batches, no collective) ---------------------------------------
 * tbk_pipeline_create hashes the two lists once (tbk_classifier_create_multi), gives every entry of
 * `devices` a replica with its own stream ring and starts one feeder thread per entry.  submit only queues a
 * batch (ASCII, or already in the packed transfer format); the next feeder whose ring has room takes it and
 * does what is left to do on the host - packing an ASCII batch with its share of the host threads, staging,
 * launching copies and kernels - off the caller's thread.  wait(ticket) returns when that batch's counts
 * are in `counts`, whichever device computed them; *device_slot (optional) = index into `devices` of the ring
 * that did.  Tickets may be waited for in any order; the caller's arrays must stay valid until then.  At most
 * tbk_pipeline_depth() + n_devices batches may be submitted and not yet waited for.  A device may be listed
 * several times: several rings on one GPU, which share that device's (read-only) table.  The handle itself may be used from one thread at a time.
 * Replaces the per-read loop of classify_by_kmers.py:99-102 for any number of GPUs of one node. */
typedef struct tbk_pipeline tbk_pipeline;
int tbk_pipeline_create(const tbk_table *a, const tbk_table *b, const int *devices, int n_devices, tbk_pipeline **out);
int tbk_pipeline_create_opts(const tbk_table *a, const tbk_table *b, const int *devices, int n_devices, const tbk_options *options, tbk_pipeline **out);
void tbk_pipeline_destroy(tbk_pipeline *p);
int tbk_pipeline_depth(const tbk_pipeline *p);     /* sum of the rings' depths */
int tbk_pipeline_devices(const tbk_pipeline *p);
int tbk_pipeline_numa(const tbk_pipeline *p, int slot, int *node, int *cpus);  /* ring `slot`: its device's NUMA node (-1 unknown), CPUs its feeder thread is bound to (0: not bound) */
tbk_classifier *tbk_pipeline_classifier(tbk_pipeline *p, int slot);  /* for stats / timing; never submit to it directly */
int tbk_pipeline_submit(tbk_pipeline *p, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int32_t *counts, uint64_t *ticket);
int tbk_pipeline_submit_packed(tbk_pipeline *p, const uint32_t *codes, const uint32_t *exc_chunk, const uint16_t *exc_mask, uint64_t n_exc,
                               const uint64_t *offsets, uint64_t n_reads, int32_t *counts, uint64_t *ticket);
int tbk_pipeline_wait(tbk_pipeline *p, uint64_t ticket, int *device_slot);
int tbk_pipeline_batches(const tbk_pipeline *p, uint64_t *per_slot, int n);  /* batches each ring has taken so far */
/* Testing hook, no GPU needed: the same queue and feeder threads over n_rings rings whose submit / wait are the
 * caller's callbacks (same contract as tbk_stream_submit / tbk_stream_wait; `slot` says which ring asks). */
typedef int (*tbk_pipeline_test_submit_fn)(void *user, int slot, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                                           int32_t *counts, uint64_t *ticket);
typedef int (*tbk_pipeline_test_wait_fn)(void *user, int slot, uint64_t ticket);
int tbk_pipeline_create_test_(int n_rings, int ring_depth, tbk_pipeline_test_submit_fn submit, tbk_pipeline_test_wait_fn wait, void *user,
                              tbk_pipeline **out);

/* The whole read / classify / write loop of classify-by-kmers as native threads (classify_by_kmers.py:80-117):
 * a reader thread (tbk_fastx_next with packing on), the calling thread feeding the pipeline and taking the
 * batches back in input order, a writer thread (tbk_score_and_bin, tbk_bin_writer_write, tbk_format_tsv ->
 * tsv_fd; tsv_fd < 0: no TSV).  out_a/out_b/out_u are the bins' file names as the reference derives them
 * (seq.py:127-134).  batch_bases / batch_reads bound a batch (0: 64 Mbases / unbounded). */
typedef struct tbk_run_stats {
    uint64_t reads, bases, batches;
    double read_s, gpu_wait_s, write_s, total_s;  /* busy seconds of the reader / waiting for tickets / of the writer; wall */
    int32_t gzip_encoder, reserved_;              /* who coded the bins' gzip members: 0 nobody (plain bins), 1 the host, 2 the device */
} tbk_run_stats;
/* gzip_output = 2: BAM bins ("BAM output" below) - the input must be BAM (TBK_ERR_INVALID otherwise), out_a/out_b/out_u name BAM
 * files, and tbk_run_stats.gzip_encoder says who coded their bgzf blocks, as for gzip.
 * gzip_output = 3: haplotag output ("Haplotag output" below) - BAM input again, out_a names the one BAM file, out_b / out_u are ignored. */
int tbk_classify_file(tbk_pipeline *p, const char *reads_path, uint64_t num_kmers_a, uint64_t num_kmers_b, const char *out_a,
                      const char *out_b, const char *out_u, int gzip_output, int gzip_level, int tsv_fd, uint64_t batch_bases,
                      uint64_t batch_reads, tbk_run_stats *stats);

/* HIP-event timing of the probe on the stream it is launched on.  A probe is four kernels: the pass
 * index, the kernels of the passes that touch several reads (more than two; exactly two), and the kernel of the
 * passes inside one read (on long reads nearly all the work: the dominant kernel).  While enabled, every probe of
 * this classifier is bracketed by events - before the first kernel, in front of the last, after the last; read
 * returns the number of probes and their summed duration since enable (total_ms: all kernels; single_ms:
 * the single-read kernel alone), and resets. */
int tbk_kernel_timing_enable(tbk_classifier *c, int on);
int tbk_kernel_timing_read(tbk_classifier *c, uint64_t *launches, double *total_ms);
int tbk_kernel_timing_read2(tbk_classifier *c, uint64_t *launches, double *total_ms, double *single_ms);
/* Passes (2048 window starts each) of the classifier's most recent probe, and how many of them touched more
 * than one read: the two-read and multi-read kernels' share of the work; the rest was the single-read kernel's. */
int tbk_classifier_last_passes(tbk_classifier *c, uint64_t *n_passes, uint64_t *n_multi);

/* Replaces calculate_scaling_factors (classify_by_kmers.py:57-77) and the binning rule
 * (classify_by_kmers.py:104-115): float64, same operation order (1.0*max/n, count*factor,
 * strict > both ways, else 'U').  Host code; bins[i] in {'A','B','U'}. */
int tbk_score_and_bin(const int32_t *counts, uint64_t n_reads, uint64_t num_kmers_a,
                      uint64_t num_kmers_b, double *score_a, double *score_b, char *bins);

/* ---- I/O either side of the path ------------------------------------ */
typedef struct tbk_fastx_reader tbk_fastx_reader; /* FASTA/FASTQ(.gz) record source            */
typedef struct tbk_fastx_batch tbk_fastx_batch;   /* one batch of records in C-ABI batch layout */
typedef struct tbk_bin_writer tbk_bin_writer;     /* the three output bins                      */

/* Replaces open_fastx_read + readfq (seq.py:45-92): gzip chosen by the ".gz" name suffix,
 * universal newlines, and exactly readfq's record rules (name = header up to the first
 * space, every line loses its last character, '+' switches to quality, quality is read until
 * its length reaches the sequence's, a short quality section turns the record into FASTA...). */
int tbk_fastx_open(const char *path, tbk_fastx_reader **out);
void tbk_fastx_close(tbk_fastx_reader *r);
int tbk_fastx_batch_create(tbk_fastx_batch **out);
void tbk_fastx_batch_destroy(tbk_fastx_batch *b);
/* Fill `b` with the next records: stops after the record that reaches max_bases or max_reads
 * (0 = no limit).  An empty batch means end of input.  The sequence bytes of a batch lie back
 * to back in pinned host memory: pass them straight to tbk_stream_submit. */
int tbk_fastx_next(tbk_fastx_reader *r, tbk_fastx_batch *b, uint64_t max_bases, uint64_t max_reads);
/* on != 0: every batch of this reader also carries its bases in the packed transfer format (see
 * tbk_stream_submit_packed), made while the records are copied - the chunk-parallel scan packs each record's
 * 16-base chunks right after copying it - so that the classify stage moves a quarter of the bytes and
 * nobody reads the batch a second time.  tbk_fastx_batch_packed hands the arrays out (*codes = NULL when the
 * batch carries none); they stay valid until the batch is refilled or destroyed. */
int tbk_fastx_set_packing(tbk_fastx_reader *r, int on);
/* BGZF input (bgzip / htslib: independent gzip members of <= 64 KiB, which the reference reads through gzip.open like any .gz,
 * seq.py:86-92) inflated on `device` - csrc/tbk_gdeflate.hip: one wave per block, CRC-32s checked there - instead of on the host's
 * threads.  Before the first read; other inputs are read as before.  tbk_fastx_inflates_on_device: 1 when that is what happens.  The text
 * arrives in windows of pinned memory, four deep; the chunk-parallel scan reads it there, and with tbk_fastx_set_borrowing a batch may
 * leave its records in a window (while two more are free) - it keeps the window, and the inflater's memory, alive until it is refilled
 * or destroyed.  When the pinned memory for two windows cannot be had, the host's threads inflate after all. */
int tbk_fastx_set_device(tbk_fastx_reader *r, int device);
int tbk_fastx_inflates_on_device(const tbk_fastx_reader *r);
/* An ordinary (non-bgzf) gzip file goes to the device as well when TBK_GZIP_INFLATE=gpu is set, the file is mapped and holds
 * TBK_PINFLATE_MIN bytes (default 16 MB) or more: tbk_gzip_inflate_device's passes, window after window, each window's text copied
 * to the parser.  tbk_fastx_gzip_stats: tbk_gzip_inflate_stats's six counts for this reader so far. */
void tbk_fastx_gzip_stats(const tbk_fastx_reader *r, uint64_t out[6]);
int tbk_fastx_batch_packed(const tbk_fastx_batch *b, const uint32_t **codes, const uint32_t **exc_chunk, const uint16_t **exc_mask,
                           uint64_t *n_exc);
/* on != 0 (and packing on): batches taken from a plain FASTQ file by the chunk-parallel scan do not copy their
 * records.  The reader maps its input; such a batch records where each record lies, carries names, offsets,
 * has_qual and the packed form as usual - the bases are packed straight from the mapping - and has no `bases` /
 * `quals` arrays (tbk_fastx_batch_view hands out one zero byte for them).  tbk_bin_writer_write writes the
 * records to their bins from the mapping: the bytes Read.print would write (seq.py:27-31), a record without a
 * header comment and with a bare '+' line as it stands in the input.  Such batches hold a reference to
 * the mapping (it is unmapped with its last holder); a batch that is refilled lets the pages of the mapping its old records lay in go (they stay in
 * the page cache: the 30 GB mapping of a large input is not torn down all at once at the end).  Batches of any other input (gzip, FASTA, irregular records) are copied as always;
 * tbk_fastx_batch_borrowed says which kind a batch is.  The loop of tbk_classify_file turns this on
 * (TBK_BORROW=0 turns it off).  A borrowed batch keeps the mapping alive: it stays readable (and writable to
 * the bins) after tbk_fastx_close of its reader, until it is refilled or destroyed.
 * tbk_fastx_batch_gather copies a batch's sequences (base_off[n_reads] bytes) and qualities (qual_off[n_reads] bytes)
 * into the caller's buffers, back to back, wherever they lie - for a borrowed batch the only way to see them as
 * arrays (either pointer may be NULL; TBK_ERR_INVALID when a buffer is too small). */
int tbk_fastx_set_borrowing(tbk_fastx_reader *r, int on);
int tbk_fastx_batch_borrowed(const tbk_fastx_batch *b);
int tbk_fastx_batch_gather(const tbk_fastx_batch *b, uint8_t *bases, uint64_t bases_cap, uint8_t *quals, uint64_t quals_cap);
/* Borrow the batch's arrays: offsets have n_reads+1 entries; has_qual[i] = 1 when the record
 * was read as FASTQ (readfq's qual is not None). */
int tbk_fastx_batch_view(const tbk_fastx_batch *b, uint64_t *n_reads, const uint8_t **bases,
                         const uint64_t **base_off, const uint8_t **names, const uint64_t **name_off,
                         const uint8_t **quals, const uint64_t **qual_off, const uint8_t **has_qual);
/* Replaces open_outfiles + Read.print (seq.py:27-42,98-136): truncating open of the three
 * files; a record is written as FASTQ when it has a non-empty quality string, else as FASTA;
 * gzip output is a sequence of gzip members deflated by `threads` threads (0 = all cores) at
 * `level` (<0: 6).  Decompressed bytes equal the reference's; the container bytes do not
 * (they never do: gzip stores a timestamp). */
int tbk_bin_writer_open(const char *path_a, const char *path_b, const char *path_u, int gzip_output,
                        int level, int threads, tbk_bin_writer **out);
/* bins[i] in {'A','B','U'} for every record of the batch; records keep input order per bin. */
/* gzip output: code the members on `device` (csrc/tbk_gdeflate.hip: per-block Huffman coding as kernels, the members' CRC-32s summed
 * on the host meanwhile, one writer thread per bin) instead of on the host's threads.  Right after tbk_bin_writer_open.  A no-op for
 * plain output, level 0, TBK_GZIP_ENCODER=cpu / zlib.  tbk_bin_writer_encoder: 1 when the device codes, 0 when the host does.
 * The decompressed bytes are the same either way (seq.py:27-42,132-134). */
int tbk_bin_writer_use_device(tbk_bin_writer *w, int device);
/* The same encoder by itself: n_members pieces of text (back to back in `text`, member_len[i] bytes each) -> as many gzip members,
 * back to back in dst (member_out_len[i] bytes each; *need = bytes used, or needed when cap is too small: TBK_ERR_NOMEM). */
int tbk_gzip_members_device(int device, const char *text, const uint64_t *member_len, uint64_t n_members, char *dst, uint64_t cap,
                            uint64_t *member_out_len, uint64_t *need);
/* The encoder timed by itself (tools/measure_gdeflate.py): `reps` jobs of these members (text in pinned host memory: tbk_host_alloc)
 * through the three-deep ring - *pipelined_s per job, the link included - and one job's kernels between HIP events on their own
 * stream - *kernels_s; *out_bytes = bytes of members a job makes. */
int tbk_gzip_bench_device(int device, const char *text, const uint64_t *member_len, uint64_t n_members, int reps, double *pipelined_s,
                          double *kernels_s, uint64_t *out_bytes);
/* The other direction (csrc/tbk_gdeflate.hip, second half): a bgzf file - the chain of independent <= 64 KiB gzip members that bgzip and
 * htslib write, which the reference reads through gzip.open like any .gz (seq.py:86-92) - inflated on `device`, one wave per block, every
 * block's CRC-32 checked there.  data / size: the file's bytes (or a run of whole blocks); *text_len: bytes of text.  The reader
 * (tbk_fastx_set_device) drives the same inflater four windows deep. */
int tbk_bgzf_inflate_device(int device, const uint8_t *data, uint64_t size, uint8_t *dst, uint64_t cap, uint64_t *text_len);
/* ---- BAM input: unaligned BAM (PacBio HiFi, ONT uBAM) read as FASTQ ------------------------------------------------------------------
 * tbk_fastx_open reads a path that ends in ".bam" as a BAM file: a bgzf stream (its first 18 bytes must be a bgzf block, TBK_ERR_FORMAT
 * otherwise) whose text is
 *     magic "BAM\1", l_text (int32), text[l_text], n_ref (int32), n_ref x { l_name (int32), name[l_name], l_ref (int32) }
 * and then records: block_size (int32: the bytes that follow) and a 32-byte fixed part.  Counted from the block_size field:
 *     +12 l_read_name (u8, counts the NUL)   +16 n_cigar_op (u16)   +18 flag (u16)   +20 l_seq (u32)   +36 read_name
 * then cigar[4 * n_cigar_op], seq[(l_seq + 1) / 2], qual[l_seq] and tags up to block_size.  Everything is little-endian.  Base i is
 * (seq[i >> 1] >> (4 * (1 - (i & 1)))) & 15 - the high nibble first - read through the table "=ACMGRSVTWYHKDBN".  The header and a
 * record may span any number of bgzf blocks; a missing bgzf end-of-file marker is accepted.
 *
 * The text of a record, which the reader's parser then sees in the file's place, is
 *     '@' name '\n' SEQ '\n' '+' '\n' QUAL '\n'        (l_read_name - 1 + 2 * l_seq + 6 bytes)
 * with name = the l_read_name - 1 bytes before the NUL and QUAL[i] = min(qual[i], 93) + 33.  When qual[0] == 0xFF the quality is
 * absent and the record is written as FASTA, '>' name '\n' SEQ '\n': has_qual is 0 and no quality is invented.  With flag & 0x10
 * SEQ is the reverse complement (the complement of the letters in code order is "=TGKCYSBAWRDMHVN") and QUAL is reversed, as samtools
 * fastq writes them.  Records with flag & skip_flags, and records with l_seq == 0, are skipped and counted; the reader's skip_flags
 * are 0x900 (secondary and supplementary: samtools fastq's default).  No /1 or /2 is added and no tag reaches the header.
 *
 * Refused with TBK_ERR_FORMAT and the record's 0-based number in tbk_last_error(), the first bad record in file order:
 *     block_size > TBK_BAM_MAX_RECORD;  block_size < 32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq;  l_read_name < 2;
 *     a name without a NUL at its end;  a name byte outside 0x21..0x7E;  a file that ends inside a record
 * and, without a record number, a file that ends inside the header and a text that does not begin with "BAM\1".
 *
 * With tbk_fastx_set_device the bgzf blocks are inflated and the records turned into text on that device (csrc/tbk_bam.hip), window
 * after window (TBK_BGZF_GPU_WINDOW bytes of the file each); without one, or when the inflater cannot be set up, the host's threads
 * do both.  An error ends the reader: every later call gives it again. */
#define TBK_BAM_MAX_RECORD (1u << 28)
/* The transcoder by itself, on `device`: records / size = a run of whole BAM records in host memory, offsets[n] = where each begins
 * (each must lie wholly within size: TBK_ERR_INVALID otherwise).  The text of the records that are not skipped is written back to back
 * into dst; *text_len = its bytes - also with TBK_ERR_NOMEM, when cap is too small (dst may then be NULL) - and *n_written /
 * *n_skipped count the records.  TBK_ERR_FORMAT names the first refused record's index in tbk_last_error(). */
int tbk_bam_fastq_device(int device, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, uint8_t *dst,
                         uint64_t cap, uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped);
/* The same by the plain C++ of csrc/tbk_bam.h (what the reader runs without a device, on all its threads). */
int tbk_bam_fastq(const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, uint8_t *dst, uint64_t cap,
                  uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped);
/* The kernels timed by themselves (tools/measure_bam.py): the window resident on the device, one warm-up, then `reps` times
 * whole_s[i] = measure, scan, the text's size home and the write kernel (wall clock, the stream idle either side) and write_s[i] = the
 * write kernel alone between HIP events; *text_len: the window's text. */
int tbk_bam_bench_device(int device, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, int reps,
                         double *whole_s, double *write_s, uint64_t *text_len);
/* 1 when the reader's file is read as BAM; out[0] = records seen so far, out[1] = of them skipped. */
int tbk_fastx_bam_counts(const tbk_fastx_reader *r, uint64_t out[2]);
/* The inflater timed by itself (bench.py's `input_bgzf_inflater`): one window of bgzf blocks, `reps` times - *kernels_s per window with the
 * input resident (HIP events around inflate, CRC-32 and check), *ring_s per window through the ring as the reader drives it (staging
 * copy, copy in, kernels, text home; two windows in flight); *text_bytes: a window's text. */
int tbk_bgzf_bench_device(int device, const uint8_t *data, uint64_t size, int reps, double *ring_s, double *kernels_s, uint64_t *text_bytes);
/* Ordinary gzip input - one member or several, any header fields, any block types; what gzip.open reads (seq.py:86-92) and bgzf is
 * not - inflated on `device` in two passes (csrc/tbk_gdeflate.hip, last part; csrc/tbk_gzplan.cpp): the host guesses block starts, one
 * wave per chunk decodes into 16-bit symbols (a byte, or a marker for a byte of the 32 KiB window the chunk does not have), the chunks
 * whose predecessor ended exactly on their start are kept, their windows filled in front to back, the markers resolved, and every
 * member's CRC-32 and ISIZE compared with its trailer.  *text_len: bytes of text - also when dst is NULL or too small (TBK_ERR_NOMEM):
 * ISIZE is only a hint, so the size query inflates.  Damage: TBK_ERR_FORMAT and the host path's message ("inflate: ...").
 * _opts: chunk / window = compressed bytes per chunk / per window, 0 = the default (TBK_GZIP_CHUNK / TBK_GZIP_WINDOW). */
int tbk_gzip_inflate_device(int device, const uint8_t *data, uint64_t size, uint8_t *dst, uint64_t cap, uint64_t *text_len);
int tbk_gzip_inflate_device_opts(int device, const uint8_t *data, uint64_t size, uint8_t *dst, uint64_t cap, uint64_t *text_len, uint64_t chunk,
                                 uint64_t window);
/* The same plan, chain check and loop with the host's own decoder (TbkInflate::run16) in the device's place: no GPU needed. */
int tbk_gzip_inflate_host(const uint8_t *data, uint64_t size, uint8_t *dst, uint64_t cap, uint64_t *text_len, uint64_t chunk, uint64_t window);
/* Of the calling thread's last tbk_gzip_inflate_device / _host: out[0] windows, [1] chunks guessed, [2] chunks accepted, [3] chunks
 * decoded again (cut off behind a wrong guess, a member's end or a full buffer), [4] bytes handed back to the host path, [5] the most
 * chunks accepted in one window. */
void tbk_gzip_inflate_stats(uint64_t out[6]);
/* The inflater timed by itself on a whole file, `reps` times: *kernels_s the kernels' own time per pass over the file (pass_s[0] the
 * marker inflate, pass_s[1] propagate + resolve + CRC-32; HIP events), *ring_s the wall time per pass (pass_s[2] of it: the host's
 * block-start guesses), *text_bytes the file's text.  pass_s may be NULL. */
int tbk_gzip_inflate_bench_device(int device, const uint8_t *data, uint64_t size, int reps, double *ring_s, double *kernels_s, uint64_t *text_bytes,
                                  double pass_s[3]);
/* (tests) The first member of `data` decoded up to the first block header at or past stop_bit by one decoder and from that bit -
 * *boundary_bit - on by a second one that is told nothing but the bit: the text of both, in dst. */
int tbk_inflate_resume_at_bit(const uint8_t *data, uint64_t size, uint64_t stop_bit, uint8_t *dst, uint64_t cap, uint64_t *text_len,
                              uint64_t *boundary_bit);
/* ---- BAM output: BAM bins from BAM input, records kept whole ----------------------------------------------------------------------------
 * With BAM input and BAM output each of the three bins is a BAM file (the reference has no such mode: an extension, opt-in):
 *   header   the input's header bytes verbatim, "BAM\1" through the last reference entry; no @PG line is added;
 *   records  for every read of the TSV its input record verbatim - block_size and all the bytes that follow, tags included, flag
 *            untouched; a reverse-strand record is NOT reverse-complemented here - in the bin the read was sorted into, in input order;
 *   skipped  records the reader skips (flag & 0x900, l_seq == 0) are in no bin, as they are in no FASTQ bin; tbk_fastx_bam_counts counts them;
 *   end      the 28-byte bgzf end-of-file marker;  a bin with no reads is header plus marker.
 * The container is bgzf: every block a gzip member 1f 8b 08 04, mtime 0, xfl 0, os ff, xlen 6, the BC subfield 02 00 and BSIZE = the
 * block's bytes - 1, a raw deflate stream, CRC-32 and ISIZE; at most 65280 bytes of payload and 65536 bytes in all.  The header may
 * span several blocks, records straddle blocks freely.  The decompressed bytes are specified, the container bytes are not.
 *
 * Reader.  tbk_fastx_set_keep_records (before the first read; TBK_ERR_INVALID when the file is not BAM): every batch then carries,
 * beside its text arrays, its reads' records back to back - tbk_fastx_batch_records, rec_off with n_reads + 1 entries; it returns NULL
 * (and sets both to NULL) for a batch that carries none.  A window's chunk of text owns the window's record bytes and where every
 * WRITTEN record lies; a chunk's text is whole records, so the k-th record parsed from it is its k-th written record, and the batch
 * filler takes them in that order.  Each read is checked against its record (name, number of bases), and none may be left over at
 * the end of the input: a difference is TBK_ERR_INTERNAL, never a silent shift.  With the option off nothing more is kept or copied.
 * tbk_fastx_bam_header: the header's bytes (the reader's, valid until it is closed), at the latest once the first batch has been read -
 * called before, it starts the reader's worker and waits for the header.
 *
 * Encoder.  tbk_bgzf_members_device: data[0 .. size) as bgzf blocks of 65280 bytes of payload (the last one shorter), coded on `device`
 * (csrc/tbk_gdeflate.hip in its bgzf mode), no BAM header and no marker; *n_members blocks in *need bytes of dst - TBK_ERR_NOMEM with
 * *need set when cap is short.  hints: a non-decreasing list of offsets into data (duplicates allowed; one beyond size: TBK_ERR_INVALID)
 * where the kind of the bytes changes.  A deflate block ends at the first hint in (8192, 16384] bytes from its start, else at 16384,
 * and always at the member's end; without hints the cuts are fixed.  (Packed seq, qual and tag arrays each want a code of their own,
 * as bases and qualities do in text.)  Each block is coded by itself or stored, so that a member of 8 blocks fits 65536 bytes whatever
 * its bytes are.  tbk_bgzf_members: the same contract and cut rule on the host (tbk_deflate.cpp's coder per block with the stored
 * fallback; zlib under TBK_GZIP_ENCODER=zlib), what the writer runs without a device.  tbk_bgzf_members_bench_device: the bgzf mode
 * timed as tbk_gzip_bench_device times the gzip mode (data in pinned memory).
 *
 * Writer.  tbk_bin_writer_open_bam codes the header into each file at once, on the host.  tbk_bin_writer_write then appends the reads'
 * records (TBK_ERR_STATE for a batch that carries none) and collects four hints per record: start of seq, of qual, of the tags, the
 * record's end.  Pieces are 65280 bytes; tbk_bin_writer_close codes the remainder and writes the marker.  tbk_bin_writer_use_device as
 * for gzip, except that the host's coder stays when the device's cannot be set up (tbk_bin_writer_encoder says which). */
int tbk_fastx_set_keep_records(tbk_fastx_reader *r, int on);
const uint8_t *tbk_fastx_batch_records(const tbk_fastx_batch *b, const uint8_t **records, const uint64_t **rec_off);
int tbk_fastx_bam_header(tbk_fastx_reader *r, const uint8_t **ptr, uint64_t *len);
int tbk_bgzf_members_device(int device, const uint8_t *data, uint64_t size, const uint64_t *hints, uint64_t n_hints, uint8_t *dst, uint64_t cap, uint64_t *need,
                            uint64_t *n_members);
int tbk_bgzf_members(const uint8_t *data, uint64_t size, const uint64_t *hints, uint64_t n_hints, uint8_t *dst, uint64_t cap, uint64_t *need, uint64_t *n_members);
int tbk_bgzf_members_threads_(const uint8_t *data, uint64_t size, const uint64_t *hints, uint64_t n_hints, uint8_t *dst, uint64_t cap, uint64_t *need, uint64_t *n_members,
                              int threads);
int tbk_bgzf_members_bench_device(int device, const uint8_t *data, uint64_t size, const uint64_t *hints, uint64_t n_hints, int reps, double *pipelined_s, double *kernels_s,
                                  uint64_t *out_bytes);
int tbk_bin_writer_open_bam(const char *path_a, const char *path_b, const char *path_u, const uint8_t *header, uint64_t header_len, int level, int threads,
                            tbk_bin_writer **out);
int tbk_bin_writer_encoder(const tbk_bin_writer *w);
int tbk_bin_writer_write(tbk_bin_writer *w, const tbk_fastx_batch *b, const char *bins);
int tbk_bin_writer_close(tbk_bin_writer *w);
/* ---- Haplotag output: one BAM file in input order, every read tagged with its haplotype and counts ----------------------------------
 * With BAM input, ONE BAM file instead of the three bins (the reference has no such mode: an extension, opt-in), in which every read
 * carries its bin as the HP tag and its two k-mer counts as ka / kb.  The rule is normative.
 *
 * Inputs: a record R as the reader keeps it (block_size and the bytes that follow), the bin of its read ('A', 'B' or 'U'; any other
 * byte counts as 'U') and its counts (a, b).  Offsets count from the block_size field.
 *   aux area  begins at 36 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq and ends at 4 + block_size.
 *   walk      field by field, tag[2] type[1] value.  The value's size by type: A c C 1 byte; s S 2; i I f 4; Z H up to and including the
 *             first NUL; B subtype[1] count[int32] count x size, with size 1 for c C, 2 for s S, 4 for i I f.
 *   output    1. block_size' (int32);  2. every byte of R from +4 up to the aux area, verbatim;  3. every field not named HP, ka or kb,
 *             verbatim and in order - a field with one of those three names is dropped, whatever its type;  4. HP C 0x01 for bin A,
 *             HP C 0x02 for bin B, nothing for U;  5. ka I a (uint32);  6. kb I b (uint32).
 * block_size' = block_size - dropped + added: a record grows by at most 18 bytes.  Flag, seq and qual are untouched; a reverse-strand
 * record is not complemented, as in the BAM bins.  All integers are little-endian.
 *
 * Refused with TBK_ERR_FORMAT, tbk_last_error() naming the first offending record in order (the transcoder's atomic-min rule on the
 * device) and the reason.  A record is walked front to back and refused at its first offence; of one field these are looked for in
 * this order:
 *     fewer than 3 bytes left for a field;  unknown type;  for B: fewer than 5 bytes left for subtype and count (a value that runs past
 *     the record's end), unknown subtype, negative count;  Z / H without a NUL before the end;  a value that runs past the record's end;
 *     then, the field being whole: a second field named HP, a second ka, a second kb;
 * and behind the last field block_size' > TBK_BAM_MAX_RECORD.  An aux area that begins past the record's end, and a block_size above
 * TBK_BAM_MAX_RECORD, are refused in the words of "BAM input".  A count below 0 is TBK_ERR_INVALID.
 *
 * The file: the input's header bytes verbatim (no @PG line is added), the tagged record of every read of the TSV in input order -
 * records the reader skips (flag & 0x900, l_seq == 0) are absent, as from the bins - and the 28-byte bgzf end-of-file marker; a run
 * with no reads writes header plus marker.  The container is bgzf as for the BAM bins: the decompressed bytes are specified, the
 * container bytes are not.
 *
 * Rewriter.  tbk_bam_haplotag_device: records / size = a run of whole records in host memory, offsets[n] = where each begins (each
 * must lie wholly within size: TBK_ERR_INVALID otherwise), bins[n], counts[n][2]; the tagged records are written back to back into
 * dst (host memory; size + 18 n bytes always suffice), out_off (n + 1 entries, may be NULL) gets where each begins and the total,
 * *out_len the total - also with TBK_ERR_NOMEM, when cap is too small and nothing is written.  n = 0 is valid and writes nothing.
 * On `device` (csrc/tbk_bam_tag.hip): a measure kernel that walks the fields of a record per thread, the exclusive scan, a write
 * kernel tiled by output bytes.  tbk_bam_haplotag: the same by the plain C++ of csrc/tbk_bam_tag.h on the host's threads.
 * tbk_bam_haplotag_bench_device (tools/measure_haplotag.py): the run resident on the device, one warm-up, then `reps` times
 * whole_s[i] = measure, scan, the size home and the write kernel (wall clock, the stream idle either side), write_s[i] = the write
 * kernel alone between HIP events, call_s[i] (may be NULL) = copy in, kernels and the records home with warm buffers.
 *
 * Writer.  tbk_bin_writer_open_haplotag opens one file and codes the header into it at once, on the host.
 * tbk_bin_writer_write_counts appends a batch: its records (TBK_ERR_STATE for a batch that carries none) are rewritten in one call,
 * and the coder's hints are taken from the tagged records, four per record as for the BAM bins.  Plain tbk_bin_writer_write on such
 * a writer is TBK_ERR_STATE, as tbk_bin_writer_write_counts is on any other.  Pieces are 65280 bytes; tbk_bin_writer_close codes
 * the rest and writes the marker.  tbk_bin_writer_use_device switches the coder to the device, and the rewrite as well when
 * TBK_HAPLOTAG_REWRITE=gpu is set (the default is the host's threads: DESIGN.md section 9 has the measurement); the host functions
 * stay in place when the device cannot be set up.  tbk_bin_writer_rewriter: 1 when the device rewrites.
 *
 * Loop.  tbk_classify_file with gzip_output = 3: out_a names the file, out_b and out_u are ignored (may be NULL); the input must be
 * BAM (TBK_ERR_INVALID otherwise); the reader keeps records as for mode 2. */
int tbk_bam_haplotag_device(int device, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts,
                            uint8_t *dst, uint64_t cap, uint64_t *out_off, uint64_t *out_len);
int tbk_bam_haplotag(const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts, uint8_t *dst, uint64_t cap,
                     uint64_t *out_off, uint64_t *out_len);
int tbk_bam_haplotag_bench_device(int device, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts,
                                  int reps, double *whole_s, double *write_s, double *call_s, uint64_t *out_len);
int tbk_bin_writer_open_haplotag(const char *path, const uint8_t *header, uint64_t header_len, int level, int threads, tbk_bin_writer **out);
int tbk_bin_writer_write_counts(tbk_bin_writer *w, const tbk_fastx_batch *b, const char *bins, const int32_t *counts);
int tbk_bin_writer_rewriter(const tbk_bin_writer *w);
/* The writer's own encoder for gzip members whose bytes do not come in runs (FASTQ of long reads:
 * nothing for LZ77 to match, so entropy coding only - dynamic-Huffman DEFLATE blocks cut at line ends,
 * so that bases and qualities get codes of their own).  One complete gzip member for src[0..n);
 * TBK_ERR_NOMEM with *len = the size needed when cap is too small (2n + 1024 always suffices).
 * Members with runs go through zlib (Z_RLE);
 * TBK_GZIP_ENCODER=zlib sends everything there. */
int tbk_gzip_member(const char *src, size_t n, char *dst, size_t cap, size_t *len);
/* zlib's crc32(crc, p, n) - the CRC-32 of gzip members - by carry-less multiplication (PCLMULQDQ folding,
 * csrc/tbk_crc.cpp; zlib's own where the CPU lacks the instruction or TBK_CRC=zlib): what the reader
 * and the bin writer sum their members with. */
uint32_t tbk_crc32_c(uint32_t crc, const uint8_t *p, size_t n);
/* Replaces the stdout line of classify_by_kmers.py:117 for a whole batch:
 * name \t bin \t str(score_a) \t str(score_b) \n with Python's float repr.  Call with out = NULL
 * to get an upper bound of the size in *len. */
int tbk_format_tsv(const tbk_fastx_batch *b, const char *bins, const double *score_a, const double *score_b,
                   char *out, size_t cap, size_t *len);
/* Python's str(float) of one value (returns the length; cap >= 40). */
int tbk_format_float(double v, char *out, size_t cap);

/* ---- device memory helpers for callers without a HIP binding (bench.py, tests) ------- */
int tbk_device_alloc(int device, size_t bytes, void **d_ptr);
int tbk_device_free(int device, void *d_ptr);
int tbk_memcpy_h2d(int device, void *d_dst, const void *h_src, size_t bytes);
int tbk_memcpy_d2h(int device, void *h_dst, const void *d_src, size_t bytes);
int tbk_device_sync(int device);
int tbk_device_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- synthetic workload generators (BASELINE.json's bench inputs) -------- */
/* Writes keys i in [first, first+n) of the deterministic k-mer sequence for `seed`: each
 * is a distinct canonical k-mer (distinct i -> distinct k-mer), packed as above. */
int tbk_synth_keys_device(int device, uint64_t seed, uint64_t first, uint64_t n, int k, void *d_keys);
/* Host restatement of the same sequence (tests, small sizes). */
int tbk_synth_keys_host(uint64_t seed, uint64_t first, uint64_t n, int k, uint64_t *keys);
/* Fills d_bases with n_reads reads of read_len uniform random ACGT and plants list k-mers
 * (random strand, non-overlapping slots): a read's origin is A/B/none with p .45/.45/.10;
 * origin reads get `plant_major` k-mers of their list and `plant_minor` of the other,
 * origin-less reads get plant_minor+plant_minor.  d_offsets gets n_reads+1 uint64.
 * Keys [0,n_a) of `key_seed` are list A, [n_a, n_a+n_b) list B. */
int tbk_synth_reads_device(int device, uint64_t read_seed, uint64_t first_read, uint64_t n_reads,
                           uint32_t read_len, uint64_t key_seed, uint64_t n_a, uint64_t n_b, int k,
                           int plant_major, int plant_minor, void *d_bases, void *d_offsets);

/* Lists and reads shaped like real trio-binning input instead of uniform keys: an implicit random
 * genome of `genome_len` bases, two haplotypes that each differ from it by SNPs at
 * snp_per_2p24 / 2^24 per base; list A / list B = the canonical k-mers of haplotype A / B that
 * cover a position where the haplotypes differ (runs of up to k overlapping k-mers sharing a few
 * minimizers, both lists clustered at the same loci).  Both lists get *n_keys entries (order not
 * deterministic, sets are); at most `capacity` are written to each of d_keys_a / d_keys_b.
 * Bits 24..31 of snp_per_2p24, when set, add repeats: that many 256ths of the genome's 8192-base
 * blocks are copies of one of 16 family sequences, each copy diverged at 2 % of its positions. */
int tbk_synth_hap_keys_device(int device, uint64_t seed, uint64_t genome_len, uint32_t snp_per_2p24, int k,
                              void *d_keys_a, void *d_keys_b, uint64_t capacity, uint64_t *n_keys);
/* Read r comes from haplotype (first_read + r) & 1, from a hashed position and strand, with
 * substitution errors at err_per_2p24 / 2^24 per base. */
int tbk_synth_hap_reads_device(int device, uint64_t seed, uint64_t genome_len, uint32_t snp_per_2p24,
                               uint64_t read_seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                               uint32_t err_per_2p24, void *d_bases, void *d_offsets);

/* Reads of any lengths (BASELINE configs[4]: "50x ONT ultra-long (N50 100 kb)"; the reference takes a read of any length
 * whole, c/kmers.c:285-287).  tbk_synth_lognormal_lengths (host code) writes offsets[0 .. n_reads]: read first_read + i gets a
 * log-normal length whose base-weighted median (N50) is n50 - ln L ~ N(ln n50 - sigma^2, sigma^2); sigma 0.9: median 44 kb,
 * mean 67 kb, 2.7e-4 of the reads beyond 1 Mb - except that a share short_fraction of the reads is debris, log-uniform
 * between min_len and 5 kb; lengths are clamped to [min_len, max_len].  A read's length depends on (seed, its index) alone.
 * The two generators below fill d_bases for offsets already on the device (d_offsets[n_reads] = total_bases): uniform
 * background with one planted list k-mer per slot_len bases (slot_len 454 = the 33 plants per 15 kb of
 * tbk_synth_reads_device; origin A / B / none as there, every 11th plant of an origin read from the other list), and
 * reads drawn from the two haplotypes (longest_read <= genome_len). */
int tbk_synth_lognormal_lengths(uint64_t seed, uint64_t first_read, uint64_t n_reads, double n50, double sigma, double short_fraction,
                                uint32_t min_len, uint32_t max_len, uint64_t *offsets);
int tbk_synth_reads_ragged_device(int device, uint64_t read_seed, uint64_t first_read, uint64_t n_reads, const void *d_offsets, uint64_t total_bases,
                                  uint64_t key_seed, uint64_t n_a, uint64_t n_b, int k, uint32_t slot_len, void *d_bases);
int tbk_synth_hap_reads_ragged_device(int device, uint64_t seed, uint64_t genome_len, uint32_t snp_per_2p24, uint64_t read_seed, uint64_t first_read,
                                      uint64_t n_reads, const void *d_offsets, uint64_t total_bases, uint64_t longest_read, uint32_t err_per_2p24, void *d_bases);

/* ---- the full-membership sweep (tests/test_gpu_scale.py, bench.py --sweep) -------------------------------------------
 * The reference stores every list line (add_to_hash, c/kmers.c:112-122) and finds every stored canonical key
 * (kmer_in_hash_set, c/kmers.c:245-268).  The paired tables here hold compressed and merged forms of the keys (short keys,
 * entries, wide entries), so that claim is checked key by key at the tables' full size: tbk_classifier_sweep_keys lays the n
 * keys at d_keys (device memory, packed as a list's) out as reads - key i as it stands when i is even, reverse-complemented
 * when odd; keys_per_read = 1: one read of k bases per key (multi-read passes); P > 1: P keys to a read with an 'N' between
 * neighbours, so that a read counts exactly its member keys (single-read and two-read passes) - chunk_keys at a time (0: 2^25),
 * classifies every chunk through tbk_classify_device and compares the counts on the device with what they must be:
 * expect = 1: every key counts (1, 0); 2: (0, 1); 0: (0, 0); or per key from d_expect (uint8, same codes: a read of P keys must count how many of its keys say 1 and how many 2).
 * out[0], out[1] = the sums of the hapA / hapB counts; out[2] = reads that differ from their expectation; out[3] = the index
 * of the first such read (all ones: none).
 * tbk_sweep_expectation_device writes d_expect for arbitrary keys from the two lists' STANDALONE tables (verbatim 64-bit
 * keys, plain hashing - tbk_table_contains; nothing of the paired table's layouts): 1 when hapA's list holds the key's
 * canonical form, else 2 when hapB's does, else 0.  tbk_synth_mutate_keys_device turns keys into near misses: one base
 * substituted (position and base hashed from seed and first + i), canonicalised - a non-member, almost always, that shares
 * m-mer, position and most flank bits with a member.  tbk_table_contains_device: tbk_table_contains with keys and answers
 * in device memory. */
int tbk_table_contains_device(tbk_table *t, const void *d_keys, uint64_t n, void *d_out);
int tbk_synth_mutate_keys_device(int device, const void *d_keys, uint64_t first, uint64_t n, int k, uint64_t seed, void *d_out);
int tbk_sweep_expectation_device(tbk_table *a, tbk_table *b, const void *d_keys, uint64_t n, void *d_expect);
int tbk_classifier_sweep_keys(tbk_classifier *c, const void *d_keys, uint64_t n, int k, uint32_t keys_per_read, int expect, const void *d_expect,
                              uint64_t chunk_keys, uint64_t out[4]);
/* Every line of both lists through the finished table, checked against the lists' standalone tables: the verification a build can
 * be given in the field (a concurrent build - compare-and-swap on slots, the wide entries' per-piece lock - leaves no other
 * trace of a lost or misfiled key).  out = {lines checked, keys counted for hapA, for hapB, lines that differ from what the
 * standalone tables say, the first such line - hapA's lines first, then hapB's; all ones: none}.  Under a second at
 * 2 x 3e8 keys; the standalone tables take 32 bytes of device memory per list line while it runs.  The command-line tool runs it
 * when TBK_VERIFY_BUILD=1. */
int tbk_classifier_verify(tbk_classifier *c, tbk_table *a, tbk_table *b, uint64_t out[5]);
/* What tbk_options.verify_build did when the classifier was made: list lines looked up again (0: not verified) - all of them
 * answered as the lists say, or the constructor would have failed - and the seconds that took. */
int tbk_classifier_verified(const tbk_classifier *c, uint64_t *lines, double *seconds);

/* ---- k-mer counting: the find-unique-kmers step ---------------------------
 * Replaces the KMC subprocesses of find_unique_kmers.py:62-233 by a counting table in HBM.
 * Semantics restated from KMC 3 at the reference's settings (kmc -k<k>, defaults -ci2 -cs255;
 * kmc_tools transform histogram; kmc_tools simple kmers_subtract; kmc_dump -ci -cx): canonical
 * k-mers of all reads, both strands, k-mers holding a symbol outside ACGT skipped, lower case
 * counted as upper case; k-mers seen once are not in the database; counters saturate at 255.
 * KMC itself is not part of the reference checkout: parity with it is unpinned.
 * The table's counters are 32-bit and neighbours share a 64-bit atomic add, so a counter that passed 2^32 (a
 * satellite k-mer of a very deep read set) would carry into the neighbouring slot's; before 2^31 more window
 * starts can have been added, every counter above 2^31 is therefore set back to 2^31 - readers cap at 255 long
 * before, and no count is ever off by a carry (tests/test_gpu_counter_shapes.py takes poly-A past 2^32). */
typedef struct tbk_counter tbk_counter;
/* Table for `capacity_kmers` distinct k-mers to start with (16 bytes per slot at load <= 0.6: a
 * bucket is one 128-byte line holding 8 keys and their 8 counters).  Before a batch that could
 * fill it the table is rebuilt twice as large (old and new coexist for the move); TBK_ERR_NOMEM
 * when HBM cannot hold that. */
int tbk_counter_create(int k, uint64_t capacity_kmers, int device, tbk_counter **out);
void tbk_counter_destroy(tbk_counter *c);
/* Counting in passes, for libraries whose distinct k-mers (sequencing errors included) outgrow one table in HBM.
 * The canonical k-mers fall into `passes` classes by a hash of the k-mer alone.  Every batch added is kept on the
 * device in packed form - one 64-bit word per 16 bases: 2-bit codes and a not-ACGT bit, 0.5 bytes per base - while
 * class 0 is counted from it into a table sized for ONE class (it starts at capacity_kmers / passes and grows by
 * the rule above).  Finishing turns the table into the class's database - the k-mers seen at least twice with
 * their counter capped at 255, 9 bytes each; the k-mers seen once only enter the histogram - then counts class 1,
 * 2, ... from the kept reads into the same table, one after the other, and frees store and table.  Histogram,
 * subtraction and dump then work on the databases and give what one pass gives.  passes = 1 is
 * tbk_counter_create: nothing is kept, nothing is distilled. */
#define TBK_COUNTER_MAX_PASSES 1024
typedef struct tbk_counter_options {
    uint32_t size;              /* sizeof(tbk_counter_options) of the caller (tbk_counter_options_init sets it) */
    int32_t passes;             /* >= 1 */
    uint64_t store_limit_bytes; /* most the kept reads may take; 0: whatever HBM gives.  A batch that would pass
                                 * it (or that HBM cannot take) is TBK_ERR_NOMEM; nothing spills to the host. */
    int32_t compress;           /* != 0: count in homopolymer-compressed space (tbk_hpc below, fold_case = 1): every batch,
                                 * host or device, is compressed before it is separated; in passes mode the kept reads are
                                 * the compressed ones.  reads_added counts the reads as given, bases_added the bases after
                                 * compression, the ones windows came from.  A caller with the older, shorter struct gets 0. */
    int32_t keep_singletons;    /* != 0: the database this counter leaves (tbk_counter_export, and in passes mode every class's)
                                 * is a FULL one: it keeps the k-mers seen once too, counters 1..255 (see tbk_kmerdb below).
                                 * Histogram, tbk_counter_unique and tbk_counter_distinct answer as without it.  The field lies
                                 * in what was the struct's tail padding (sizeof stays 24), so its size cannot tell an older
                                 * caller from a newer one: tbk_counter_options_init writes 0 here, and a caller who fills the
                                 * struct by hand has to zero it (the whole struct, padding included, before setting fields). */
} tbk_counter_options;
void tbk_counter_options_init(tbk_counter_options *o);  /* passes = 1, no limit, no compression, once-seen k-mers not kept */
/* opts may be NULL (= tbk_counter_create). */
int tbk_counter_create_opts(int k, uint64_t capacity_kmers, const tbk_counter_options *opts, int device, tbk_counter **out);
/* No more batches: adding to a finished counter is TBK_ERR_INVALID.  With passes > 1 this counts the remaining
 * classes (see above); tbk_counter_histogram, tbk_counter_distinct and tbk_counter_unique finish such a counter
 * themselves.  With passes = 1 only this call finishes, and it does nothing else. */
int tbk_counter_finish(tbk_counter *c);
typedef struct tbk_counter_info {
    uint32_t size;              /* in: sizeof(tbk_counter_info) of the caller */
    int32_t passes;
    int32_t finished;
    uint32_t reserved;
    uint64_t store_bytes;       /* HBM held by the kept reads (0 once finished, and with passes = 1) */
    uint64_t store_used_bytes;  /* of which filled: 8 bytes per 16 bases of the separated stream, each batch rounded up */
    uint64_t peak_table_bytes;  /* the largest table held at any time (while it is rebuilt, the old one is held too) */
    uint64_t database_bytes;    /* 9 bytes per kept k-mer, over the classes distilled so far: the k-mers seen at least twice,
                                 * or with keep_singletons every distinct k-mer */
    uint64_t distinct;          /* distinct k-mers met: the classes distilled so far plus the class in the table;
                                 * never finishes the counter (tbk_counter_distinct does) */
} tbk_counter_info;
int tbk_counter_stats_ex(const tbk_counter *c, tbk_counter_info *info);
/* Count the canonical k-mers of a batch of reads (the classifier's batch layout; host memory). */
int tbk_counter_add_batch(tbk_counter *c, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads);
/* Same for a batch already in HBM (d_bases readable up to total_bases). */
int tbk_counter_add_device(tbk_counter *c, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t total_bases);
/* HIP-event timing of the counting kernel (every launch is bracketed by an event pair on the stream
 * it runs on): launches, window starts they covered and their summed duration since the last reset. */
int tbk_counter_kernel_timing(tbk_counter *c, uint64_t *launches, uint64_t *window_starts, double *total_ms, int reset);
int tbk_counter_adds_issued(tbk_counter *c, uint64_t *adds);
/* hist[c], c = 1..255: number of distinct k-mers whose counter (capped at 255) is c - the rows
 * kmc_tools writes, except that KMC's -ci2 database has no row-1 k-mers (callers zero hist[1]);
 * hist[0]: all distinct k-mers met. */
int tbk_counter_histogram(tbk_counter *c, uint64_t hist[256]);
/* Distinct k-mers met so far (slots taken).  A counter working in passes is finished first: the number is the sum
 * over its classes. */
int tbk_counter_distinct(const tbk_counter *c, uint64_t *distinct);
int tbk_counter_stats(const tbk_counter *c, uint64_t *n_slots, uint64_t *table_bytes, uint64_t *bases_added, uint64_t *reads_added);
/* Bucket selection of the table as it stands (it is chosen again whenever the table is rebuilt): w m-mers of m bases
 * from base o of the k-mer, t as in the classifier (always 0 here); w = 0 is plain mode.  m > 16 runs the counting
 * kernel's 64-bit m-mer path.  Any pointer may be NULL. */
int tbk_counter_params(const tbk_counter *c, int *w, int *m, int *o, int *t);
/* kmers_subtract + kmc_dump: write to out_path, one k-mer per line in lexicographic order, the
 * k-mers of `a` seen at least twice whose counter lies in [min_count, max_count] and that `b` has
 * seen at most once.  Both counters must work in the same number of passes (TBK_ERR_INVALID otherwise: their
 * classes would not match); counters working in passes are finished first, and the file is the same.  A compressing
 * counter against a plain one is TBK_ERR_INVALID too: their k-mers live in different spaces. */
int tbk_counter_unique(tbk_counter *a, tbk_counter *b, uint32_t min_count, uint32_t max_count, const char *out_path,
                       uint64_t *n_written);

/* ---- count databases: what a counter leaves behind, kept -----------------------------------
 * The reference's `kmc` leaves haplotypeA.* / haplotypeB.* under --outpath (find_unique_kmers.py:247) and its
 * HistogramError tells the user to choose cut-offs by hand and dump again.  A tbk_kmerdb is that database: on
 * one device, k, n keys - lexicographic ranks (base 0 in the top bits of the 2k, A < C < G < T), strictly
 * ascending - n one-byte counters in 2..255, the whole 256-row histogram of the counter it came from (row 1 the
 * k-mers seen once, row 0 all distinct k-mers, as tbk_counter_histogram defines them) and the reads and bases
 * that were counted.  9 bytes of HBM per k-mer; twice that while tbk_counter_export orders one.  It outlives
 * its counter.
 * A database has a FLOOR, the lowest counter it holds.  2 is the form above.  1 is a FULL database, what a counter with
 * keep_singletons leaves: the k-mers seen once are entries too, counters lie in 1..255, and n == hist[0] ==
 * sum(hist[1..255]).  Two databases of floor 2 cannot be united - a k-mer seen once in each half is in neither, so a
 * union would not equal one count of both halves - but two full ones can, exactly (tbk_kmerdb_union), and
 * tbk_kmerdb_solid takes a full database back to floor 2.  The query session takes either form; the subtractions and
 * list builders below take floor 2 only. */
typedef struct tbk_kmerdb tbk_kmerdb;
/* Finishes the counter (no more batches: tbk_counter_add_batch is TBK_ERR_INVALID afterwards; a counter in passes
 * counts its remaining classes first) and makes its database.  A one-pass counter's table is only read:
 * tbk_counter_histogram and tbk_counter_unique answer afterwards as before.  The database is the same whatever
 * `passes` was.  TBK_ERR_NOMEM leaves the counter as it was (a one-pass counter not even finished). */
int tbk_counter_export(tbk_counter *c, tbk_kmerdb **out);
void tbk_kmerdb_destroy(tbk_kmerdb *db);
/* The file (*.tbkdb, little-endian; INTEGRATION.md has the table): a 2096-byte header - magic "TBKKMDB1", header
 * size, k, n, reads, bases, the histogram, CRC-32 of all that, a zero word - then n keys, then n counters: exactly
 * 2096 + 9n bytes.  Written to path + ".tmp" in pieces and renamed, so an interrupted save leaves no file of the
 * right name; no time stamp, no host name: equal databases give equal bytes.
 * The database of a compressing counter (tbk_counter_options.compress) is a different thing from a plain one of the
 * same k, and its file says so: magic "TBKKMDH1", otherwise the identical layout - a build that does not know
 * compressed databases refuses the file instead of mixing the two spaces.  tbk_counter_export carries the flag,
 * tbk_kmerdb_save writes the matching magic, tbk_kmerdb_load accepts both and remembers which it was. */
int tbk_kmerdb_save(const tbk_kmerdb *db, const char *path);
/* A file is checked before it is used.  On the host: magic, header size, k in 1..32, CRC, zero pad, file size
 * against n, sum(hist[2..255]) == n, hist[0] >= hist[1] + n.  On the device, in one pass before anything
 * searches the keys: strictly ascending keys, no key bit above 2k, no counter below 2, and the counters' tally
 * equal to the header's rows 2..255.  A missing or unreadable file is TBK_ERR_IO, everything else TBK_ERR_FORMAT
 * with the reason in tbk_last_error(); *out stays NULL and the device stays usable. */
int tbk_kmerdb_load(const char *path, int device, tbk_kmerdb **out);
/* The header alone, with the host-side checks above; needs no device.  Any out pointer may be NULL. */
int tbk_kmerdb_file_info(const char *path, int *k, uint64_t *n, uint64_t hist[256], uint64_t *reads, uint64_t *bases);
/* *flag = 1 when the database was counted in homopolymer-compressed space, else 0: of a database in HBM, and of a file
 * (the host-side checks of tbk_kmerdb_file_info; needs no device). */
int tbk_kmerdb_compressed(const tbk_kmerdb *db, int *flag);
int tbk_kmerdb_file_compressed(const char *path, int *flag);
/* A full database's file has a magic of its own, "TBKKMFB1" (plain) or "TBKKMFH1" (compressed), and otherwise the identical
 * 2096 + 9n layout; a build that does not know full databases refuses it at the magic.  Its header must state rows 1..255
 * summing to n and row 0 == n; on the device no counter may be below 1 and the tally of rows 1..255 must equal the header's.
 * tbk_kmerdb_save writes the magic that matches floor and space. */
int tbk_kmerdb_floor(const tbk_kmerdb *db, int *floor);      /* 2, or 1: the database holds the k-mers seen once */
int tbk_kmerdb_file_floor(const char *path, int *floor);     /* host-side checks only, needs no device */
/* The database of both read sets: what one counter with keep_singletons, fed the reads of `a` and then those of `b`, would
 * export, byte for byte - the ascending union of the keys, min(255, ca + cb) for a key both hold (added in 32 bits) and the
 * own counter otherwise, reads and bases summed, the histogram tallied from the merged counters on the device (rows 1..255;
 * row 0 = n).  Exact because min(255, min(255, x) + min(255, y)) == min(255, x + y).  Both must be full, of one k, one device
 * and one space: anything else is TBK_ERR_INVALID with the reason in tbk_last_error() - for a floor-2 argument, that it was
 * kept without the once-seen k-mers and cannot be united exactly.  Either may be empty.  Nothing is sorted or concatenated:
 * both inputs ascend, so every entry's place is its index plus its lower bound in the other database less the shared keys
 * before it.  Launches: flag the entries of A that B holds (a bit per entry, a count per tile of 1024), scan the counts,
 * scatter A, scatter B (B's copy of a shared key writes nothing), tally.  The output is allocated at its exact size once the
 * number of shared keys is known; beside it the call takes n_a/8 + n_a/64 bytes and 2 KiB, freed before it returns.
 * TBK_ERR_NOMEM leaves both inputs as they were and the device usable; *out is NULL after every error. */
int tbk_kmerdb_union(const tbk_kmerdb *a, const tbk_kmerdb *b, tbk_kmerdb **out);
/* From a full database the floor-2 database of the same reads: the entries with a counter of 2 or more, in place order (flag,
 * scan, scatter of keys and counters); histogram, reads and bases carried over - row 1 stays the number of once-seen k-mers,
 * row 0 all distinct ones.  Saved, it is byte for byte the file the same counter without keep_singletons would have left.  A
 * floor-2 argument is TBK_ERR_INVALID.  n/8 + n/64 bytes beside the output; *out is NULL after every error. */
int tbk_kmerdb_solid(const tbk_kmerdb *db, tbk_kmerdb **out);
/* bytes: HBM the database holds (9n).  Any out pointer may be NULL. */
int tbk_kmerdb_info(const tbk_kmerdb *db, int *k, uint64_t *n, int *device, uint64_t *bytes);
int tbk_kmerdb_stats(const tbk_kmerdb *db, uint64_t *reads_added, uint64_t *bases_added);
int tbk_kmerdb_histogram(const tbk_kmerdb *db, uint64_t hist[256]);
/* Entries first .. first + count - 1 to host memory (either pointer may be NULL); a range outside the database
 * is TBK_ERR_INVALID. */
int tbk_kmerdb_read(const tbk_kmerdb *db, uint64_t first, uint64_t count, uint64_t *keys, uint8_t *counts);
/* tbk_counter_unique between two databases: the k-mers of `a` whose counter lies in [max(2, min_count),
 * min(255, max_count)] and that `b` does not hold, one per line in lexicographic order - the same file.  An
 * empty range or an empty `a` gives an empty file and TBK_OK; a different k or device is TBK_ERR_INVALID, and so
 * is a compressed database against a plain one - here and in the three calls below, the child's database included -
 * with the reason in tbk_last_error().  So is a full database in any position of these four calls: membership in `b` is
 * tested by key alone, and a full `b` would subtract the k-mers it saw once; the message names tbk_kmerdb_solid. */
int tbk_kmerdb_unique(const tbk_kmerdb *a, const tbk_kmerdb *b, uint32_t min_count, uint32_t max_count, const char *out_path,
                      uint64_t *n_written);
/* The same selection as a k-mer list in HBM on the databases' device, without the text: for every consumer
 * (tbk_table_num_kmers, tbk_table_k, tbk_table_keys, tbk_classifier_create*, tbk_pipeline_create*, the other
 * devices of a multi-device classifier) *out is what tbk_table_create_from_file gives on the file
 * tbk_kmerdb_unique would have written - the same keys (tbk_kmer_to_int's packing) in the same, lexicographic,
 * order, the same number of lines; tbk_table_origin says 3.  A's ranks ascend, so the selected ones are
 * compacted in place order and nothing is sorted: three launches (one bit per entry of A and a count per tile of
 * 1024 entries; a scan of the tile counts; the scatter, which turns each rank into its key), no block waiting
 * for another.  The keys are allocated at their exact number once it is known; beside them the call takes
 * n/8 + n/64 bytes for A's n entries, freed before it returns.  A different k or device is TBK_ERR_INVALID, as
 * above.  An empty selection is TBK_ERR_FORMAT, "empty k-mer list", as an empty list file is.  TBK_ERR_NOMEM
 * leaves both databases as they were and the device usable.  *out is NULL after every error. */
int tbk_kmerdb_unique_table(const tbk_kmerdb *a, const tbk_kmerdb *b, uint32_t min_count, uint32_t max_count, tbk_table **out);
/* The same two calls with a third database, the child's: of the k-mers above (counter of `a` in [max(2, min_count),
 * min(255, max_count)], not held by `b`) only those that `child` holds with a counter in [max(2, child_min),
 * min(255, child_max)] - the parental k-mers the child inherited.  A child database, like any other, holds only
 * k-mers seen at least twice.  tbk_kmerdb_inherited writes the file tbk_kmerdb_unique would write for that set
 * (lexicographic, one k-mer per line; an empty selection is an empty file and TBK_OK); the set comes compacted in
 * A's order, so nothing is sorted and no buffer is larger than the list.  tbk_kmerdb_inherited_table leaves it as
 * the list tbk_kmerdb_unique_table would make of that set: the same order and key form, tbk_table_origin 3, an
 * empty selection TBK_ERR_FORMAT "empty k-mer list".  One block flags a tile of 1024 entries of A: it first finds
 * where the tile's first and last rank would stand in `b` and in `child`, and each entry then searches between
 * those places only, `b` before `child`.  Beside the output both calls take n/8 + n/64 bytes for A's n entries,
 * freed before they return.  A NULL database, a different k or a different device among the three is
 * TBK_ERR_INVALID; TBK_ERR_NOMEM leaves all three databases as they were and the device usable; *out is NULL after
 * every error. */
int tbk_kmerdb_inherited(const tbk_kmerdb *a, const tbk_kmerdb *b, const tbk_kmerdb *child, uint32_t min_count, uint32_t max_count,
                         uint32_t child_min, uint32_t child_max, const char *out_path, uint64_t *n_written);
int tbk_kmerdb_inherited_table(const tbk_kmerdb *a, const tbk_kmerdb *b, const tbk_kmerdb *child, uint32_t min_count, uint32_t max_count,
                               uint32_t child_min, uint32_t child_max, tbk_table **out);
/* Two databases held against each other: the joint k-mer spectrum (the matrix `kat comp` and Merqury's read-set comparisons
 * plot).  spec[cx * 256 + cy] is the number of distinct k-mers whose counter is cx in `x` and cy in `y`; counter 0 means "the
 * database holds no entry for it".  Either floor is accepted in either position, and what 0 means follows from each database's
 * floor: for a full database (floor 1) "never seen in its reads" - its once-seen k-mers are entries with counter 1 - and for a
 * floor-2 database "seen once or never".  By construction spec[0] (the cell 0,0) is 0, row c >= 1 sums to the entries of `x`
 * with counter c, column c >= 1 to those of `y`, and the whole matrix to the size of the union of the two key sets.  Two
 * launches, each striding over the tiles of 1024 entries of the database it walks (csrc/tbk_compare.hip): over `x`, where every
 * entry searches `y` between its tile's bounds there and goes to the cell (cx, cy or 0), and over `y`, where the entries `x`
 * lacks go to the cell (0, cy).  Blocks tally in LDS and flush once.  Beside the inputs the call holds the matrix (512 KiB).
 * Both calls: all databases must have one k, one device and one space (plain or homopolymer-compressed); a NULL argument or a
 * mismatch is TBK_ERR_INVALID with the reason in tbk_last_error().  Empty databases are legal in any position.  The inputs are
 * only read; TBK_ERR_NOMEM leaves every database as it was and the device usable. */
int tbk_kmerdb_joint_spectrum(const tbk_kmerdb *x, const tbk_kmerdb *y, uint64_t spec[256 * 256]);
/* The entries of `base` by counter and by which of two partners hold them: spec[cls * 256 + c] is the number of entries of
 * `base` with counter c and class cls.  Bit 0 of cls is set when `y` holds the key with a counter in [y_min, y_max], bit 1 is
 * the same for `z`.  The ranges are taken literally - 1 <= min <= max <= 255, TBK_ERR_INVALID otherwise - and are NOT the
 * "2 or more" rule of the subtractions above: a full partner is asked with min = 2 to ignore its once-seen k-mers.  Row 0 of
 * every class is 0, and the four classes of a counter sum to the entries of `base` with that counter.  One launch over `base`;
 * the call holds 8 KiB beside the inputs.  With base = the child and the parents as partners, class 0 is what the child holds
 * of neither parent; with base = a parent, partners the other parent and the child, class 0 | 2 is that parent's own k-mers
 * and class 2 those of them the child inherited. */
int tbk_kmerdb_origin_spectrum(const tbk_kmerdb *base, const tbk_kmerdb *y, uint32_t y_min, uint32_t y_max,
                               const tbk_kmerdb *z, uint32_t z_min, uint32_t z_max, uint64_t spec[4 * 256]);
/* ONE database by the GC content of its k-mers: k-mer multiplicity against GC, the matrix `kat gcp` plots - a contaminant of
 * another GC and depth is a second cloud in it, and a library that under-covers AT-rich or GC-rich sequence shows in its rows.
 * spec[g * 256 + c] is the number of entries whose key has g G-or-C bases and whose counter is c.  THE GC OF A KEY: a key is a
 * rank, 2 bits a base with A, C, G, T = 0, 1, 2, 3, and a base is G or C exactly when its two bits differ, so
 * g = popcount((key ^ (key >> 1)) & 0x5555555555555555), 0..k; a k-mer and its reverse complement have one g, so the canonical
 * choice does not matter, and in a homopolymer-compressed database g is the GC of the compressed k-mer.  Rows above k are 0 and
 * column 0 is 0; column c >= 1 sums over g to row c of the database's own counters (tbk_kmerdb_histogram, from the floor on),
 * and the whole matrix to n.  Either floor and either space are accepted; an empty database gives a zero matrix and TBK_OK.
 * One launch striding over the tiles of 1024 entries (csrc/tbk_compare.hip); blocks tally the (k + 1) x 256 cells in LDS and
 * flush once.  Beside the input the call holds the matrix (66 KiB).  A NULL argument is TBK_ERR_INVALID with the reason in
 * tbk_last_error(); the database is only read; TBK_ERR_NOMEM leaves it as it was and the device usable. */
int tbk_kmerdb_gc_spectrum(const tbk_kmerdb *db, uint64_t spec[33 * 256]);
/* A selection that stays a database: the entries of `base` that up to two partners let pass, with a counter of choice - the
 * hap-mer databases of Merqury's hapmers.sh ("the parental k-mers the child inherited, with the child's counters"), the k-mers
 * two lanes share, a library minus a contaminant.  Every other join here ends in text, in keys without counters or in a tally.
 * WHICH ENTRIES ARE KEPT.  An entry of `base` is kept when its counter lies in [o->min_count, o->max_count] and, for every
 * partner, "the partner holds the key with a counter in the partner's [min_count, max_count]" is true for TBK_SELECT_REQUIRE
 * and false for TBK_SELECT_EXCLUDE.  All ranges are taken literally - 1 <= min <= max <= 255, as in
 * tbk_kmerdb_origin_spectrum - and are NOT the "2 or more" rule of the subtractions: a full partner is asked with min = 2 to
 * ignore its once-seen k-mers, a floor-2 partner asked with [1, 255] means "holds the key at all".  n_partners is 0, 1 or 2
 * (`partners` may be NULL for 0); more partners are done by chaining calls.  A database may appear more than once and may be
 * `base` itself; either floor is accepted in every position.  On top of all that an entry is kept only when the G-or-C bases
 * of its key (tbk_kmerdb_gc_spectrum has the rule) lie in [o->min_gc, o->max_gc]: a cloud of that matrix carved out as a
 * database.  The bounds are bases, not per cent; 0 and 32, which tbk_select_options_init sets, never bind, nor does any bound
 * above k.  The two fields were added behind `counter`: a caller whose `size` is the struct's of before them (24 bytes) is
 * accepted as it was and gets no GC bound.
 * THE COUNTER OF A KEPT ENTRY.  TBK_SELECT_COUNTER_BASE: the base's.  _MIN: the minimum of the base's counter and every REQUIRE
 * partner's.  _SUM: min(255, base + the REQUIRE partners'), added in 32 bits.  EXCLUDE partners never contribute; with no
 * REQUIRE partner all three rules give the base's counter.
 * THE RESULT is a database in the FULL form (floor 1) whatever the inputs' floors were: its keys are the kept ranks in base's
 * order, which stays ascending, so nothing is sorted.  Rows 1..255 of its histogram are tallied from its own counters, row 0 is
 * n, reads and bases are 0 - a selection is no library, as an import without --reads is none; k and the space (plain or
 * compressed) are base's.  Full is the form that states exactly the multiset held: tbk_kmerdb_union of two selections is exact
 * multiset addition, the query session takes it as it is, and tbk_kmerdb_solid (load_solid_database) drops its counter-1
 * entries and nothing else.  A floor-2 header would claim that every k-mer of a library seen twice is here; a selection makes
 * no such claim.  An empty selection, or an empty base, is TBK_OK and a valid database of n = 0 (its file: 2096 bytes).
 * REFUSALS are TBK_ERR_INVALID with the reason in tbk_last_error(): a NULL base, o, out or partner's db; n_partners outside
 * 0..2; a mode, counter rule or range outside the above (min_gc > max_gc or max_gc > 32 among them); a different k, device or space among the databases (the messages of
 * the spectra above).  *out is NULL after every error; TBK_ERR_NOMEM leaves every input as it was and the device usable.
 * LAUNCHES (csrc/tbk_select.hip): flag - one block per tile of 1024 entries of base finds the tile's bounds in both partners,
 * and every entry tests its own counter and GC, then the first partner, then the second only if the first let it pass (EXCLUDE
 * partners are asked first); the scan of the tile counts; the scatter of keys and counters - for _MIN and _SUM with one more
 * bounded bisection per kept entry and REQUIRE partner, the kept entries dealt to consecutive threads so that a wave bisects
 * with all its lanes; the tally of the output's counters.  No block waits for another.  The
 * output is allocated at its exact size once the number kept is known; beside it the call holds n/8 + n/64 bytes for base's n
 * entries and 2 KiB, freed before it returns. */
#define TBK_SELECT_REQUIRE 1
#define TBK_SELECT_EXCLUDE 2
#define TBK_SELECT_COUNTER_BASE 0
#define TBK_SELECT_COUNTER_MIN  1
#define TBK_SELECT_COUNTER_SUM  2
typedef struct tbk_select_partner {
    const tbk_kmerdb *db;
    uint32_t min_count, max_count;  /* the partner's counter range, 1 <= min <= max <= 255 */
    int mode;                       /* TBK_SELECT_REQUIRE or TBK_SELECT_EXCLUDE */
} tbk_select_partner;
typedef struct tbk_select_options {
    size_t size;                    /* sizeof(tbk_select_options) of the caller (tbk_select_options_init sets it) */
    uint32_t min_count, max_count;  /* base's counter range, 1 <= min <= max <= 255 */
    int counter;                    /* TBK_SELECT_COUNTER_BASE, _MIN or _SUM */
    uint32_t min_gc, max_gc;        /* base's GC range in bases, 0 <= min <= max <= 32; read only from a `size` that reaches them */
} tbk_select_options;
void tbk_select_options_init(tbk_select_options *o);  /* 1, 255, TBK_SELECT_COUNTER_BASE, 0, 32 */
int tbk_kmerdb_select(const tbk_kmerdb *base, const tbk_select_partner *partners, int n_partners, const tbk_select_options *o,
                      tbk_kmerdb **out);
/* The het-mer pairs of ONE database: the look inside a library that the k-mer-pair analysis of Smudgeplot / PloidyPlot takes
 * from the reads alone - how heterozygous is it, is it diploid at all - and, with the parents' databases beside the child's,
 * how many of its heterozygous sites the parents' k-mers mark.  All integer, all exact.
 * PARTNERS.  k is odd and m = (k - 1) / 2: position m is the only one reverse complement maps to itself.  For a canonical k-mer
 * x (the lexicographic minimum of a k-mer and its reverse complement, as the counter has it), substitute each of the three
 * other bases at position m, make each result canonical and drop x itself: the distinct canonical k-mers that remain are the
 * MIDDLE PARTNERS of x.  They are a set: a variant can be x itself (AAT -> ATT, its reverse complement) and two variants can be
 * one k-mer (whenever the flanks are each other's reverse complement: AAT has the single partner ACT).  A k-mer has 3 partners,
 * or 1 when its flanks are self-reverse-complementary; the relation is symmetric and transitive, so classes hold 4 or 2 k-mers.
 * CANDIDATES AND PAIRS.  The candidates are the entries of `db` whose counter lies in [o->min_count, o->max_count], taken
 * literally, 1 <= min <= max <= 255; either floor is accepted.  A candidate's partners in range are its middle partners that
 * are candidates too, 0 to 3 of them.  A HET-MER PAIR is a candidate with exactly one partner in range, and that partner
 * (which then has exactly one, the first).  The MINOR member of a pair has the lower counter, on a tie the lower rank.
 * THE RESULT.  candidates; partners[j], the candidates with j partners in range (partners[1] == 2 * pairs, partners[2] % 3 == 0,
 * partners[3] % 4 == 0); pairs; spec[c_minor * 256 + c_major], whose cells with c_minor > c_major and whose row and column 0
 * are 0 and which sums to pairs; origin[cls_minor * 4 + cls_major], where cls is the class of tbk_kmerdb_origin_spectrum: bit 0
 * set when o->y holds the key with a counter in [y_min, y_max], bit 1 likewise for o->z.  A partner that is NULL contributes
 * bit 0; the 16 cells sum to pairs, and with neither partner all pairs are in origin[0].  With o->want_pairs, *out_pairs
 * takes the pairs themselves, pairs records in memory of tbk_host_alloc that is the caller's to tbk_host_free (NULL when there
 * is none, and after every error): ranks in the form tbk_kmerdb_read hands out, ascending by the rank of each pair's
 * lower-ranked member.  out_pairs may be NULL when no pairs are wanted.
 * REFUSALS, TBK_ERR_INVALID with the reason in tbk_last_error() before any kernel runs: an even k (the middle base must be its
 * own mirror under reverse complement); a range outside 1 <= min <= max <= 255; a partner of another k, device or space; a
 * database of more than 2^32 - 1 entries (the directory's offsets are 32-bit words and its last one is n itself; y and z are
 * bisected with 64-bit offsets and may be larger).  An empty database is legal: everything is zero.  Homopolymer-compressed
 * databases are accepted when all given are: a variant that puts two equal bases side by side is no compressed k-mer, is in no
 * such database and is simply never found - no rule is needed.  TBK_ERR_NOMEM leaves every input as it was and the device
 * usable.
 * LAUNCHES (csrc/tbk_hetmer.hip): the directory over the top floor(log2 n) - 1 bits of the rank (the query session's kernel);
 * the tally - blocks stride over tiles of 1024 entries, every candidate makes its three variants canonical, drops the equal
 * ones and searches the rest side by side through the directory, and only pairs ask y and z; with want_pairs also flag, the
 * scan of the tile counts and a scatter that finds each pair's partner again.  No block waits for another.  Beside the inputs
 * and the records the call holds the directory (4 * (2^P + 1) bytes, at most 2 n + 4 and at most 1 GiB), the two result
 * matrices (512 KiB + 176 bytes) and, with want_pairs, n/8 + n/64 bytes; all freed before it returns. */
typedef struct tbk_hetmer_pair {
    uint64_t minor, major;        /* the two ranks */
    uint8_t c_minor, c_major;     /* their counters, c_minor <= c_major */
    uint8_t cls_minor, cls_major; /* their origin classes, 0..3 */
    uint8_t reserved[4];          /* 0 */
} tbk_hetmer_pair;
typedef struct tbk_hetmer_options {
    size_t size;                    /* sizeof(tbk_hetmer_options) of the caller (tbk_hetmer_options_init sets it) */
    uint32_t min_count, max_count;  /* the candidates' counter range, 1 <= min <= max <= 255 */
    const tbk_kmerdb *y, *z;        /* partner databases, each may be NULL */
    uint32_t y_min, y_max;          /* 1 <= min <= max <= 255, checked whether or not y is given */
    uint32_t z_min, z_max;
    int want_pairs;                 /* not 0: the records too */
} tbk_hetmer_options;
typedef struct tbk_hetmer_result {
    size_t size;                    /* sizeof(tbk_hetmer_result) of the caller (tbk_hetmer_result_init sets it) */
    uint64_t candidates;
    uint64_t partners[4];
    uint64_t pairs;
    uint64_t origin[16];
} tbk_hetmer_result;
void tbk_hetmer_options_init(tbk_hetmer_options *o);  /* 1, 255, no partners, their ranges 1..255, no pairs */
void tbk_hetmer_result_init(tbk_hetmer_result *r);    /* the size, everything else 0 */
int tbk_kmerdb_hetmers(const tbk_kmerdb *db, const tbk_hetmer_options *o, tbk_hetmer_result *result, uint64_t spec[256 * 256],
                       tbk_hetmer_pair **out_pairs);

/* ---- counted k-mer dumps: a database from the text other counters print, and back ----------------------------
 * `kmc_dump`, `meryl print` (tab) and `jellyfish dump -c` (space) print one line per k-mer, KMER<sep>COUNT.
 * tbk_kmerdb_import_text makes a database of such text on one device; tbk_kmerdb_dump_text writes a database as such text.
 * THE LINE RULE.  A line is K S D and then '\n': K exactly k bytes, each one of ACGT (lower case, N and anything else are
 * refused); S one tab or one space; D 1 to 32 decimal digits and nothing else (no sign, no '\r').  The last line of a file
 * may lack its '\n'.  An empty line is refused; an empty file is fine.  A line longer than k + 35 bytes is refused ("line too
 * long").  The value of D saturates at 255; 0 is refused.  Several files are read as one text, each under its own line rule.
 * THE KEY is the canonical k-mer - the smaller, as strings, of the k-mer and its reverse complement - as the database's
 * lexicographic rank.  REPEATED KEYS (both strands listed, several lanes' dumps, one file given twice) fold to min(255, sum):
 * exact on saturated counters for the reason tbk_kmerdb_union is.
 * floor = 1 makes a full database: every entry kept, rows 1..255 summing to n, row 0 = n.  floor = 2 makes the solid form:
 * entries whose folded counter is 1 are left out but tallied in row 1, row 0 is the number of distinct keys.  floor = 0 means
 * 1 when any folded counter is 1, else 2.  compressed = 1: a k-mer with two equal adjacent bases is refused, and the database
 * says that it lives in homopolymer-compressed space.  The file magic follows floor and space as for any database.
 * REFUSALS are TBK_ERR_FORMAT, "<file>: line <1-based number>: <reason>" - the FIRST offending line in file order, whichever
 * window it lies in; *out is NULL and the device stays usable.  A missing file is TBK_ERR_IO, no memory TBK_ERR_NOMEM.
 * On the device (csrc/tbk_dump.hip): the files are mapped and cut into windows of window_bytes at a newline, staged through
 * two pinned buffers on a stream of the call's own; per window one bit per byte for newlines and a count per tile of 4096
 * bytes, the scan of the counts, and the parse - the lane that holds a line start takes the line's number from the scanned
 * count and the popcounts below it and writes its pair there.  Then one checking pass: keys that ascend strictly (kmc_dump,
 * meryl print of canonical counts) are neither sorted nor folded; otherwise the pairs are sorted (rocPRIM, 2k bits), the heads
 * of runs of equal keys flagged, scanned, and scattered with their runs' saturating sums.  No block waits for another.
 * MEMORY: 9 bytes per pair while appending, reserved for the most lines the text can hold (its bytes / (k + 3)); a second 9 n
 * plus rocPRIM's temporary storage only when the sort runs; one window of text, n/8 + n/64 bytes during a compaction. */
typedef struct tbk_dump_options {
    size_t size;            /* sizeof(tbk_dump_options) of the caller (tbk_dump_options_init sets it) */
    int k;                  /* 0: taken from the first line of the first file that has one */
    int floor;              /* 0 auto, 1, 2 (above) */
    int compressed;         /* 1: the k-mers are homopolymer-compressed; checked on every line, and the database says so */
    uint64_t reads, bases;  /* stamped into the header (a dump does not know them); default 0 */
    uint64_t window_bytes;  /* text per device window; 0 = default (64 MiB); at least 4096 */
} tbk_dump_options;
void tbk_dump_options_init(tbk_dump_options *o);
int tbk_kmerdb_import_text(const char *const *paths, int n_paths, const tbk_dump_options *o, int device, tbk_kmerdb **out);
/* Host only, no device: the bytes before the first tab or space of line 1.  An empty file, a line 1 without a separator and a
 * k outside 1..32 are TBK_ERR_FORMAT. */
int tbk_dump_file_k(const char *path, int *k);
/* What `kmc_dump -ciMIN -cxMAX` writes: KMER<tab>COUNT<newline> in lexicographic order for the entries whose counter lies in
 * [max(floor, min_count), min(255, max_count)], of any database - solid or full, plain or compressed.  An empty selection is an
 * empty file and TBK_OK.  The selection runs on the device (flag, scan, scatter of keys and counters; skipped when every entry
 * is selected); the 9-byte entries come home in pieces and the host's threads format them - text is (k + 4) / 9 of the entries'
 * bytes and the link bounds a dump, so nothing is gained by formatting on the device.  Written to out_path + ".tmp" and renamed. */
int tbk_kmerdb_dump_text(const tbk_kmerdb *db, uint32_t min_count, uint32_t max_count, const char *out_path, uint64_t *n_written);
/* Running totals of this process's imports: calls that reached a device, those of them that had to sort, windows launched,
 * lines parsed, and the HIP-event time of the newline and parse kernels.  Any pointer may be NULL. */
int tbk_dump_import_stats(uint64_t *imports, uint64_t *sorts, uint64_t *windows, uint64_t *lines, double *parse_ms);

/* ---- homopolymer compression: every run of equal bases written once, before k-mers are cut --------------------
 * The dominant error of ONT and HiFi reads is the length of a homopolymer run; pipelines beside this one bin in
 * homopolymer-compressed space for that reason (meryl `count compress`, Canu's and Verkko's trio modes): parental
 * libraries and reads then agree wherever they differ in run length only.
 * compress(read, fold_case) keeps byte i of a read iff i == 0 or f(b[i]) != f(b[i-1]).  With fold_case, f clears bit
 * 5 of ASCII letters (a compares equal to A); without it f is the identity.  A kept byte is written verbatim: the
 * first byte of its run, in its own case.  A run never crosses a read boundary.  Bytes outside ACGT are compared like
 * any others (NNNN becomes N, which still breaks windows downstream).  An empty read stays empty; read count and order
 * are unchanged.  The counter folds case (fold_case = 1); the classifier does not (0: lower case stays not-ACGT).
 * A session lives on one device and owns a stream and its buffers, which grow to the largest batch seen; one batch at
 * a time per session.  The result is a batch in the usual layout, left in HBM: bases back to back (16-byte aligned,
 * 64 zero bytes behind the last), uint64 offsets with offsets[0] == 0 - what tbk_classify_device,
 * tbk_stream_submit_device and tbk_counter_add_device take.  Both compress calls return when the result is complete;
 * it is valid until the session's next call.  n_reads == 0 or no bases at all: TBK_OK and an empty result.  Offsets
 * that do not ascend (for a device batch: not from 0 to total_bases; checked on the device, nothing is written out of
 * bounds): TBK_ERR_INVALID.  TBK_ERR_NOMEM leaves the session usable.  After an error the out pointers are NULL.
 * On the device (csrc/tbk_hpc.hip): one bit per base for read starts; one bit per base for `keep` and a count per
 * tile of 4096 bases, read as 16-byte vectors; an exclusive scan of the tile counts; a scatter of the kept bytes; one
 * thread per read turning offsets[r] into its rank among the kept bits.  No block waits for another. */
typedef struct tbk_hpc tbk_hpc;
int tbk_hpc_create(int device, tbk_hpc **out);
void tbk_hpc_destroy(tbk_hpc *h);
int tbk_hpc_compress(tbk_hpc *h, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int fold_case, void **d_bases,
                     void **d_offsets, uint64_t *total_out);
/* The same for a batch already in HBM: d_bases 16-byte aligned and readable up to total_bases, d_offsets[n_reads] == total_bases. */
int tbk_hpc_compress_device(tbk_hpc *h, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t total_bases, int fold_case,
                            void **d_bases_out, void **d_offsets_out, uint64_t *total_out);
/* The last result to host memory: total_out bytes to `bases` (cap: its room; too little is TBK_ERR_INVALID) and
 * n_reads + 1 offsets to `offsets` (may be NULL). */
int tbk_hpc_fetch(tbk_hpc *h, uint8_t *bases, uint64_t cap, uint64_t *offsets);
/* The map read backwards.  The session keeps the keep bits and the scanned tile counts of its last result until its
 * next compress call.  With total / offsets the batch as given and total_c / coff its compressed form: kept byte j
 * (0 <= j < total_c) came from input position lift(j), the position of the j-th set keep bit, and lift(total_c) =
 * total.  Then lift(coff[r]) == offsets[r] for every r in 0 .. n_reads (empty reads included), and window w of k bytes
 * of compressed read r covers the original bases [lift(coff[r] + w) - offsets[r], lift(coff[r] + w + k) - offsets[r])
 * of read r: that span compresses to exactly the window's bytes, and a window that reaches the compressed end of
 * the read ends at the read's length - its trailing run belongs to it.
 * tbk_hpc_lift: out[i] = lift(positions[i]) for n positions in host arrays, in any order, duplicates allowed.  n == 0
 * is TBK_OK; a position above total_c is TBK_ERR_INVALID (nothing is written); a session without a result is
 * TBK_ERR_INVALID; the session and its result stay usable after either refusal.  One lane bisects the tile offsets for
 * the last tile that starts at or before its position (a homopolymer longer than a tile leaves tiles without a kept bit,
 * which share their successor's offset); the wave then finds the keep word among the tile's 64 by popcounts and the lane
 * selects the bit.
 * tbk_hpc_expand: one value per kept byte in (total_c bytes), one per base of the batch as given out (total bytes):
 * out[lift(j)] = values[j], every other byte 0.  An empty batch writes nothing. */
int tbk_hpc_lift(tbk_hpc *h, const uint64_t *positions, uint64_t n, uint64_t *out);
int tbk_hpc_expand(tbk_hpc *h, const uint8_t *values, uint8_t *out);

/* ---- hit tracker: WHERE along a sequence the haplotype k-mers lie ------------------------ */
/* The classifier answers with two numbers per read; the tracker keeps the positions.  A window start is a MARKER of
 * hapA or hapB by the rule of tbk_count_kmers_in_read: windows 0 .. len - k, key = min(forward, reverse complement),
 * a window holding a byte outside upper-case ACGT is none, hapA is asked first (a key both lists hold marks A only),
 * lists hold their lines verbatim (a non-canonical line never hits).  ignore_case != 0 reads lower-case acgt as
 * upper-case; 0 leaves them not-ACGT, as the classifier does.
 * A raw RUN is a maximal sequence of one read's markers, in position order, that are of one haplotype: consecutive in
 * marker order, however far apart, and never across a read boundary.  first / last: window starts of its first and
 * last marker within the read; a run's extent in bases is last + k - first.
 * The tracker borrows the two lists (they must outlive it; same k, same device, else TBK_ERR_INVALID), builds their
 * standalone tables on first use and owns its device buffers, which grow to the largest batch seen.  One batch at a
 * time per tracker.  The work is on the device: separation, marking (one wave per 2048 window starts, one bit per
 * window start and list), then compaction of the markers and of the run heads, each as counts per tile, an
 * exclusive scan and a scatter; only the runs (or the marks) travel home. */
typedef struct tbk_hit_run { uint64_t read, first, last; uint32_t markers, hap; } tbk_hit_run;  /* hap: 0 = A, 1 = B */
typedef struct tbk_hit_tracker tbk_hit_tracker;
int tbk_hit_tracker_create(tbk_table *hap_a, tbk_table *hap_b, tbk_hit_tracker **out);
void tbk_hit_tracker_destroy(tbk_hit_tracker *t);
/* The batch's runs ordered by (read, first), in memory of tbk_host_alloc: *runs is the caller's to tbk_host_free (NULL
 * when *n_runs is 0: an empty batch, reads shorter than k, no hit).  counts, when not NULL, gets the markers per read
 * and list (n_reads x 2, what tbk_classify_batch counts), added up from the runs. */
int tbk_hit_tracker_runs(tbk_hit_tracker *t, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int ignore_case,
                         tbk_hit_run **runs, uint64_t *n_runs, int32_t *counts);
/* One byte per base of the batch, in the batch's own coordinates: marks[offsets[r] + w] is 0 (none), 1 (A) or 2 (B)
 * for window start w of read r; the last k - 1 bytes of a read are 0. */
int tbk_hit_tracker_marks(tbk_hit_tracker *t, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int ignore_case,
                          uint8_t *marks);
/* The same in homopolymer-compressed space, for lists made of compressed k-mers, reported in the coordinates of the
 * batch as given.  The tracker owns one tbk_hpc session, made on first use; the batch goes through tbk_hpc_compress
 * with fold_case = ignore_case, and separation, marking, compaction and run extraction run on the compressed batch as
 * they do on a plain one.  Markers, runs and counts are those of the compressed batch (counts: what the classifier
 * counts in compressed mode); only the coordinates are lifted (tbk_hpc_lift above), on the device.  Of a lifted run,
 * first and last are the original positions of the first kept byte of its first and last marker's windows and end is
 * the original end of the last marker's window, all relative to the read as given: the run covers [first, end), and
 * end is the read's length when the window reaches the compressed end of the read.
 * tbk_hit_tracker_marks_compressed: one byte per base of the batch as given; a window's mark sits on the first base
 * of the window's first run, every other base is 0. */
typedef struct tbk_hit_run_lifted { uint64_t read, first, last, end; uint32_t markers, hap; } tbk_hit_run_lifted;
int tbk_hit_tracker_runs_compressed(tbk_hit_tracker *t, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int ignore_case,
                                    tbk_hit_run_lifted **runs, uint64_t *n_runs, int32_t *counts);
int tbk_hit_tracker_marks_compressed(tbk_hit_tracker *t, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int ignore_case,
                                     uint8_t *marks);

/* ---- database query: how often did the reads see the k-mers of a sequence? --------------- */
/* A query session scores sequences (an assembly's contigs) against ONE count database.  A window start of a sequence
 * is CLEAN when its k bases are all ACGT, either case: case is folded as the counter folds it (the database was
 * counted that way, so a database queried with its own reads finds them).  A clean window's k-mer is the counter's
 * canonical one - the lexicographic minimum of the window and its reverse complement - and its counter c is the
 * database's, 2..255, or 0 when the database does not hold it (a k-mer the reads hold once is in no floor-2 database;
 * a full database holds it, and c is then 1..255: wherever "max(2, min_count)" stands below, a full database has
 * max(1, min_count), so min_count = 1 counts presence).
 * The session borrows the database (it must outlive the session) and owns, on the database's device:
 *   - a DIRECTORY over the top P bits of the 2k-bit rank: 2^P + 1 32-bit offsets, dir[p] = the first entry whose
 *     rank has prefix >= p, built once at creation by one bisection per prefix.  P = floor(log2 n) - 1, so that a
 *     bucket holds 2 to 4 entries on average, at most 2k and at most 28: the directory takes 4 (2^P + 1) bytes -
 *     at most 2n + 4 beside the database's 9n for n >= 4, and never more than 1 GiB + 4.  A lookup reads two
 *     neighbouring offsets and bisects the bucket between them.  Offsets are 32 bits wide: a database of 2^32 or
 *     more entries is refused at creation (TBK_ERR_INVALID);
 *   - the SEEN bitmap, one bit per entry (n / 8 bytes): set when any clean window so far was that entry;
 *   - with copies != 0, COPIES, one 32-bit counter per entry (4n bytes): the clean windows so far that were that
 *     entry, whichever strand (a k-mer that is its own reverse complement counts once per window);
 *   - the HISTOGRAM of c over the clean windows so far (row 0: absent) and the running total of window starts;
 *   - batch buffers that grow to the largest batch seen.  One batch at a time per session.
 * A batch that would take the running total of window starts (sum of max(len - k + 1, 0)) past 2^32 - 1 is refused
 * with TBK_ERR_INVALID before anything is counted, so no copy counter can wrap.  An empty database (n = 0) is valid:
 * every window is absent.  TBK_ERR_NOMEM at creation leaves the database usable and *out NULL. */
typedef struct tbk_kmerdb_query tbk_kmerdb_query;
int tbk_kmerdb_query_create(const tbk_kmerdb *db, int copies, tbk_kmerdb_query **out);
void tbk_kmerdb_query_destroy(tbk_kmerdb_query *q);
/* Look up every window of a batch (reads back to back, offsets as for tbk_counter_add_batch) and add it to the
 * session's histogram, seen bits and copies.  per_read (n_reads x 2, may be NULL): the sequence's clean windows and,
 * of those, the FOUND ones, c >= max(2, min_count).  counts (may be NULL): one byte per base in the batch's own
 * coordinates, like tbk_hit_tracker_marks - counts[offsets[r] + w] = c of window w of read r, 0 for a window that is
 * absent or not clean; the last k - 1 bytes of a sequence are 0.  min_count does not change counts. */
int tbk_kmerdb_query_add(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t min_count,
                         uint64_t *per_read, uint8_t *counts);
/* The clean windows so far by counter; row 0: absent. */
int tbk_kmerdb_query_histogram(tbk_kmerdb_query *q, uint64_t hist[256]);
/* k-mer completeness: *solid = entries whose counter lies in [max(2, min_count), min(255, max_count)], *seen = those
 * of them that a window so far was. */
int tbk_kmerdb_query_completeness(tbk_kmerdb_query *q, uint32_t min_count, uint32_t max_count, uint64_t *seen, uint64_t *solid);
/* The copy spectrum: spec[min(copies, 5)][counter] = entries, over all n entries (rows 0..4: that many windows; row 5:
 * more than four).  TBK_ERR_INVALID for a session made without copies. */
int tbk_kmerdb_query_copy_spectrum(tbk_kmerdb_query *q, uint64_t spec[6][256]);
/* Clears seen, copies, the histogram and the window total: the next assembly against the same database. */
int tbk_kmerdb_query_reset(tbk_kmerdb_query *q);

/* ---- copy-number track: where do the reads' depth and the sequences' copies disagree? ---- */
/* A second pass over sequences (usually the ones the session was fed with tbk_kmerdb_query_add): per bin of `window`
 * window starts, the read depth, the copies the session has counted, and how many k-mers say "collapsed" or "duplicated".
 * q is a session made with copies != 0, k its database's k, peak >= 1 the read depth of a k-mer that the sequences
 * should hold once, window = W >= 1.
 * WINDOWS.  A sequence of length L has nw = max(L - k + 1, 0) window starts.  Clean windows, canonical k-mers and the
 * counter c (0 when absent) are exactly those of tbk_kmerdb_query_add.  For a present window (c >= 1), a is the entry's
 * copy counter in the session at the time of the call, a 32-bit value; it may be 0 when the sequence was never added.
 * BINS.  A sequence has ceil(nw / W) bins; bin b holds the window starts [b W, min((b + 1) W, nw)).  A sequence shorter
 * than k has no bins.
 * PER BIN:
 *   clean      clean windows in the bin;
 *   absent     clean windows with c == 0 (present = clean - absent);
 *   saturated  present windows with c == 255: the counter is capped there and no verdict is drawn from it;
 *   collapsed  present, c < 255 and 2c > (2a + 1) peak: the reads hold the k-mer more often than the sequences do;
 *   expanded   present, c < 255, a >= 1 and 2c < (2a - 1) peak: the sequences hold it more often than the reads do;
 *   depth      the lower median of c over the present windows - the lower median of m sorted values v is v[(m - 1) / 2] -
 *              and 0 when nothing is present;
 *   copies     the lower median of min(a, 255) over the present windows, 0 when there are none.
 * The verdicts are drawn in 64-bit integers, and a tie is consistent: with peak 10 and a = 1, c = 15 and c = 5 are
 * neither collapsed nor expanded.  (2c <= 508, so every peak above 508 draws the verdicts of 509: no collapse, and an
 * expansion wherever a >= 1.)
 * The call only reads the session: the histogram, the seen bits, the copies and the window total are as they were, and
 * the batch does not count towards the limit of 2^32 - 1 window starts.
 * bins is host memory: the bins of sequence 0 first, each sequence's in order; pad is written as 0.  n_bins must be
 * the sum of ceil(nw_r / window) over the sequences.  TBK_ERR_INVALID, with a message, for a session made without
 * copies, for window == 0 or peak == 0, and for an n_bins that is not that sum; nothing is written then and the session
 * stays usable.  n_reads == 0 or n_bins == 0 (with a matching sum) is valid and writes nothing.  An empty database is
 * valid: every clean window is absent.
 * The call uses the session's batch buffers and grows them as needed.  On the device it takes, per base of the batch
 * (rounded up to passes of 2048 stream positions, one position more per sequence): the bases and their separated copy
 * (2 bytes), c and min(a, 255) per stream position (2 bytes) and five bitmaps (5 bits) - 4.625 bytes, of which
 * tbk_kmerdb_query_add's own buffers already hold up to 3.25 - and 16 bytes per sequence and 24 per bin beside them. */
typedef struct tbk_depth_bin { uint32_t clean, absent, saturated, collapsed, expanded; uint8_t depth, copies, pad[2]; } tbk_depth_bin; /* 24 bytes */
int tbk_kmerdb_query_track(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                           uint32_t window, uint32_t peak, tbk_depth_bin *bins, uint64_t n_bins);

/* ---- repair candidates: which one-base edit mends each stretch of broken windows? ---------- */
/* A third pass over sequences: every maximal stretch of windows the database does not hold, and the one-base edits that
 * make every window over the edited position a k-mer the database holds.  q is a session with or without copies, k its
 * database's k, min_count in 1..255, min_support in 1..32.  The threshold is m = max(floor, min_count), floor 2 for a solid
 * database and 1 for a full one, as tbk_kmerdb_query_add has it.
 * WINDOWS AND STRETCHES.  Clean windows, case folding, canonical k-mers and the counter c are exactly those of
 * tbk_kmerdb_query_add.  A window is BROKEN when it is clean and c < m.  A STRETCH is a maximal run [f, l] of consecutive
 * broken window starts of one sequence, r = l - f + 1; its neighbours are found, not clean, or the sequence's ends.
 * Stretches never join across sequences.
 * CANDIDATES.  A stretch with r > k is LONG and is not attempted.  Otherwise every window of the stretch holds the
 * positions P = [l, f + k - 1] - k - r + 1 of them, all ACGT - and the gaps Q = [l + 1, f + k - 1], gap q in front of
 * base q.  With s the sequence, case folded:
 *   SUB(p, b)  p in P, b each of the three bases that differ from s[p];
 *   DEL(p)     p in P, unless p - 1 is in P and s[p-1] == s[p]: deleting any base of a run is one edit, left-aligned;
 *   INS(q, b)  q in Q, b in ACGT, unless q - 1 is in Q and s[q-1] == b: the same left alignment.
 * At most 8k - 4 candidates.
 * THE WINDOWS THAT COUNT, of the edited sequence s' of a sequence of length L:
 *   SUB  window starts max(0, p-k+1) .. min(p, L-k);
 *   DEL  those that hold both s'[p-1] and s'[p]: max(0, p-k+1) .. min(p-1, L-1-k); none for p = 0 or p = L-1;
 *   INS  those that hold s'[q]: max(0, q-k+1) .. min(q, L+1-k).
 * ACCEPTANCE.  Windows of s' that are not clean are skipped; support is the number of clean ones among them, depth the
 * smallest c among the clean ones.  A candidate is ACCEPTED when support >= min_support and every clean window has c >= m.
 * RESULT.  One record per stretch, ordered by (read, first), in memory of tbk_host_alloc: *repairs is the caller's to
 * tbk_host_free (NULL when there is no stretch).  first = f, windows = r, accepted = the number of accepted candidates;
 * kind is 0 NONE (attempted, nothing accepted), 1 SUB, 2 DEL, 3 INS or 4 LONG.  For kinds 1 to 3, pos (p, or q for an
 * insertion), base (the new base as upper-case ASCII, 0 for DEL), support and depth describe the accepted candidate that
 * is smallest by (kind, pos, base); for kinds 0 and 4 they are 0.  pad is 0.
 * The call only reads the session: the histogram, the seen bits, the copies and the window total are as they were, and
 * the batch does not count towards the limit of 2^32 - 1 window starts.  An empty database is valid: every clean window is
 * broken and nothing is accepted.  TBK_ERR_INVALID, with a message, for min_count outside 1..255 or min_support outside
 * 1..32 - nothing is written then and the session stays usable - and for a sequence of 2^32 or more bases.
 * The call uses the session's batch buffers and grows them as needed.  On the device it takes, per base of the batch
 * (rounded up to passes of 2048 stream positions, one position more per sequence): the bases and their separated copy
 * (2 bytes), the clean and the broken bitmap (2 bits) and, until the call returns, the compaction's flags (1 bit and 16
 * bytes per 1024 positions) - 2.39 bytes, of which tbk_kmerdb_query_add's own buffers already hold 2.25 - and 8 bytes per
 * sequence and 40 per stretch beside them. */
enum { TBK_REPAIR_NONE = 0, TBK_REPAIR_SUB = 1, TBK_REPAIR_DEL = 2, TBK_REPAIR_INS = 3, TBK_REPAIR_LONG = 4 };
typedef struct tbk_repair { uint64_t read, first, pos; uint32_t windows; uint16_t accepted;
                            uint8_t kind, base, support, depth, pad[6]; } tbk_repair;  /* 40 bytes, pad 0 */
int tbk_kmerdb_query_repairs(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                             uint32_t min_count, uint32_t min_support, tbk_repair **repairs, uint64_t *n_repairs);

/* ---- read evidence: how many of a read's k-mers does the database hold, and how much of it do they cover? ---------- */
/* A pass over reads that carries a database's k-mers back to them: per sequence, the windows the database holds with a
 * counter in a range, and the bases those windows cover.  q is a session with or without copies, k its database's k,
 * min_count in 1..255 and max_count in min_count..255.  The lower bound is m = max(floor, min_count), floor 2 for a solid
 * database and 1 for a full one, as the repair candidates have it.
 * WINDOWS.  A sequence of length L has nw = max(L - k + 1, 0) window starts.  Clean windows (ACGT only, either case),
 * canonical k-mers and the counter c are exactly those of tbk_kmerdb_query_add; c is 0 when the k-mer is absent.  A window
 * is HELD when it is clean and m <= c <= max_count.
 * COVERAGE.  A base position p in [0, L) is COVERED when some held window w has w <= p <= w + k - 1.  A held window starts
 * at L - k at most, so the last position any window covers is L - 1: coverage never reaches past a sequence's end, and
 * nothing joins across sequences.  (The evidence kernel relies on this: it dilates the held bits by k - 1 positions upward
 * and neither masks the result nor looks at the position behind the sequence.)
 * PER SEQUENCE:
 *   clean      clean windows;
 *   held       held windows;
 *   covered    covered positions;
 *   longest    the length of the longest run of consecutive covered positions, 0 when there is none;
 *   stretches  the number of maximal runs of consecutive covered positions.
 * A sequence shorter than k, or an empty one, gets five zeros.
 * out is host memory, one record per sequence in the batch's order.  TBK_ERR_INVALID, with a message, for min_count outside
 * 1..255 and for max_count outside min_count..255, before anything runs: nothing is written then and the session stays
 * usable.  A range that is empty after the floor - (1, 1) on a solid database - is valid and holds nothing.  n_reads == 0 is
 * valid and writes nothing.  An empty database is valid: no window is held.
 * The call only reads the session: the histogram, the seen bits, the copies and the window total are as they were, and
 * the batch does not count towards the limit of 2^32 - 1 window starts.
 * The call uses the session's batch buffers and grows them as needed.  On the device it takes, per base of the batch
 * (rounded up to passes of 2048 stream positions, one position more per sequence): the bases and their separated copy
 * (2 bytes) and the clean and the held bitmap (2 bits) - 2.25 bytes, all of which tbk_kmerdb_query_add's own buffers
 * already hold - and 8 bytes per sequence for the offsets and 40 for its record beside them.  No byte per base comes home. */
typedef struct tbk_read_evidence { uint64_t clean, held, covered, longest, stretches; } tbk_read_evidence; /* 40 bytes */
int tbk_kmerdb_query_evidence(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                              uint32_t min_count, uint32_t max_count, tbk_read_evidence *out /* n_reads */);

/* ---- read depth: how often did the library see a read's k-mers? --------------------------------------------------- */
/* A pass over reads that brings home, per sequence, a five-number summary of the counters of its windows: what kat sect,
 * BBNorm and khmer's normalize-by-median and filter-abund compute before they keep, drop or thin reads.  q is a session
 * with or without copies, k its database's k, min_count in 1..255.  The lower bound is m = max(floor, min_count), floor 2
 * for a solid database and 1 for a full one, as the read evidence has it.
 * WINDOWS AND DEPTHS.  A sequence of length L has nw = max(L - k + 1, 0) window starts.  Clean windows (ACGT only, either
 * case), canonical k-mers and the counter c are exactly those of tbk_kmerdb_query_add.  The DEPTH d of a clean window is c
 * when c >= m and 0 otherwise: an absent k-mer and a counter below m both read as depth 0.
 * PER SEQUENCE:
 *   clean           clean windows;
 *   present         clean windows with d >= 1;
 *   saturated       clean windows with d == 255: the counter stops there, so their true depth is 255 or more;
 *   sum             the sum of d over the clean windows - the mean depth is sum / clean, and no float is computed anywhere;
 *   lowest, q1, median, q3, highest
 *                   with the depths of the clean windows sorted ascending as v[0 .. clean - 1], these are
 *                   v[floor(j (clean - 1) / 4)] for j = 0 .. 4, the arithmetic in 64-bit integers: the minimum, the lower
 *                   quartile, the LOWER median (as tbk_depth_bin's depth is per bin), the upper quartile and the maximum;
 *   present_median  the same rank rule with j = 2 over the present windows only - v'[floor((present - 1) / 2)] of their sorted
 *                   depths - and 0 when there are none: the read's copy depth when most of its k-mers carry a sequencing
 *                   error and the median itself is 0;
 *   pad             two zero bytes.
 * A sequence without a clean window - an empty one, one shorter than k, one with an N in every window - gets an all-zero
 * record.
 * out is host memory, one record per sequence in the batch's order.  TBK_ERR_INVALID, with a message, before anything runs
 * and with nothing written, for min_count outside 1..255, for a NULL q or out, and for a sequence of 2^32 or more window
 * starts (the per-read kernel counts a sequence's depths in 32-bit rows); the session stays usable.  n_reads == 0 is valid
 * and writes nothing.  An empty database is valid: every depth is 0.
 * The call only reads the session: the histogram, the seen bits, the copies and the window total are as they were, and
 * the batch does not count towards the limit of 2^32 - 1 window starts.
 * The call uses the session's batch buffers and grows them as needed.  On the device it takes, per base of the batch
 * (rounded up to passes of 2048 stream positions, one position more per sequence): the bases and their separated copy
 * (2 bytes), the depth byte (1 byte) and the clean bitmap (1 bit) - 3.125 bytes, all in buffers that
 * tbk_kmerdb_query_add grows as well (the depth bytes in the one of its per-base counters) - and 8 bytes per sequence for
 * the offsets and 40 for its record beside them.  No byte per base comes home. */
typedef struct tbk_read_depth {
    uint64_t clean, present, saturated, sum;
    uint8_t  lowest, q1, median, q3, highest, present_median, pad[2];   /* pad 0 */
} tbk_read_depth;                                                        /* 40 bytes */
int tbk_kmerdb_query_read_depth(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets,
                                uint64_t n_reads, uint32_t min_count, tbk_read_depth *out /* n_reads */);

/* ---- read pieces: where along a read do the database's k-mers lie, and where do they not? ------------------------- */
/* The read evidence says how much of a sequence the held windows cover; this says where: the maximal runs of covered - or
 * of uncovered - positions as intervals, what khmer's trim-low-abund and BBDuk's ktrim and kmask work with.  q is a session
 * with or without copies, k its database's k, min_count in 1..255, max_count in min_count..255, side TBK_PIECES_COVERED or
 * _UNCOVERED, which TBK_PIECES_ALL or _LONGEST.
 * WINDOWS, HELD, COVERED.  Exactly as the read evidence defines them: clean windows (ACGT only, either case), canonical
 * k-mers, the counter c, the lower bound m = max(floor, min_count), a window HELD when it is clean and m <= c <= max_count,
 * a position p in [0, L) COVERED when some held window w has w <= p <= w + k - 1.  A base that is not ACGT lies in no clean
 * window and is therefore never covered.
 * SIDE.  Position p in [0, L) of a sequence is ON THE SIDE when it is covered (TBK_PIECES_COVERED) or when it is not
 * (TBK_PIECES_UNCOVERED).
 * PIECE.  A piece is a maximal run [first, end) of consecutive on-side positions of one sequence.  Pieces never join across
 * sequences.  An empty sequence has no piece.  A sequence shorter than k has none on the covered side and exactly one,
 * [0, L), on the uncovered side.
 * MIN_LENGTH.  Pieces with end - first < min_length are left out; 0 and 1 mean the same.
 * WHICH.  With TBK_PIECES_LONGEST only the longest of a sequence's pieces that passed min_length is returned; among equals
 * the one with the smallest first.
 * RESULT.  The records are ordered by (read, first), in memory of tbk_host_alloc: *pieces is the caller's to tbk_host_free
 * (NULL when there is no piece), as tbk_kmerdb_query_repairs returns its list.
 * EVIDENCE.  When evidence is not NULL it takes n_reads records, byte for byte what tbk_kmerdb_query_evidence writes for the
 * same arguments; they come from the same lookup pass, there is no second lookup.
 * The call only reads the session: the histogram, the seen bits, the copies and the window total are as they were, and the
 * batch does not count towards the limit of 2^32 - 1 window starts.  n_reads == 0 is valid and gives no piece.  An empty
 * database is valid: nothing is covered.  A range that is empty after the floor - (1, 1) on a solid database - is valid and
 * covers nothing.
 * TBK_ERR_INVALID, with a message, before anything runs and with nothing written - not *pieces, *n_pieces or evidence - for
 * min_count outside 1..255, max_count outside min_count..255, side > 1, which > 1, a NULL q, pieces or n_pieces, and a
 * sequence of 2^32 or more bases (the longest piece of a read is chosen by a 64-bit key of its length and its first
 * position, 32 bits each); the session stays usable.
 * The call uses the session's batch buffers and grows them as needed.  On the device it takes, per base of the batch
 * (rounded up to passes of 2048 stream positions, one position more per sequence): the bases and their separated copy
 * (2 bytes), the clean and the held bitmap (2 bits), the side bitmap (1 bit) and, until the call returns, the flags of the
 * two compactions of starts and ends (2 bits and 32 bytes per 1024 positions) - 2.66 bytes, of which
 * tbk_kmerdb_query_add's own buffers already hold 2.25.  Per sequence: 8 bytes for the offsets, 40 for the evidence record
 * when it is asked for and 8 for the key with TBK_PIECES_LONGEST.  Per piece of the batch before min_length and which are
 * applied: 24 bytes, and, when either leaves pieces out, 1 bit of flags and 24 bytes for every piece that stays.  A batch has
 * at most (bases + n_reads) / 2 pieces - a piece is one position at least and so is the gap behind it - and at most n_reads
 * come home with TBK_PIECES_LONGEST. */
enum { TBK_PIECES_COVERED = 0, TBK_PIECES_UNCOVERED = 1 };   /* side  */
enum { TBK_PIECES_ALL = 0, TBK_PIECES_LONGEST = 1 };         /* which */
typedef struct tbk_read_piece { uint64_t read, first, end; } tbk_read_piece;   /* 24 bytes; [first, end) */
int tbk_kmerdb_query_pieces(tbk_kmerdb_query *q, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                            uint32_t min_count, uint32_t max_count, uint32_t side, uint32_t which, uint64_t min_length,
                            tbk_read_evidence *evidence /* n_reads, may be NULL */,
                            tbk_read_piece **pieces, uint64_t *n_pieces);
/* The writer's side: a batch's records cut to their pieces.  Per read of the batch, in input order: bins[i] == 'A' sends
 * the read's pieces, in their order, to the first file - a read without a piece writes nothing; 'B' sends the read whole to
 * the second file and anything else sends it whole to the third, with the bytes tbk_bin_writer_write writes.
 * A piece [f, e) is written in the form tbk_bin_writer_write gives a record: FASTQ when the record has a non-empty quality
 * string, sequence and quality both cut to [f, e), else FASTA; the name is the header up to the first space.  With
 * suffix != 0 a piece that is not the whole record is renamed name:F-E, F = f + 1 and E = e (1-based and closed, as
 * samtools faidx names a region); a piece that is the whole record keeps the name, so a read that is kept untouched is the
 * same bytes as tbk_bin_writer_write's.  The text goes through the bins' buffers; gzip members are coded as for any bin,
 * by the host or the device.
 * TBK_ERR_INVALID for pieces that are not ordered by (read, first), that overlap, that are empty, that name a read the batch
 * does not have or that reach past a record's end; TBK_ERR_STATE for a BAM-bin or a haplotag writer and for a borrowed
 * batch.  Nothing is written in any of these cases.  The cut is the host's: the text of a record is gathered by the host for
 * every bin, and a device that rewrote record bytes lost to the host once the copy home was counted. */
int tbk_bin_writer_write_pieces(tbk_bin_writer *w, const tbk_fastx_batch *b, const tbk_read_piece *pieces, uint64_t n_pieces,
                                const char *bins /* per READ */, int suffix);

/* Host threads the library starts for its own host-side work (list parsing, gzip members,
 * scoring): hardware threads limited by the CPU affinity mask and the cgroup CPU quota, divided by the
 * number of ranks the launcher started on this node (LOCAL_WORLD_SIZE, or TBK_LOCAL_RANKS): one process per GPU
 * means N processes sharing the node's CPUs.  Env TBK_HOST_THREADS overrides. */
int tbk_host_threads(void);

/* ---- roofline calibration (SURVEY §8d "random-read roofline") -------------------------- */
/* Independent uniformly random line-aligned loads over a `footprint_bytes` buffer:
 * `line_bytes` in {64,128}, `lanes_per_line` in {1,4,8} (16 B per lane when >1, the whole
 * line per lane when 1), `loads_in_flight` per lane in 1..8.  Reports lines/s. */
int tbk_calib_gather(int device, uint64_t footprint_bytes, int line_bytes, int lanes_per_line,
                     int loads_in_flight, uint64_t n_lines, int reps, double *lines_per_sec,
                     double *ms_per_rep);
/* Fire-and-forget 32-bit atomic adds over a `footprint_bytes` buffer: each lane sends `run` (1..32)
 * consecutive adds to consecutive words of one random 128-byte line, then moves to another line.
 * The ceiling of the k-mer counting kernel (one add per k-mer occurrence). */
int tbk_calib_atomics(int device, uint64_t footprint_bytes, int run, int reps, double *atomics_per_sec);
/* The same with the instruction the counting kernel really issues: 64-bit adds that count two neighbouring 32-bit counters
 * at once, `run` (1..4) of them on the four counter words of one random line.  tbk_counter_adds_issued: how many of those
 * the kernel has sent so far - adds per second over this ceiling is the counting kernel's roofline fraction (<= 1). */
int tbk_calib_atomics64(int device, uint64_t footprint_bytes, int run, int reps, double *atomics_per_sec);
/* Streaming read of the same buffer (the 6.3 TB/s figure on this box). */
int tbk_calib_stream(int device, uint64_t footprint_bytes, int reps, double *bytes_per_sec);
/* The same two ceilings in tuned shapes (round 5: a yardstick must not sit below what it measures).  tbk_calib_gather_pairs: the
 * entry kernels' own request shape - one-wave blocks, `waves_per_simd` (1..8) of them resident per SIMD, two lanes x 16 bytes of a
 * line's first 32, `loads_in_flight` (1, 2, 3, 4, 6, 8) independent lines per pair before any is used.  tbk_calib_stream_nt:
 * `unroll` (1, 2, 4, 8) x 16 bytes per thread in flight, non-temporal loads, a grid of `blocks` x 256 threads.
 * tools/calib_ceilings.py sweeps both and writes profiles/calibration.json's ceilings. */
int tbk_calib_gather_pairs(int device, uint64_t footprint_bytes, int loads_in_flight, int waves_per_simd, uint64_t n_lines, int reps, double *lines_per_sec);
int tbk_calib_stream_nt(int device, uint64_t footprint_bytes, int unroll, int blocks, int reps, double *bytes_per_sec);

#ifdef __cplusplus
}
#endif
#endif /* TBK_H */
