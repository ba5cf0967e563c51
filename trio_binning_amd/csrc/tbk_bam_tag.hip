// tbk_bam_tag.hip — BAM records rewritten with their haplotype and counts as tags on the GPU (include/tbk.h "Haplotag
// output" has the rule, tbk_bam_tag.h the host pieces and the field walk the measure kernel shares with them).
//
// The plan is tbk_bam.hip's: measure, scan, output-tiled write.  Per run of records
//   1. tbk_tag_measure_kernel   one thread per record walks the aux area field by field, every step bounded by the record's
//                               end (a Z / H value is searched for its NUL in aligned words), and writes the tagged record's
//                               length and where the at most three fields it loses lie;
//   2. the exclusive scan of the lengths (tbk_launch_kmerdb_scan): where every tagged record begins, their size last;
//   3. tbk_tag_write_kernel     one block per tile of 4096 bytes of OUTPUT, a lane per aligned 16-byte vector.  A lane finds
//                               its record by bisecting the scanned offsets between the records of its tile's first and last
//                               byte.  A vector that lies in one stretch of a record's kept bytes is five aligned words of
//                               the input shifted into place; one that covers block_size', a lost field's place, the new
//                               tags or a record boundary is put together a byte at a time.
// A record that breaks the rule lowers one 64-bit word to (its index << 8 | reason) with a vector atomicMin: the first
// offender wins (the transcoder's rule).  Neither kernel strides: a thread per record, a block per tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/tbk.h"
#include "tbk_bam_tag.h"
#include "tbk_compact_host.h"

extern "C" void tbk_set_error_(int, const char *msg);

constexpr uint32_t TBK_TAG_TILE = 4096;   // bytes of output per tile: 256 lanes x 16

__global__ void __launch_bounds__(256)
tbk_tag_measure_kernel(const uint8_t *__restrict__ records, const uint64_t *__restrict__ offsets, uint64_t n, const char *__restrict__ bins,
                       unsigned long long *__restrict__ lengths, TbkTagDrops *__restrict__ drops, unsigned long long *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    TbkTagDrops d;
    uint32_t len = 0;
    const uint32_t why = tbk_tag_measure(records + offsets[i], bins[i], &d, &len);
    if (why != TBK_BAM_OK) atomicMin(&words[0], (unsigned long long)((i << 8) | why));
    lengths[i] = len;
    drops[i] = d;
}

namespace {
// the record a lane is writing (measured already)
struct TagCur {
    const uint8_t *rec;
    uint32_t kept_len;   // block_size field and the bytes kept: what comes before the new tags
    uint32_t new_bs;
    uint32_t at[3], len[3];
    uint32_t a, b;
    char bin;
    uint64_t start, end;   // of the tagged record in the output
};

__device__ __forceinline__ void tag_load(TagCur &c, const uint8_t *__restrict__ records, const uint64_t *__restrict__ offsets, const char *__restrict__ bins,
                                         const int32_t *__restrict__ counts, const TbkTagDrops *__restrict__ drops, const unsigned long long *__restrict__ out_off,
                                         uint64_t r) {
    const uint8_t *rec = records + offsets[r];
    c.rec = rec;
    const TbkTagDrops d = drops[r];
    uint32_t dropped = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) { c.at[k] = d.at[k]; c.len[k] = d.len[k]; dropped += d.len[k]; }
    c.kept_len = 4 + tbk_bam_u32(rec) - dropped;
    c.start = out_off[r];
    c.end = out_off[r + 1];
    c.new_bs = (uint32_t)(c.end - c.start) - 4;
    c.a = (uint32_t)counts[2 * r];
    c.b = (uint32_t)counts[2 * r + 1];
    c.bin = bins[r];
}

// where byte q (4 <= q < kept_len) of the tagged record lies in the input record: behind every lost field in front of it
__device__ __forceinline__ uint32_t tag_source(const TagCur &c, uint32_t q) {
    uint32_t p = q;
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (p >= c.at[k]) p += c.len[k];   // (an unused entry is {0, 0})
    return p;
}

// byte t of the new tags
__device__ __forceinline__ uint32_t tag_tail_byte(const TagCur &c, uint32_t t) {
    if (c.bin == 'A' || c.bin == 'B') {
        if (t < 4) return t == 0 ? 'H' : t == 1 ? 'P' : t == 2 ? 'C' : (c.bin == 'A' ? 1u : 2u);
        t -= 4;
    }
    const bool second = t >= 7;
    if (second) t -= 7;
    if (t < 3) return t == 0 ? 'k' : t == 1 ? (second ? 'b' : 'a') : 'I';
    return ((second ? c.b : c.a) >> (8 * (t - 3))) & 0xFFu;
}

__device__ __forceinline__ uint32_t tag_byte(const TagCur &c, uint32_t q) {
    if (q < 4) return (c.new_bs >> (8 * q)) & 0xFFu;
    if (q < c.kept_len) return c.rec[tag_source(c, q)];
    return tag_tail_byte(c, q - c.kept_len);
}
}  // namespace

// out_off: n + 1 scanned lengths, out_off[n] = out_len > 0.  records are readable 16 bytes past their end; dst is 16-byte
// aligned and holds out_len bytes.
__global__ void __launch_bounds__(256)
tbk_tag_write_kernel(const uint8_t *__restrict__ records, const uint64_t *__restrict__ offsets, const char *__restrict__ bins, const int32_t *__restrict__ counts,
                     const TbkTagDrops *__restrict__ drops, const unsigned long long *__restrict__ out_off, uint64_t n, uint64_t out_len, uint8_t *__restrict__ dst) {
    __shared__ uint64_t range[2];   // the records of the tile's first and last byte
    const uint64_t tile0 = (uint64_t)blockIdx.x * TBK_TAG_TILE;
    if (threadIdx.x < 2) {
        const uint64_t at = threadIdx.x == 0 ? tile0 : (tile0 + TBK_TAG_TILE - 1 < out_len - 1 ? tile0 + TBK_TAG_TILE - 1 : out_len - 1);
        uint64_t lo = 1, hi = n;   // first index in [1, n] whose offset lies behind `at` (out_off[n] = out_len does)
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (out_off[mid] > at) hi = mid; else lo = mid + 1;
        }
        range[threadIdx.x] = lo - 1;
    }
    __syncthreads();
    const uint64_t P = tile0 + (uint64_t)threadIdx.x * 16;
    if (P >= out_len) return;
    uint64_t r;
    {
        uint64_t lo = range[0] + 1, hi = range[1] + 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (out_off[mid] > P) hi = mid; else lo = mid + 1;
        }
        r = lo - 1;
    }
    TagCur c;
    tag_load(c, records, offsets, bins, counts, drops, out_off, r);
    const uint32_t valid = out_len - P >= 16 ? 16u : (uint32_t)(out_len - P);
    const uint32_t q = (uint32_t)(P - c.start);
    uint32_t o[4] = {0, 0, 0, 0};
    uint32_t p0 = 0;
    bool whole = q >= 4 && (uint64_t)q + 16 <= c.kept_len;
    if (whole) {
        p0 = tag_source(c, q);
        whole = tag_source(c, q + 15) == p0 + 15;   // no lost field in between
    }
    if (whole) {
        // sixteen kept bytes that lie together in the input, at any address: five aligned words, shifted
        const uint8_t *src = c.rec + p0;
        const uint32_t s = (uint32_t)((uintptr_t)src & 3u);
        const uint32_t *wp = reinterpret_cast<const uint32_t *>(src - s);
        uint32_t w[5];
#pragma unroll
        for (int k = 0; k < 5; k++) w[k] = wp[k];   // (w[4] lies within 4 bytes of the sixteen: the records' 16 spare bytes cover it)
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = (uint32_t)((((uint64_t)w[k + 1] << 32) | w[k]) >> (8 * s));
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
            if (j < valid) {
                if (P + j >= c.end) {
                    r++;   // (every tagged record has bytes; P + j < out_len = out_off[n])
                    tag_load(c, records, offsets, bins, counts, drops, out_off, r);
                }
                o[j >> 2] |= tag_byte(c, (uint32_t)(P + j - c.start)) << (8 * (j & 3u));
            }
        }
    }
    if (valid == 16) {
        *reinterpret_cast<uint4 *>(dst + P) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
            if (j < valid) dst[P + j] = (uint8_t)((o[j >> 2] >> (8 * (j & 3u))) & 0xFFu);
    }
}

// =======================================================================================
// the host side: a rewriter that keeps its buffers between batches (the bin writer, tbk_fastx.cpp) and the public one-shots
// =======================================================================================
namespace {
struct TagBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t need(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t c = n + n / 4 + 4096;
        const hipError_t e = hipMalloc(&p, c);
        if (e == hipSuccess) cap = c;
        return e;
    }
    void drop() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

int tfail(int code, const char *what, hipError_t e) {
    char buf[256];
    snprintf(buf, sizeof buf, "BAM haplotag rewriter: %s: %s", what, hipGetErrorString(e));
    tbk_set_error_(code, buf);
    (void)hipGetLastError();
    return code;
}
}  // namespace

struct tbk_bamtag {
    int device = 0;
    hipStream_t stream = nullptr;
    TagBuf d_records, d_offsets, d_bins, d_counts, d_lengths, d_out_off, d_drops, d_words, d_dst;
    uint64_t n = 0, out_len = 0;   // of the run measured last
};

int tbk_bamtag_create(int device, tbk_bamtag **out) {
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { (void)hipGetLastError(); tbk_set_error_(TBK_ERR_NO_DEVICE, "BAM haplotag rewriter: no such device"); return TBK_ERR_NO_DEVICE; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return tfail(TBK_ERR_HIP, "hipSetDevice", e);
    tbk_bamtag *t = new tbk_bamtag();
    t->device = device;
    e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = t->d_words.need(8);
    if (e != hipSuccess) { tbk_bamtag_destroy(t); return tfail(TBK_ERR_HIP, "setup", e); }
    *out = t;
    return TBK_OK;
}

void tbk_bamtag_destroy(tbk_bamtag *t) {
    if (!t) return;
    if (hipSetDevice(t->device) == hipSuccess) {
        if (t->stream) { (void)hipStreamSynchronize(t->stream); (void)hipStreamDestroy(t->stream); }
        for (TagBuf *x : {&t->d_records, &t->d_offsets, &t->d_bins, &t->d_counts, &t->d_lengths, &t->d_out_off, &t->d_drops, &t->d_words, &t->d_dst}) x->drop();
    }
    delete t;
}

// records, offsets, bins and counts to the device (d_records readable 16 bytes past `size`); asynchronous on the rewriter's stream
static int tag_copy_in(tbk_bamtag *t, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts) {
    hipError_t e = hipSetDevice(t->device);
    if (e == hipSuccess) e = t->d_records.need(size + 16);
    if (e == hipSuccess) e = t->d_offsets.need(n * 8);
    if (e == hipSuccess) e = t->d_bins.need(n);
    if (e == hipSuccess) e = t->d_counts.need(n * 8);
    if (e != hipSuccess) return tfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "buffers", e);
    e = hipMemcpyAsync(t->d_records.p, records, size, hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)t->d_records.p + size, 0, 16, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_offsets.p, offsets, n * 8, hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_bins.p, bins, n, hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_counts.p, counts, n * 8, hipMemcpyHostToDevice, t->stream);
    if (e != hipSuccess) return tfail(TBK_ERR_HIP, "copy in", e);
    return TBK_OK;
}

// The run that lies on the device measured and scanned: *out_len and *bad come home.
static int tag_measure(tbk_bamtag *t, uint64_t n, uint64_t *out_len, uint64_t *bad) {
    *out_len = 0; *bad = TBK_BAM_NO_BAD;
    t->n = n; t->out_len = 0;
    if (n > 0x7FFFFFFFull * 256) { tbk_set_error_(TBK_ERR_INVALID, "BAM haplotag rewriter: too many records in a run"); return TBK_ERR_INVALID; }
    hipError_t e = hipSetDevice(t->device);
    if (e == hipSuccess) e = t->d_lengths.need((n + 1) * 8);
    if (e == hipSuccess) e = t->d_out_off.need((n + 1) * 8);
    if (e == hipSuccess) e = t->d_drops.need(n * sizeof(TbkTagDrops));
    if (e != hipSuccess) return tfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "buffers", e);
    unsigned long long *d_words = (unsigned long long *)t->d_words.p, *d_lengths = (unsigned long long *)t->d_lengths.p, *d_out_off = (unsigned long long *)t->d_out_off.p;
    e = hipMemsetAsync(d_words, 0xFF, 8, t->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_lengths + n, 0, 8, t->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tbk_tag_measure_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t->stream, (const uint8_t *)t->d_records.p, (const uint64_t *)t->d_offsets.p, n,
                           (const char *)t->d_bins.p, d_lengths, (TbkTagDrops *)t->d_drops.p, d_words);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = tbk_launch_kmerdb_scan(d_lengths, d_out_off, n + 1, t->stream);
    unsigned long long home[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&home[0], d_words, 8, hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&home[1], d_out_off + n, 8, hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return tfail(TBK_ERR_HIP, "measure", e);
    *bad = home[0];
    if (home[0] == TBK_BAM_NO_BAD) { *out_len = home[1]; t->out_len = home[1]; }
    return TBK_OK;
}

// The tagged records of the run measured last into d_dst (out_len bytes).  Asynchronous on the rewriter's stream.
static int tag_write(tbk_bamtag *t) {
    if (!t->out_len) return TBK_OK;
    const uint64_t tiles = (t->out_len + TBK_TAG_TILE - 1) / TBK_TAG_TILE;
    if (tiles > 0x7FFFFFFFull) { tbk_set_error_(TBK_ERR_INVALID, "BAM haplotag rewriter: a run's records are too long"); return TBK_ERR_INVALID; }
    hipLaunchKernelGGL(tbk_tag_write_kernel, dim3((unsigned)tiles), dim3(256), 0, t->stream, (const uint8_t *)t->d_records.p, (const uint64_t *)t->d_offsets.p,
                       (const char *)t->d_bins.p, (const int32_t *)t->d_counts.p, (const TbkTagDrops *)t->d_drops.p, (const unsigned long long *)t->d_out_off.p, t->n, t->out_len,
                       (uint8_t *)t->d_dst.p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tfail(TBK_ERR_HIP, "launch", e);
    return TBK_OK;
}

int tbk_bamtag_run(tbk_bamtag *t, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts, uint8_t *dst,
                   uint64_t cap, uint64_t *out_off, uint64_t *out_len, uint64_t *bad) {
    *out_len = 0; *bad = TBK_BAM_NO_BAD;
    if (out_off) out_off[0] = 0;
    if (!n) return TBK_OK;
    int rc = tag_copy_in(t, records, size, offsets, n, bins, counts);
    if (!rc) rc = tag_measure(t, n, out_len, bad);
    if (rc || *bad != TBK_BAM_NO_BAD) return rc;
    if (*out_len > cap || !dst) { tbk_set_error_(TBK_ERR_NOMEM, "BAM haplotag rewriter: dst too small"); return TBK_ERR_NOMEM; }
    hipError_t e = t->d_dst.need(*out_len + 16);
    if (e != hipSuccess) return tfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "buffers", e);
    if ((rc = tag_write(t))) return rc;
    e = hipMemcpyAsync(dst, t->d_dst.p, *out_len, hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess && out_off) e = hipMemcpyAsync(out_off, t->d_out_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return tfail(TBK_ERR_HIP, "records home", e);
    return TBK_OK;
}

static int tag_refuse(const char *who, uint64_t bad) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: BAM record %llu: %s", who, (unsigned long long)(bad >> 8), tbk_tag_reason((uint32_t)(bad & 0xFFu)));
    tbk_set_error_(TBK_ERR_FORMAT, buf);
    return TBK_ERR_FORMAT;
}

// The arguments every entry point checks the same way: pointers, offsets that name whole records of the run (the kernels
// trust them), counts that are not negative.
static int tag_check_args(const char *who, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts,
                          uint64_t *out_len) {
    char buf[200];
    if (!out_len || (n && (!records || !offsets || !bins || !counts))) { snprintf(buf, sizeof buf, "%s: NULL argument", who); tbk_set_error_(TBK_ERR_INVALID, buf); return TBK_ERR_INVALID; }
    *out_len = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t p = offsets[i];
        if (p > size || size - p < 36 || tbk_bam_u32(records + p) < 32 || (uint64_t)tbk_bam_u32(records + p) > size - p - 4) {
            snprintf(buf, sizeof buf, "%s: offsets[%llu] names no whole record of the run", who, (unsigned long long)i);
            tbk_set_error_(TBK_ERR_INVALID, buf);
            return TBK_ERR_INVALID;
        }
        if (counts[2 * i] < 0 || counts[2 * i + 1] < 0) {
            snprintf(buf, sizeof buf, "%s: record %llu has a count below 0", who, (unsigned long long)i);
            tbk_set_error_(TBK_ERR_INVALID, buf);
            return TBK_ERR_INVALID;
        }
    }
    return TBK_OK;
}

extern "C" int tbk_bam_haplotag_device(int device, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts,
                                       uint8_t *dst, uint64_t cap, uint64_t *out_off, uint64_t *out_len) {
    int rc = tag_check_args("tbk_bam_haplotag_device", records, size, offsets, n, bins, counts, out_len);
    if (rc) return rc;
    tbk_bamtag *t = nullptr;
    if ((rc = tbk_bamtag_create(device, &t))) return rc;
    uint64_t bad = TBK_BAM_NO_BAD;
    rc = tbk_bamtag_run(t, records, size, offsets, n, bins, counts, dst, cap, out_off, out_len, &bad);
    if (!rc && bad != TBK_BAM_NO_BAD) rc = tag_refuse("tbk_bam_haplotag_device", bad);
    tbk_bamtag_destroy(t);
    return rc;
}

// The same through the plain C++ of tbk_bam_tag.h on the host's threads (tbk_host_threads): the second opinion on the kernels,
// and what the writer runs without a device.
extern "C" int tbk_bam_haplotag(const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts, uint8_t *dst,
                                uint64_t cap, uint64_t *out_off, uint64_t *out_len) {
    const int rc = tag_check_args("tbk_bam_haplotag", records, size, offsets, n, bins, counts, out_len);
    if (rc) return rc;
    bool fits = true;
    const uint64_t bad = tbk_bam_haplotag_host(records, offsets, n, bins, counts, dst, cap, out_off, out_len, &fits, tbk_host_threads());
    if (bad != TBK_BAM_NO_BAD) { *out_len = 0; return tag_refuse("tbk_bam_haplotag", bad); }
    if (!fits) { tbk_set_error_(TBK_ERR_NOMEM, "tbk_bam_haplotag: dst too small"); return TBK_ERR_NOMEM; }
    return TBK_OK;
}

// The kernels timed by themselves (tools/measure_haplotag.py).  The run is copied to the device once and stays there; after a
// warm-up, `reps` times: whole_s[i] = measure kernel, scan, the size brought home and the write kernel, wall clock around the
// calls with the stream idle before and after; write_s[i] = the write kernel alone between two HIP events; call_s[i] (may be
// NULL) = what the bin writer pays per batch with its buffers warm: copy in, kernels, records and offsets home into pageable memory.
extern "C" int tbk_bam_haplotag_bench_device(int device, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins,
                                             const int32_t *counts, int reps, double *whole_s, double *write_s, double *call_s, uint64_t *out_len) {
    int rc = tag_check_args("tbk_bam_haplotag_bench_device", records, size, offsets, n, bins, counts, out_len);
    if (rc) return rc;
    if (!n || reps < 1 || !whole_s || !write_s) { tbk_set_error_(TBK_ERR_INVALID, "tbk_bam_haplotag_bench_device: bad argument"); return TBK_ERR_INVALID; }
    tbk_bamtag *t = nullptr;
    if ((rc = tbk_bamtag_create(device, &t))) return rc;
    uint64_t bad = TBK_BAM_NO_BAD;
    std::vector<uint8_t> home((size_t)(size + TBK_TAG_GROWTH * n));
    std::vector<uint64_t> home_off((size_t)n + 1);
    rc = tbk_bamtag_run(t, records, size, offsets, n, bins, counts, home.data(), home.size(), home_off.data(), out_len, &bad);
    if (!rc && bad != TBK_BAM_NO_BAD) rc = tag_refuse("tbk_bam_haplotag_bench_device", bad);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipSuccess;
    if (!rc) e = hipEventCreate(&e0);
    if (!rc && e == hipSuccess) e = hipEventCreate(&e1);
    if (!rc && e != hipSuccess) rc = tfail(TBK_ERR_HIP, "events", e);
    for (int i = -1; i < reps && !rc; i++) {   // (-1: the warm-up)
        auto t0 = std::chrono::steady_clock::now();
        rc = tag_measure(t, n, out_len, &bad);
        if (!rc) rc = tag_write(t);
        if (!rc && (e = hipStreamSynchronize(t->stream)) != hipSuccess) rc = tfail(TBK_ERR_HIP, "bench", e);
        const double whole = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        float ms = 0;
        if (!rc) {
            e = hipEventRecord(e0, t->stream);
            if (e == hipSuccess) rc = tag_write(t);
            if (e == hipSuccess && !rc) e = hipEventRecord(e1, t->stream);
            if (e == hipSuccess && !rc) e = hipEventSynchronize(e1);
            if (e == hipSuccess && !rc) e = hipEventElapsedTime(&ms, e0, e1);
            if (!rc && e != hipSuccess) rc = tfail(TBK_ERR_HIP, "timing", e);
        }
        double call = 0;
        if (!rc && call_s) {
            t0 = std::chrono::steady_clock::now();
            rc = tbk_bamtag_run(t, records, size, offsets, n, bins, counts, home.data(), home.size(), home_off.data(), out_len, &bad);
            call = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        if (i >= 0) { whole_s[i] = whole; write_s[i] = ms / 1e3; if (call_s) call_s[i] = call; }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    tbk_bamtag_destroy(t);
    return rc;
}
