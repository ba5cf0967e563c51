// tbk_bam.hip — a window of unaligned BAM records turned into FASTQ text on the GPU (include/tbk.h "BAM input" has the
// rule, tbk_bam.h the host pieces and the record check the measure kernel shares with them).
//
// The host has walked the block_size chain (tbk_bam_index: one dependent 4-byte read per record), so the window comes
// with the offset of every record.  Per window
//   1. tbk_bam_measure_kernel   one thread per record: the fixed part, the name and qual[0] are read and checked, and the
//                               record's text length is written - 0 for a record that is skipped;
//   2. the exclusive scan of the lengths (tbk_launch_kmerdb_scan): where every record's text begins, the text's size last;
//   3. tbk_bam_fastq_kernel     one block per tile of 4096 bytes of OUTPUT, a lane per aligned 16-byte vector.  Every
//                               output byte is a function of (record, position in the record's text), so the work is
//                               the same whatever the read lengths are.  A lane finds its record by bisecting the scanned
//                               offsets between the records of its tile's first and last byte, and goes on to the next
//                               records when its vector covers the end of one and the start of others.
// A record that breaks the rule lowers one 64-bit word to (its index << 8 | reason) with a vector atomicMin: the first
// offender wins (tbk_dump.hip's rule).  No block waits for another; the other atomics are two counters, one add per wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/tbk.h"
#include "tbk_bam.h"
#include "tbk_compact_host.h"

extern "C" void tbk_set_error_(int, const char *msg);

static_assert(TBK_BAM_MAX_RECORD == TBK_BAM_MAX_RECORD_, "tbk_bam.h restates the public bound");
constexpr uint32_t TBK_BAM_TILE = 4096;   // bytes of text per tile: 256 lanes x 16

__global__ void __launch_bounds__(256)
tbk_bam_measure_kernel(const uint8_t *__restrict__ records, const uint64_t *__restrict__ offsets, uint64_t n, uint32_t skip_flags, uint64_t first_record,
                       unsigned long long *__restrict__ lengths, unsigned long long *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t len = 0, why = TBK_BAM_OK;
    const bool in = i < n;
    if (in) {
        TbkBamRec r;
        why = tbk_bam_measure(records + offsets[i], skip_flags, &r, &len);
        if (why != TBK_BAM_OK) atomicMin(&words[0], (unsigned long long)(((first_record + i) << 8) | why));
        lengths[i] = len;
    }
    // words[1]: records written, words[2]: records skipped
    const unsigned long long wrote = __ballot(in && why == TBK_BAM_OK && len > 0), skipped = __ballot(in && why == TBK_BAM_OK && len == 0);
    if ((threadIdx.x & 63u) == 0) {
        if (wrote) atomicAdd(&words[1], (unsigned long long)__popcll(wrote));
        if (skipped) atomicAdd(&words[2], (unsigned long long)__popcll(skipped));
    }
}

namespace {
// the record a lane is writing: what its text depends on (checked by the measure kernel already)
struct BamCur {
    const uint8_t *rec;
    uint32_t name_len, l_seq, seq_at, qual_at;
    bool has_qual, rev;
    uint64_t start, end;   // of its text
};

constexpr uint64_t bam_pack8(const char *s) {
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)(uint8_t)s[i] << (8 * i);
    return v;
}
constexpr uint64_t BAM_FWD_LO = bam_pack8("=ACMGRSV"), BAM_FWD_HI = bam_pack8("TWYHKDBN");
constexpr uint64_t BAM_REV_LO = bam_pack8("=TGKCYSB"), BAM_REV_HI = bam_pack8("AWRDMHVN");

__device__ __forceinline__ void bam_load(BamCur &c, const uint8_t *__restrict__ records, const uint64_t *__restrict__ offsets,
                                         const unsigned long long *__restrict__ text_off, uint64_t r) {
    const uint8_t *rec = records + offsets[r];
    c.rec = rec;
    c.name_len = (uint32_t)rec[12] - 1;
    c.l_seq = tbk_bam_u32(rec + 20);
    c.seq_at = 36 + c.name_len + 1 + 4 * tbk_bam_u16(rec + 16);
    c.qual_at = c.seq_at + (c.l_seq + 1) / 2;
    c.has_qual = rec[c.qual_at] != 0xFF;
    c.rev = (tbk_bam_u16(rec + 18) & 0x10u) != 0;
    c.start = text_off[r];
    c.end = text_off[r + 1];
}

// the letter of a 4-bit code: a 16-entry table in two 64-bit registers
__device__ __forceinline__ uint32_t bam_letter(uint32_t code, uint64_t lo, uint64_t hi) {
    return (uint32_t)(((code & 8u) ? hi : lo) >> (8 * (code & 7u))) & 0xFFu;
}

// byte q of the record's text
__device__ __forceinline__ uint32_t bam_text_byte(const BamCur &c, uint32_t q) {
    if (q == 0) return c.has_qual ? '@' : '>';
    if (q <= c.name_len) return c.rec[36 + q - 1];
    uint32_t s = q - c.name_len - 1;   // 0: the newline behind the name
    if (s == 0) return '\n';
    s -= 1;
    if (s < c.l_seq) {
        const uint32_t i = c.rev ? c.l_seq - 1 - s : s;
        const uint32_t code = ((uint32_t)c.rec[c.seq_at + (i >> 1)] >> (4 * (1 - (i & 1)))) & 15u;
        return c.rev ? bam_letter(code, BAM_REV_LO, BAM_REV_HI) : bam_letter(code, BAM_FWD_LO, BAM_FWD_HI);
    }
    s -= c.l_seq;   // 0: newline, 1: '+', 2: newline, then the qualities and a newline
    if (s == 1) return '+';
    if (s < 3) return '\n';
    s -= 3;
    if (s < c.l_seq) {
        const uint32_t v = c.rec[c.qual_at + (c.rev ? c.l_seq - 1 - s : s)];
        return (v > 93u ? 93u : v) + 33u;
    }
    return '\n';
}

// min(byte, 93) + 33 in each byte of a word
__device__ __forceinline__ uint32_t bam_qual4(uint32_t w) {
    const uint32_t over = (((w & 0x7F7F7F7Fu) + 0x22222222u) | w) & 0x80808080u;   // 0x80 where the byte is 94 or more (0x22 = 128 - 94)
    const uint32_t mask = (over >> 7) * 0xFFu;
    return ((w & ~mask) | (0x5D5D5D5Du & mask)) + 0x21212121u;
}
}  // namespace

// text_off: n + 1 scanned lengths, text_off[n] = text_len.  records are readable 16 bytes past their end; text is 16-byte
// aligned and holds text_len bytes.
__global__ void __launch_bounds__(256)
tbk_bam_fastq_kernel(const uint8_t *__restrict__ records, const uint64_t *__restrict__ offsets, const unsigned long long *__restrict__ text_off, uint64_t n,
                     uint64_t text_len, uint8_t *__restrict__ text) {
    __shared__ uint64_t range[2];   // the records of the tile's first and last byte
    const uint64_t tile0 = (uint64_t)blockIdx.x * TBK_BAM_TILE;
    if (threadIdx.x < 2) {
        const uint64_t at = threadIdx.x == 0 ? tile0 : (tile0 + TBK_BAM_TILE - 1 < text_len - 1 ? tile0 + TBK_BAM_TILE - 1 : text_len - 1);
        uint64_t lo = 1, hi = n;   // first index in [1, n] whose offset lies behind `at` (text_off[n] = text_len does)
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (text_off[mid] > at) hi = mid; else lo = mid + 1;
        }
        range[threadIdx.x] = lo - 1;
    }
    __syncthreads();
    const uint64_t P = tile0 + (uint64_t)threadIdx.x * 16;
    if (P >= text_len) return;
    uint64_t r;
    {
        uint64_t lo = range[0] + 1, hi = range[1] + 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (text_off[mid] > P) hi = mid; else lo = mid + 1;
        }
        r = lo - 1;
    }
    BamCur c;
    bam_load(c, records, offsets, text_off, r);
    const uint32_t valid = text_len - P >= 16 ? 16u : (uint32_t)(text_len - P);
    const uint32_t q = (uint32_t)(P - c.start);
    const uint32_t seq0 = c.name_len + 2, qual0 = seq0 + c.l_seq + 3;
    uint64_t out_lo = 0, out_hi = 0;
    if (c.end - P >= 16 && q >= seq0 && q - seq0 + 16 <= c.l_seq) {
        // sixteen letters from 8 or 9 bytes of seq: the nibbles in base order (a byte's high nibble is the earlier base), a code at a time
        // through the table in registers
        const uint32_t i0 = q - seq0;
        const uint32_t low = c.rev ? c.l_seq - 16 - i0 : i0;   // the lowest of the sixteen bases' indices
        const uint8_t *sp = c.rec + c.seq_at + (low >> 1);
        uint64_t b;
        __builtin_memcpy(&b, sp, 8);
        b = ((b & 0x0F0F0F0F0F0F0F0Full) << 4) | ((b >> 4) & 0x0F0F0F0F0F0F0F0Full);   // nibble g of the bytes at bits 4g
        if (low & 1u) b = (b >> 4) | ((uint64_t)(sp[8] >> 4) << 60);
        if (c.rev) {
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) {
                const uint64_t l = bam_letter((uint32_t)(b >> (4 * (15 - k))) & 15u, BAM_REV_LO, BAM_REV_HI);
                if (k < 8) out_lo |= l << (8 * k); else out_hi |= l << (8 * (k - 8));
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) {
                const uint64_t l = bam_letter((uint32_t)(b >> (4 * k)) & 15u, BAM_FWD_LO, BAM_FWD_HI);
                if (k < 8) out_lo |= l << (8 * k); else out_hi |= l << (8 * (k - 8));
            }
        }
    } else if (c.end - P >= 16 && c.has_qual && q >= qual0 && q - qual0 + 16 <= c.l_seq) {
        // sixteen qualities, clamped and raised four at a time
        const uint32_t t0 = q - qual0;
        const uint8_t *qp = c.rec + c.qual_at + (c.rev ? c.l_seq - 16 - t0 : t0);
        uint32_t a0, a1, a2, a3;
        __builtin_memcpy(&a0, qp, 4);
        __builtin_memcpy(&a1, qp + 4, 4);
        __builtin_memcpy(&a2, qp + 8, 4);
        __builtin_memcpy(&a3, qp + 12, 4);
        a0 = bam_qual4(a0); a1 = bam_qual4(a1); a2 = bam_qual4(a2); a3 = bam_qual4(a3);
        if (c.rev) {
            out_lo = (uint64_t)__builtin_bswap32(a3) | ((uint64_t)__builtin_bswap32(a2) << 32);
            out_hi = (uint64_t)__builtin_bswap32(a1) | ((uint64_t)__builtin_bswap32(a0) << 32);
        } else {
            out_lo = (uint64_t)a0 | ((uint64_t)a1 << 32);
            out_hi = (uint64_t)a2 | ((uint64_t)a3 << 32);
        }
    } else {
        // names, separators, the ends of seq and qual, and vectors that cover more than one record: a byte at a time
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
            if (j < valid) {
                if (P + j >= c.end) {
                    do r++; while (P + j >= text_off[r + 1]);   // (skipped records have no text; P + j < text_len = text_off[n])
                    bam_load(c, records, offsets, text_off, r);
                }
                const uint64_t v = bam_text_byte(c, (uint32_t)(P + j - c.start));
                if (j < 8) out_lo |= v << (8 * j); else out_hi |= v << (8 * (j - 8));
            }
        }
    }
    if (valid == 16) {
        *reinterpret_cast<uint4 *>(text + P) = make_uint4((uint32_t)out_lo, (uint32_t)(out_lo >> 32), (uint32_t)out_hi, (uint32_t)(out_hi >> 32));
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
            if (j < valid) text[P + j] = (uint8_t)((j < 8 ? out_lo >> (8 * j) : out_hi >> (8 * (j - 8))) & 0xFFu);
    }
}

// =======================================================================================
// the host side: a transcoder that keeps its buffers between windows (the reader's BAM loop, tbk_fastx.cpp) and the
// public one-shot
// =======================================================================================
namespace {
struct BamBuf {
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

int bfail(int code, const char *what, hipError_t e) {
    char buf[256];
    snprintf(buf, sizeof buf, "BAM transcoder: %s: %s", what, hipGetErrorString(e));
    tbk_set_error_(code, buf);
    (void)hipGetLastError();
    return code;
}
}  // namespace

struct tbk_bamdev {
    int device = 0;
    hipStream_t stream = nullptr;
    BamBuf d_records, d_offsets, d_lengths, d_text_off, d_words, d_text;
    uint64_t n = 0, text_len = 0;   // of the window measured last
};

int tbk_bamdev_create(int device, tbk_bamdev **out) {
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { (void)hipGetLastError(); tbk_set_error_(TBK_ERR_NO_DEVICE, "BAM transcoder: no such device"); return TBK_ERR_NO_DEVICE; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return bfail(TBK_ERR_HIP, "hipSetDevice", e);
    tbk_bamdev *b = new tbk_bamdev();
    b->device = device;
    e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = b->d_words.need(3 * 8);
    if (e != hipSuccess) { delete b; return bfail(TBK_ERR_HIP, "setup", e); }
    *out = b;
    return TBK_OK;
}

void tbk_bamdev_destroy(tbk_bamdev *b) {
    if (!b) return;
    if (hipSetDevice(b->device) == hipSuccess) {
        if (b->stream) { (void)hipStreamSynchronize(b->stream); (void)hipStreamDestroy(b->stream); }
        for (BamBuf *x : {&b->d_records, &b->d_offsets, &b->d_lengths, &b->d_text_off, &b->d_words, &b->d_text}) x->drop();
    }
    delete b;
}

// The form the kernels are driven in: records and offsets lie on the device (d_records readable 16 bytes past `size`).
// Measures and scans; the answers come home: *text_len, the counts, *bad = TBK_BAM_NO_BAD or (first_record + index << 8 | reason).
int tbk_bamdev_measure_device(tbk_bamdev *b, const uint8_t *d_records, const uint64_t *d_offsets, uint64_t n, uint32_t skip_flags, uint64_t first_record,
                              uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped, uint64_t *bad) {
    *text_len = 0; *n_written = 0; *n_skipped = 0; *bad = TBK_BAM_NO_BAD;
    b->n = n; b->text_len = 0;
    if (!n) return TBK_OK;
    if (n > 0x7FFFFFFFull * 256) { tbk_set_error_(TBK_ERR_INVALID, "BAM transcoder: too many records in a window"); return TBK_ERR_INVALID; }
    hipError_t e = hipSetDevice(b->device);
    if (e == hipSuccess) e = b->d_lengths.need((n + 1) * 8);
    if (e == hipSuccess) e = b->d_text_off.need((n + 1) * 8);
    if (e != hipSuccess) return bfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "buffers", e);
    unsigned long long *d_words = (unsigned long long *)b->d_words.p, *d_lengths = (unsigned long long *)b->d_lengths.p, *d_text_off = (unsigned long long *)b->d_text_off.p;
    e = hipMemsetAsync(d_words, 0xFF, 8, b->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_words + 1, 0, 16, b->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_lengths + n, 0, 8, b->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tbk_bam_measure_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, d_records, d_offsets, n, skip_flags, first_record, d_lengths, d_words);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = tbk_launch_kmerdb_scan(d_lengths, d_text_off, n + 1, b->stream);
    unsigned long long home[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&home[0], d_words, 24, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&home[3], d_text_off + n, 8, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return bfail(TBK_ERR_HIP, "measure", e);
    *bad = home[0]; *n_written = home[1]; *n_skipped = home[2]; *text_len = home[3];
    if (home[0] == TBK_BAM_NO_BAD) b->text_len = home[3];
    return TBK_OK;
}

// The text of the window measured last, into d_text (16-byte aligned, text_len bytes).  Asynchronous on the transcoder's stream.
int tbk_bamdev_write_device(tbk_bamdev *b, const uint8_t *d_records, const uint64_t *d_offsets, uint8_t *d_text) {
    if (!b->text_len) return TBK_OK;
    const uint64_t tiles = (b->text_len + TBK_BAM_TILE - 1) / TBK_BAM_TILE;
    if (tiles > 0x7FFFFFFFull) { tbk_set_error_(TBK_ERR_INVALID, "BAM transcoder: a window's text is too long"); return TBK_ERR_INVALID; }
    hipLaunchKernelGGL(tbk_bam_fastq_kernel, dim3((unsigned)tiles), dim3(256), 0, b->stream, d_records, d_offsets, (const unsigned long long *)b->d_text_off.p, b->n, b->text_len,
                       d_text);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bfail(TBK_ERR_HIP, "launch", e);
    return TBK_OK;
}

int tbk_bamdev_time_write(tbk_bamdev *b, double *seconds) {
    *seconds = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    hipError_t e = hipSetDevice(b->device);
    if (e == hipSuccess) e = hipEventCreate(&t0);
    if (e == hipSuccess) e = hipEventCreate(&t1);
    if (e == hipSuccess) e = hipEventRecord(t0, b->stream);
    int rc = TBK_OK;
    if (e == hipSuccess) rc = tbk_bamdev_write_device(b, (const uint8_t *)b->d_records.p, (const uint64_t *)b->d_offsets.p, (uint8_t *)b->d_text.p);
    if (e == hipSuccess && !rc) e = hipEventRecord(t1, b->stream);
    if (e == hipSuccess && !rc) e = hipEventSynchronize(t1);
    float ms = 0;
    if (e == hipSuccess && !rc) e = hipEventElapsedTime(&ms, t0, t1);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (rc) return rc;
    if (e != hipSuccess) return bfail(TBK_ERR_HIP, "timing", e);
    *seconds = ms / 1e3;
    return TBK_OK;
}

// From host memory: the window goes to the device and is measured ...
int tbk_bamdev_measure(tbk_bamdev *b, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, uint64_t first_record,
                       uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped, uint64_t *bad) {
    *text_len = 0; *n_written = 0; *n_skipped = 0; *bad = TBK_BAM_NO_BAD;
    b->n = n; b->text_len = 0;
    if (!n) return TBK_OK;
    hipError_t e = hipSetDevice(b->device);
    if (e == hipSuccess) e = b->d_records.need(size + 16);
    if (e == hipSuccess) e = b->d_offsets.need(n * 8);
    if (e != hipSuccess) return bfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "buffers", e);
    e = hipMemcpyAsync(b->d_records.p, records, size, hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)b->d_records.p + size, 0, 16, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_offsets.p, offsets, n * 8, hipMemcpyHostToDevice, b->stream);
    if (e != hipSuccess) return bfail(TBK_ERR_HIP, "copy in", e);
    return tbk_bamdev_measure_device(b, (const uint8_t *)b->d_records.p, (const uint64_t *)b->d_offsets.p, n, skip_flags, first_record, text_len, n_written, n_skipped, bad);
}

// ... and its text comes home into dst (at least the measured text_len bytes).
int tbk_bamdev_write(tbk_bamdev *b, uint8_t *dst) {
    if (!b->text_len) return TBK_OK;
    hipError_t e = hipSetDevice(b->device);
    if (e == hipSuccess) e = b->d_text.need(b->text_len + 16);
    if (e != hipSuccess) return bfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "buffers", e);
    const int rc = tbk_bamdev_write_device(b, (const uint8_t *)b->d_records.p, (const uint64_t *)b->d_offsets.p, (uint8_t *)b->d_text.p);
    if (rc) return rc;
    e = hipMemcpyAsync(dst, b->d_text.p, b->text_len, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return bfail(TBK_ERR_HIP, "text home", e);
    return TBK_OK;
}

static int bam_refuse(const char *who, uint64_t bad) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: BAM record %llu: %s", who, (unsigned long long)(bad >> 8), tbk_bam_reason((uint32_t)(bad & 0xFFu)));
    tbk_set_error_(TBK_ERR_FORMAT, buf);
    return TBK_ERR_FORMAT;
}

// every offset must name a record that lies within `size` (what tbk_bam_index hands out): the kernels trust them
static int bam_check_offsets(const char *who, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t p = offsets[i];
        if (p > size || size - p < 36 || tbk_bam_u32(records + p) < 32 || (uint64_t)tbk_bam_u32(records + p) > size - p - 4) {
            char buf[160];
            snprintf(buf, sizeof buf, "%s: offsets[%llu] names no whole record of the window", who, (unsigned long long)i);
            tbk_set_error_(TBK_ERR_INVALID, buf);
            return TBK_ERR_INVALID;
        }
    }
    return TBK_OK;
}

extern "C" int tbk_bam_fastq_device(int device, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, uint8_t *dst,
                                    uint64_t cap, uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped) {
    if (!text_len || (n && (!records || !offsets))) { tbk_set_error_(TBK_ERR_INVALID, "tbk_bam_fastq_device: NULL argument"); return TBK_ERR_INVALID; }
    *text_len = 0;
    int rc = bam_check_offsets("tbk_bam_fastq_device", records, size, offsets, n);
    if (rc) return rc;
    tbk_bamdev *b = nullptr;
    if ((rc = tbk_bamdev_create(device, &b))) return rc;
    uint64_t written = 0, skipped = 0, bad = TBK_BAM_NO_BAD;
    rc = tbk_bamdev_measure(b, records, size, offsets, n, skip_flags, 0, text_len, &written, &skipped, &bad);
    if (!rc && bad != TBK_BAM_NO_BAD) { *text_len = 0; rc = bam_refuse("tbk_bam_fastq_device", bad); }
    if (!rc) {
        if (n_written) *n_written = written;
        if (n_skipped) *n_skipped = skipped;
        if (*text_len > cap || (!dst && *text_len)) { tbk_set_error_(TBK_ERR_NOMEM, "tbk_bam_fastq_device: dst too small"); rc = TBK_ERR_NOMEM; }
    }
    if (!rc) rc = tbk_bamdev_write(b, dst);
    tbk_bamdev_destroy(b);
    return rc;
}

// The same through the plain C++ transcoder of tbk_bam.h on the host's threads (tbk_host_threads): the second opinion on the
// kernels, and what the reader runs without a device.
extern "C" int tbk_bam_fastq(const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, uint8_t *dst, uint64_t cap,
                             uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped) {
    if (!text_len || (n && (!records || !offsets))) { tbk_set_error_(TBK_ERR_INVALID, "tbk_bam_fastq: NULL argument"); return TBK_ERR_INVALID; }
    *text_len = 0;
    const int rc = bam_check_offsets("tbk_bam_fastq", records, size, offsets, n);
    if (rc) return rc;
    TbkBamShares shares;
    uint64_t need = 0, written = 0, skipped = 0;
    const uint64_t bad = tbk_bam_fastq_shares(records, offsets, n, skip_flags, tbk_host_threads(), shares, nullptr, &need, &written, &skipped);
    if (bad != TBK_BAM_NO_BAD) return bam_refuse("tbk_bam_fastq", bad);
    *text_len = need;
    if (n_written) *n_written = written;
    if (n_skipped) *n_skipped = skipped;
    if (need > cap || (!dst && need)) { tbk_set_error_(TBK_ERR_NOMEM, "tbk_bam_fastq: dst too small"); return TBK_ERR_NOMEM; }
    if (need) (void)tbk_bam_fastq_shares(records, offsets, n, skip_flags, tbk_host_threads(), shares, dst, &need, &written, &skipped);
    return TBK_OK;
}

// The kernels timed by themselves (tools/measure_bam.py): the window is copied to the device once and stays there; after a
// warm-up, `reps` times: whole_s[i] = measure kernel, scan, the text's size brought home and the write kernel, wall clock
// around the calls with the stream idle before and after; write_s[i] = the write kernel alone between two HIP events.
extern "C" int tbk_bam_bench_device(int device, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, int reps,
                                    double *whole_s, double *write_s, uint64_t *text_len) {
    if (!records || !offsets || !n || reps < 1 || !whole_s || !write_s || !text_len) { tbk_set_error_(TBK_ERR_INVALID, "tbk_bam_bench_device: bad argument"); return TBK_ERR_INVALID; }
    int rc = bam_check_offsets("tbk_bam_bench_device", records, size, offsets, n);
    if (rc) return rc;
    tbk_bamdev *b = nullptr;
    if ((rc = tbk_bamdev_create(device, &b))) return rc;
    uint64_t written = 0, skipped = 0, bad = TBK_BAM_NO_BAD;
    rc = tbk_bamdev_measure(b, records, size, offsets, n, skip_flags, 0, text_len, &written, &skipped, &bad);
    if (!rc && bad != TBK_BAM_NO_BAD) rc = bam_refuse("tbk_bam_bench_device", bad);
    if (!rc && !*text_len) { tbk_set_error_(TBK_ERR_INVALID, "tbk_bam_bench_device: the window has no text"); rc = TBK_ERR_INVALID; }
    hipError_t e = hipSuccess;
    if (!rc) e = b->d_text.need(*text_len + 16);
    if (!rc && e != hipSuccess) rc = bfail(TBK_ERR_NOMEM, "buffers", e);
    for (int i = -1; i < reps && !rc; i++) {   // (-1: the warm-up)
        const auto t0 = std::chrono::steady_clock::now();
        rc = tbk_bamdev_measure_device(b, (const uint8_t *)b->d_records.p, (const uint64_t *)b->d_offsets.p, n, skip_flags, 0, text_len, &written, &skipped, &bad);
        if (!rc) rc = tbk_bamdev_write_device(b, (const uint8_t *)b->d_records.p, (const uint64_t *)b->d_offsets.p, (uint8_t *)b->d_text.p);
        if (!rc && (e = hipStreamSynchronize(b->stream)) != hipSuccess) rc = bfail(TBK_ERR_HIP, "bench", e);
        const double whole = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        double alone = 0;
        if (!rc) rc = tbk_bamdev_time_write(b, &alone);
        if (i >= 0) { whole_s[i] = whole; write_s[i] = alone; }
    }
    tbk_bamdev_destroy(b);
    return rc;
}
