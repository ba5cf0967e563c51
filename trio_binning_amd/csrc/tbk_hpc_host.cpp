// tbk_hpc_host.cpp — host side of homopolymer compression (kernels: tbk_hpc.hip; the contract: include/tbk.h).
// A session owns a stream and its device buffers, which grow to the largest batch seen; a batch is five launches
// queued back to back and one 16-byte copy home (the compressed total and the verdict on the offsets).  The keep bits
// and the tile offsets stay until the next compress call: lift and expand read the map backwards from them.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/tbk.h"
#include "tbk_common.h"

extern "C" void tbk_set_error_(int code, const char *msg);
extern "C" int tbk_check_offsets_(const uint64_t *offsets, uint64_t n_reads);
extern "C" uint32_t tbk_hpc_tile(void);
extern "C" uint64_t tbk_hpc_tiles(uint64_t total);
extern "C" hipError_t tbk_launch_hpc_mark(const uint8_t *, const uint64_t *, uint64_t, uint64_t, int, uint32_t *, uint64_t *, unsigned long long *,
                                          unsigned long long *, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_hpc_move(const uint8_t *, const uint64_t *, uint64_t, uint64_t, const uint64_t *, const unsigned long long *, uint8_t *,
                                          uint64_t, uint64_t *, hipStream_t);
extern "C" hipError_t tbk_launch_hpc_lift(const uint64_t *, uint64_t, const uint64_t *, const unsigned long long *, uint64_t, uint64_t *, hipStream_t);
extern "C" hipError_t tbk_launch_hpc_expand(const uint8_t *, uint64_t, const uint64_t *, const unsigned long long *, uint64_t, uint8_t *, hipStream_t);

static int hfail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    tbk_set_error_(code, buf);
    return code;
}
#define HHIP(expr)                                                                                                      \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) {                                                                                         \
            (void)hipGetLastError();                                                                                    \
            return hfail(e_ == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
        }                                                                                                               \
    } while (0)

// a device buffer that only ever grows
struct HpcBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct tbk_hpc {
    int device = 0;
    hipStream_t stream = nullptr;
    HpcBuf in_bases, in_offsets;        // a host batch on its way in
    HpcBuf out_bases, out_offsets;      // the result
    HpcBuf starts, keep, tiles;         // one bit per base each; tiles + 1 counts, tiles + 1 offsets, the verdict word
    HpcBuf back_in, back_out;           // a host array on its way through lift or expand
    bool valid = false;                 // a result is there to fetch
    uint64_t n_reads = 0, total = 0;    // of the result
    uint64_t in_total = 0;              // bases of the batch it was made of: what `keep` and the tile offsets describe
};

static int hpc_device(const tbk_hpc *h) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return hfail(TBK_ERR_NO_DEVICE, "no HIP device visible; libtbk_hip has no CPU fallback");
    HHIP(hipSetDevice(h->device));
    return TBK_OK;
}

// A buffer that fails to grow is left empty, never dangling: the session stays usable.
static int hpc_reserve(HpcBuf &b, size_t need) {
    need = (need + 255) & ~(size_t)255;
    if (need <= b.cap) return TBK_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const size_t want = need + need / 8;
    const hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();
        return hfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "homopolymer compression buffer (%zu bytes): %s", want, hipGetErrorString(e));
    }
    b.cap = want;
    return TBK_OK;
}

extern "C" int tbk_hpc_create(int device, tbk_hpc **out) {
    if (!out) return hfail(TBK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    tbk_hpc tmp;
    tmp.device = device;
    const int rc = hpc_device(&tmp);
    if (rc) return rc;
    hipStream_t stream = nullptr;
    HHIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    tbk_hpc *h = new tbk_hpc();
    h->device = device;
    h->stream = stream;
    *out = h;
    return TBK_OK;
}

extern "C" void tbk_hpc_destroy(tbk_hpc *h) {
    if (!h) return;
    if (hipSetDevice(h->device) == hipSuccess) {
        if (h->stream) {
            (void)hipStreamSynchronize(h->stream);
            (void)hipStreamDestroy(h->stream);
        }
        for (HpcBuf *b : {&h->in_bases, &h->in_offsets, &h->out_bases, &h->out_offsets, &h->starts, &h->keep, &h->tiles, &h->back_in, &h->back_out})
            if (b->p) (void)hipFree(b->p);
    }
    delete h;
}

// d_bases / d_offsets: the batch in HBM (d_bases 16-byte aligned).  Leaves the result in the session's buffers.
static int hpc_run(tbk_hpc *h, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t total, int fold_case) {
    h->valid = false;
    int rc;
    if ((rc = hpc_reserve(h->out_offsets, (size_t)(n_reads + 1) * 8)) || (rc = hpc_reserve(h->out_bases, (((size_t)total + 15) & ~(size_t)15) + 64))) return rc;
    if (!n_reads || !total) {
        // nothing to compress: every read, if there is one, is empty
        HHIP(hipMemsetAsync(h->out_offsets.p, 0, (size_t)(n_reads + 1) * 8, h->stream));
        HHIP(hipMemsetAsync(h->out_bases.p, 0, 64, h->stream));
        HHIP(hipStreamSynchronize(h->stream));
        h->valid = true; h->n_reads = n_reads; h->total = 0; h->in_total = 0;
        return TBK_OK;
    }
    if (((uintptr_t)d_bases & 15u) != 0) return hfail(TBK_ERR_INVALID, "the bases of a device batch must be 16-byte aligned");
    const uint64_t tiles = tbk_hpc_tiles(total);
    const size_t bitmap = (size_t)tiles * (tbk_hpc_tile() / 8);
    if ((rc = hpc_reserve(h->starts, bitmap)) || (rc = hpc_reserve(h->keep, bitmap)) || (rc = hpc_reserve(h->tiles, (size_t)(2 * (tiles + 1) + 1) * 8))) return rc;
    unsigned long long *d_counts = h->tiles.as<unsigned long long>(), *d_tile_offsets = d_counts + tiles + 1, *d_bad = d_tile_offsets + tiles + 1;
    HHIP(tbk_launch_hpc_mark(d_bases, d_offsets, n_reads, total, fold_case, h->starts.as<uint32_t>(), h->keep.as<uint64_t>(), d_counts, d_tile_offsets, d_bad,
                             h->stream));
    HHIP(tbk_launch_hpc_move(d_bases, d_offsets, n_reads, total, h->keep.as<uint64_t>(), d_tile_offsets, h->out_bases.as<uint8_t>(), total,
                             h->out_offsets.as<uint64_t>(), h->stream));
    unsigned long long home[2] = {0, 0};  // the last tile offset - the total - and the verdict behind it
    HHIP(hipMemcpyAsync(home, d_tile_offsets + tiles, sizeof home, hipMemcpyDeviceToHost, h->stream));
    HHIP(hipStreamSynchronize(h->stream));
    if (home[1]) return hfail(TBK_ERR_INVALID, "the offsets of the device batch do not ascend from 0 to total_bases");
    if (home[0] > total) return hfail(TBK_ERR_HIP, "homopolymer compression kept %llu of %llu bases", home[0], (unsigned long long)total);
    // what lies behind the result reads as not-ACGT, whatever a consumer's vector loads take with them
    HHIP(hipMemsetAsync(h->out_bases.as<uint8_t>() + home[0], 0, 64, h->stream));
    HHIP(hipStreamSynchronize(h->stream));
    h->valid = true; h->n_reads = n_reads; h->total = home[0]; h->in_total = total;
    return TBK_OK;
}

static void hpc_result(const tbk_hpc *h, int rc, void **d_bases, void **d_offsets, uint64_t *total_out) {
    if (d_bases) *d_bases = rc ? nullptr : h->out_bases.p;
    if (d_offsets) *d_offsets = rc ? nullptr : h->out_offsets.p;
    if (total_out) *total_out = rc ? 0 : h->total;
}

extern "C" int tbk_hpc_compress_device(tbk_hpc *h, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t total_bases, int fold_case,
                                       void **d_bases_out, void **d_offsets_out, uint64_t *total_out) {
    if (h) hpc_result(h, TBK_ERR_INVALID, d_bases_out, d_offsets_out, total_out);
    if (h) h->valid = false;
    if (!h || (n_reads && !d_offsets) || (total_bases && !d_bases)) return hfail(TBK_ERR_INVALID, "NULL argument");
    if (!n_reads && total_bases) return hfail(TBK_ERR_INVALID, "no reads, yet %llu bases", (unsigned long long)total_bases);
    int rc = hpc_device(h);
    if (!rc) rc = hpc_run(h, (const uint8_t *)d_bases, (const uint64_t *)d_offsets, n_reads, total_bases, fold_case);
    hpc_result(h, rc, d_bases_out, d_offsets_out, total_out);
    return rc;
}

extern "C" int tbk_hpc_compress(tbk_hpc *h, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int fold_case, void **d_bases_out,
                                void **d_offsets_out, uint64_t *total_out) {
    if (h) hpc_result(h, TBK_ERR_INVALID, d_bases_out, d_offsets_out, total_out);
    if (h) h->valid = false;
    if (!h || (n_reads && !offsets)) return hfail(TBK_ERR_INVALID, "NULL argument");
    int rc = n_reads ? tbk_check_offsets_(offsets, n_reads) : TBK_OK;
    if (rc) return rc;
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    if (total && !bases) return hfail(TBK_ERR_INVALID, "bases is NULL");
    if ((rc = hpc_device(h))) return rc;
    if (n_reads && total) {
        if ((rc = hpc_reserve(h->in_bases, (size_t)total + 16)) || (rc = hpc_reserve(h->in_offsets, (size_t)(n_reads + 1) * 8))) return rc;
        HHIP(hipMemcpyAsync(h->in_bases.p, bases, total, hipMemcpyHostToDevice, h->stream));
        HHIP(hipMemcpyAsync(h->in_offsets.p, offsets, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, h->stream));
    }
    rc = hpc_run(h, h->in_bases.as<uint8_t>(), h->in_offsets.as<uint64_t>(), n_reads, total, fold_case);
    if (rc) (void)hipStreamSynchronize(h->stream);  // (the caller's arrays are free to go whatever happened)
    hpc_result(h, rc, d_bases_out, d_offsets_out, total_out);
    return rc;
}

extern "C" int tbk_hpc_fetch(tbk_hpc *h, uint8_t *bases, uint64_t cap, uint64_t *offsets) {
    if (!h) return hfail(TBK_ERR_INVALID, "session is NULL");
    if (!h->valid) return hfail(TBK_ERR_INVALID, "the session holds no result");
    if (h->total > cap) return hfail(TBK_ERR_INVALID, "the result has %llu bases, the buffer room for %llu", (unsigned long long)h->total, (unsigned long long)cap);
    if (h->total && !bases) return hfail(TBK_ERR_INVALID, "bases is NULL");
    const int rc = hpc_device(h);
    if (rc) return rc;
    if (h->total) HHIP(hipMemcpyAsync(bases, h->out_bases.p, h->total, hipMemcpyDeviceToHost, h->stream));
    if (offsets) HHIP(hipMemcpyAsync(offsets, h->out_offsets.p, (size_t)(h->n_reads + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HHIP(hipStreamSynchronize(h->stream));
    return TBK_OK;
}

// ---- the map read backwards ----------------------------------------------------------------------------------------
static unsigned long long *hpc_tile_offsets(const tbk_hpc *h) { return h->tiles.as<unsigned long long>() + tbk_hpc_tiles(h->in_total) + 1; }

// For the hit tracker: n positions of the last result's compressed stream, in HBM, to positions of the batch it was made
// of.  Queued on `stream`, which must be ordered behind the compress call's return; nothing is waited for.
extern "C" int tbk_hpc_lift_device_(tbk_hpc *h, const uint64_t *d_positions, uint64_t n, uint64_t *d_out, hipStream_t stream) {
    if (!h || !h->valid) return hfail(TBK_ERR_INVALID, "the session holds no result");
    if (!n) return TBK_OK;
    if (!h->in_total) {  // an empty batch: the one position there is, 0, is its end
        HHIP(hipMemsetAsync(d_out, 0, (size_t)n * 8, stream));
        return TBK_OK;
    }
    HHIP(tbk_launch_hpc_lift(d_positions, n, h->keep.as<uint64_t>(), hpc_tile_offsets(h), h->in_total, d_out, stream));
    return TBK_OK;
}

// One byte per kept byte in, one byte per base of the batch out (d_out 16-byte aligned, room rounded up to 16).
extern "C" int tbk_hpc_expand_device_(tbk_hpc *h, const uint8_t *d_values, uint8_t *d_out, hipStream_t stream) {
    if (!h || !h->valid) return hfail(TBK_ERR_INVALID, "the session holds no result");
    if (!h->in_total) return TBK_OK;
    HHIP(tbk_launch_hpc_expand(d_values, h->total, h->keep.as<uint64_t>(), hpc_tile_offsets(h), h->in_total, d_out, stream));
    return TBK_OK;
}

extern "C" int tbk_hpc_lift(tbk_hpc *h, const uint64_t *positions, uint64_t n, uint64_t *out) {
    if (!h) return hfail(TBK_ERR_INVALID, "session is NULL");
    if (!h->valid) return hfail(TBK_ERR_INVALID, "the session holds no result");
    if (!n) return TBK_OK;
    if (!positions || !out) return hfail(TBK_ERR_INVALID, "NULL argument");
    for (uint64_t i = 0; i < n; i++)
        if (positions[i] > h->total)
            return hfail(TBK_ERR_INVALID, "position %llu (number %llu) lies behind the %llu compressed bases", (unsigned long long)positions[i],
                         (unsigned long long)i, (unsigned long long)h->total);
    int rc = hpc_device(h);
    if (rc || (rc = hpc_reserve(h->back_in, (size_t)n * 8)) || (rc = hpc_reserve(h->back_out, (size_t)n * 8))) return rc;
    HHIP(hipMemcpyAsync(h->back_in.p, positions, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    rc = tbk_hpc_lift_device_(h, h->back_in.as<uint64_t>(), n, h->back_out.as<uint64_t>(), h->stream);
    if (!rc) HHIP(hipMemcpyAsync(out, h->back_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HHIP(hipStreamSynchronize(h->stream));
    return rc;
}

extern "C" int tbk_hpc_expand(tbk_hpc *h, const uint8_t *values, uint8_t *out) {
    if (!h) return hfail(TBK_ERR_INVALID, "session is NULL");
    if (!h->valid) return hfail(TBK_ERR_INVALID, "the session holds no result");
    if (!h->in_total) return TBK_OK;
    if (!values || !out) return hfail(TBK_ERR_INVALID, "NULL argument");
    int rc = hpc_device(h);
    if (rc || (rc = hpc_reserve(h->back_in, (size_t)h->total)) || (rc = hpc_reserve(h->back_out, (((size_t)h->in_total + 15) & ~(size_t)15)))) return rc;
    HHIP(hipMemcpyAsync(h->back_in.p, values, (size_t)h->total, hipMemcpyHostToDevice, h->stream));
    rc = tbk_hpc_expand_device_(h, h->back_in.as<uint8_t>(), h->back_out.as<uint8_t>(), h->stream);
    if (!rc) HHIP(hipMemcpyAsync(out, h->back_out.p, (size_t)h->in_total, hipMemcpyDeviceToHost, h->stream));
    HHIP(hipStreamSynchronize(h->stream));
    return rc;
}
