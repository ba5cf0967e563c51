// tbk_gzplan.cpp — see tbk_gzplan.h.  Host only: the sanitizer build covers it.
#include "tbk_gzplan.h"

#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

#include "../../include/tbk.h"
#include "tbk_inflate.h"

extern "C" void tbk_set_error_(int, const char *msg);
uint32_t tbk_crc32(uint32_t crc, const uint8_t *p, size_t n);  // tbk_crc.cpp

namespace {
constexpr size_t GZ_MAX_RATIO = 1040;   // DEFLATE makes at most 258 bytes from two bits: 1032 to one, and a little
thread_local TbkGzStats last_stats = {0, 0, 0, 0, 0, 0.0, 0};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class F> void run_threads(int n, size_t items, F &&fn) {
    std::atomic<size_t> next{0};
    auto work = [&] { for (size_t i; (i = next.fetch_add(1)) < items;) fn(i); };
    std::vector<std::thread> pool;
    const int nt = (int)std::min<size_t>((size_t)std::max(1, n), items);
    for (int t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (std::thread &th : pool) th.join();
}
}  // namespace

TbkGzOptions tbk_gz_options_from_env(int threads) {
    TbkGzOptions o;
    o.threads = std::max(1, std::min(threads, 64));
    if (const char *e = getenv("TBK_GZIP_CHUNK")) if (*e) o.chunk = (size_t)strtoull(e, nullptr, 10);
    if (const char *e = getenv("TBK_GZIP_WINDOW")) if (*e) o.window = (size_t)strtoull(e, nullptr, 10);
    if (const char *e = getenv("TBK_GZIP_RATIO")) if (*e) o.ratio = (size_t)strtoull(e, nullptr, 10);
    o.chunk = std::max<size_t>(o.chunk, 1024);
    o.window = std::max<size_t>(o.window, o.chunk);
    o.ratio = std::min(std::max<size_t>(o.ratio, 1), GZ_MAX_RATIO);
    return o;
}

void tbk_gz_plan_window(const uint8_t *data, size_t size, uint64_t start_bit, const TbkGzOptions &opt, size_t window_bytes, size_t ratio,
                        std::vector<TbkGzChunk> &chunks, size_t *in_lo, size_t *in_bytes) {
    const size_t lo = (size_t)(start_bit >> 3), hi = std::min(size, lo + std::max<size_t>(window_bytes, 1));
    const size_t n_spans = (hi - lo + opt.chunk - 1) / opt.chunk;
    std::vector<uint64_t> found(n_spans, ~0ull);
    if (n_spans > 1) {
        run_threads(opt.threads, n_spans - 1, [&](size_t k) {
            const size_t s_lo = lo + (k + 1) * opt.chunk, s_hi = std::min(hi, s_lo + opt.chunk);
            if (s_lo + 64 >= size) return;
            static thread_local std::unique_ptr<TbkInflate> d;
            if (!d) d.reset(new TbkInflate());
            for (uint64_t bit = (uint64_t)s_lo * 8; bit < (uint64_t)s_hi * 8; bit++)
                if (d->open_dynamic_block_at(data, size, bit)) { found[k + 1] = bit; return; }
        });
    }
    chunks.clear();
    const uint64_t base = (uint64_t)lo * 8;
    chunks.push_back(TbkGzChunk{start_bit - base, 0, 0, 0, 1});
    for (size_t k = 1; k < n_spans; k++)
        if (found[k] != ~0ull) chunks.push_back(TbkGzChunk{found[k] - base, 0, 0, 0, 0});
    uint64_t at = 0;
    size_t keep = 0;
    for (size_t i = 0; i < chunks.size(); i++, keep++) {
        TbkGzChunk &c = chunks[i];
        c.stop_bit = i + 1 < chunks.size() ? chunks[i + 1].start_bit : std::max<uint64_t>((uint64_t)(hi - lo) * 8, c.start_bit + 1);
        const uint64_t bytes = (c.stop_bit - c.start_bit + 7) / 8;
        uint64_t cap = std::min<uint64_t>(bytes * ratio + 4096, 0x7FFF0000ull);
        if (i == 0) cap = std::min<uint64_t>(cap, opt.max_symbols);
        else if (at + TBK_GZ_HIST + cap + 16 > opt.max_symbols) break;   // the window is as long as its symbols have room
        c.out_cap = (uint32_t)cap;
        c.sym_off = at;
        at += (TBK_GZ_HIST + cap + 8 + 7) & ~(uint64_t)7;
    }
    chunks.resize(keep);   // (the last chunk kept still stops at the first one dropped)
    const size_t slack = std::max<size_t>(opt.chunk, (size_t)1 << 20);
    *in_lo = lo;
    *in_bytes = std::min(size - lo, (size_t)((chunks.back().stop_bit + 7) / 8) + slack);
}

size_t tbk_gz_chain_accept(const TbkGzChunk *chunks, const TbkGzResult *res, size_t n) {
    auto decoded = [&](size_t i) { return res[i].status == TBK_GZ_BOUNDARY || res[i].status == TBK_GZ_MEMBER_DONE; };
    if (!n || !decoded(0)) return 0;
    size_t good = 1;
    while (good < n && res[good - 1].status == TBK_GZ_BOUNDARY && res[good - 1].end_bit == chunks[good].start_bit && decoded(good)) good++;
    return good;
}

// what the host's decoder says about the stream from `bit` on (chunk 0 of a window did not decode on the device)
static std::string host_verdict(const uint8_t *data, size_t size, uint64_t bit, const std::vector<uint16_t> &tail) {
    std::unique_ptr<TbkInflate> d(new TbkInflate());
    d->position_at_bit(data, size, bit);
    const size_t room = (size_t)1 << 20;
    std::vector<uint16_t> sym(TBK_GZ_HIST + room);
    memcpy(sym.data(), tail.data(), TBK_GZ_HIST * 2);
    for (;;) {
        size_t pos = TBK_GZ_HIST;
        const TbkInflate::Status st = d->run16(sym.data(), &pos, sym.size(), ~0ull);
        if (st == TbkInflate::ERROR) return std::string("inflate: ") + d->error();
        if (st != TbkInflate::NEED_OUTPUT || pos < 2 * (size_t)TBK_GZ_HIST) break;
        memmove(sym.data(), sym.data() + pos - TBK_GZ_HIST, TBK_GZ_HIST * 2);
    }
    return "inflate: the device's decoder refused a stream the host's takes";
}

int tbk_gz_run(TbkGzBackend &be, const uint8_t *data, size_t size, const TbkGzOptions &opt, const std::function<bool(const uint8_t *, size_t, bool)> &sink,
               TbkGzStats *stats, std::string *err) {
    TbkGzStats st = {0, 0, 0, 0, 0, 0.0, 0};
    auto done = [&](int code, const std::string &msg) {
        if (stats) *stats = st;
        last_stats = st;
        if (code != TBK_OK) { if (err) *err = msg; tbk_set_error_(code, msg.c_str()); }
        return code;
    };
    std::unique_ptr<TbkInflate> hdr(new TbkInflate());
    std::vector<TbkGzChunk> chunks;
    std::vector<TbkGzResult> res;
    std::vector<uint64_t> text_off;
    std::vector<uint32_t> crcs;
    std::vector<uint8_t> bad;
    std::vector<uint16_t> tail(TBK_GZ_HIST);
    size_t ratio = opt.ratio, off = 0;   // (1 .. GZ_MAX_RATIO: tbk_gz_options_from_env)
    for (;;) {   // members
        bool at_end = false;
        if (!hdr->open_member_at(data, size, off, &at_end)) return done(TBK_ERR_FORMAT, std::string("inflate: ") + hdr->error());
        if (at_end) break;
        uint64_t bit = hdr->bit_position();
        std::fill(tail.begin(), tail.end(), TBK_GZ_NOTHING);
        uint32_t member_crc = (uint32_t)crc32(0L, Z_NULL, 0);
        uint64_t member_size = 0;
        size_t window_bytes = opt.window;
        for (bool member_done = false; !member_done;) {   // windows
            size_t in_lo = 0, in_bytes = 0;
            const double t0 = now_s();
            tbk_gz_plan_window(data, size, bit, opt, window_bytes, ratio, chunks, &in_lo, &in_bytes);
            st.guess_s += now_s() - t0;
            const size_t n = chunks.size();
            res.assign(n, TbkGzResult{TBK_GZ_SKIPPED, 0, 0});
            const int rc = be.decode(data + in_lo, in_bytes, chunks.data(), n, tail.data(), res.data());
            if (rc != TBK_OK) return done(rc, std::string("inflate: ") + tbk_last_error());
            st.windows++; st.guessed += n - 1;
            const size_t n_acc = tbk_gz_chain_accept(chunks.data(), res.data(), n);
            st.accepted += n_acc; st.redecoded += n - n_acc;
            st.most_accepted = std::max<uint32_t>(st.most_accepted, (uint32_t)n_acc);
            if (n_acc < n && res[n_acc].status == TBK_GZ_NO_ROOM) {
                const bool clamped = n_acc == 0 && (uint64_t)chunks[0].out_cap >= opt.max_symbols;
                if (clamped || ratio >= GZ_MAX_RATIO) {
                    if (n_acc == 0) {
                        if (window_bytes < 2048) return done(TBK_ERR_NOMEM, "inflate: a DEFLATE block too long for the device's symbol buffer");
                        window_bytes /= 2;   // (chunk 0 stops at the first block header past the window: a shorter one, sooner)
                    }
                } else {
                    ratio = std::min(ratio * (n_acc == 0 ? 8 : 2), GZ_MAX_RATIO);
                }
            }
            if (n_acc == 0) {
                if (res[0].status == TBK_GZ_NO_ROOM) continue;
                if (res[0].status == TBK_GZ_NO_INPUT) {
                    if (in_lo + in_bytes >= size) return done(TBK_ERR_FORMAT, "inflate: truncated gzip file");
                    window_bytes = window_bytes * 2 + ((size_t)1 << 20);   // a block longer than the slack behind the window
                    continue;
                }
                return done(TBK_ERR_FORMAT, host_verdict(data, size, bit, tail));
            }
            text_off.resize(n_acc + 1);
            uint64_t total = 0;
            for (size_t i = 0; i < n_acc; i++) { text_off[i] = total; total += res[i].n_sym; }
            text_off[n_acc] = total;
            crcs.assign(n_acc, 0); bad.assign(n_acc, 0);
            uint8_t *text = nullptr;
            const int rc2 = be.resolve(n_acc, res.data(), text_off.data(), total, &text, crcs.data(), bad.data());
            if (rc2 != TBK_OK) return done(rc2, std::string("inflate: ") + tbk_last_error());
            for (size_t i = 0; i < n_acc; i++) {
                if (bad[i]) return done(TBK_ERR_FORMAT, "inflate: distance too far back");
                member_crc = (uint32_t)crc32_combine(member_crc, crcs[i], (z_off_t)res[i].n_sym);
                member_size += res[i].n_sym;
            }
            const TbkGzResult &last = res[n_acc - 1];
            if (last.status == TBK_GZ_MEMBER_DONE) {
                const size_t byte = in_lo + (size_t)((last.end_bit + 7) >> 3);
                if (byte + 8 > size) return done(TBK_ERR_FORMAT, "inflate: truncated gzip file");
                const uint8_t *t = data + byte;
                const uint32_t t_crc = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
                const uint32_t t_isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
                if (member_crc != t_crc || (uint32_t)member_size != t_isize) return done(TBK_ERR_FORMAT, "inflate: gzip CRC or size mismatch");
                off = byte + 8;
                member_done = true;
            } else {
                bit = (uint64_t)in_lo * 8 + last.end_bit;
                // the window in front of the next chunk 0: the last 32 Ki of (the window so far, this window's text)
                const size_t take = (size_t)std::min<uint64_t>(TBK_GZ_HIST, total), keep = TBK_GZ_HIST - take;
                if (keep) memmove(tail.data(), tail.data() + take, keep * 2);
                for (size_t k = 0; k < take; k++) tail[keep + k] = text[total - take + k];
                window_bytes = opt.window;
            }
            if (total && !sink(text, (size_t)total, false)) return done(TBK_ERR_STATE, "inflate: stopped");
        }
    }
    if (!sink(nullptr, 0, true)) return done(TBK_ERR_STATE, "inflate: stopped");
    return done(TBK_OK, "");
}

// ---- TbkInflate::run16 standing in for the device -------------------------------------------------------------------------------------
namespace {
struct HostBackend : TbkGzBackend {
    int threads;
    std::vector<std::vector<uint16_t>> sym;
    std::vector<uint8_t> text;
    explicit HostBackend(int t) : threads(t) {}
    int decode(const uint8_t *in, size_t in_bytes, const TbkGzChunk *chunks, size_t n, const uint16_t *window0, TbkGzResult *res) override {
        sym.resize(n);
        run_threads(threads, n, [&](size_t i) {
            const TbkGzChunk &c = chunks[i];
            std::vector<uint16_t> &s = sym[i];
            s.resize((size_t)TBK_GZ_HIST + c.out_cap + 512);
            if (c.window_known) memcpy(s.data(), window0, TBK_GZ_HIST * 2);
            else for (size_t w = 0; w < TBK_GZ_HIST; w++) s[w] = (uint16_t)(0x8000u + w);
            std::unique_ptr<TbkInflate> d(new TbkInflate());
            d->position_at_bit(in, in_bytes, c.start_bit);
            size_t pos = TBK_GZ_HIST;
            const TbkInflate::Status st = d->run16(s.data(), &pos, (size_t)TBK_GZ_HIST + c.out_cap, c.stop_bit);
            TbkGzResult r = {TBK_GZ_FAILED, (uint32_t)(pos - TBK_GZ_HIST), d->bit_position()};
            if (st == TbkInflate::BOUNDARY) r.status = TBK_GZ_BOUNDARY;
            else if (st == TbkInflate::MEMBER_DONE) { r.status = TBK_GZ_MEMBER_DONE; r.end_bit -= 64; }   // (run16 has read the trailer)
            else if (st == TbkInflate::ERROR && d->cut_in_trailer()) r.status = TBK_GZ_MEMBER_DONE;   // (as the device, which never reads a trailer: the loop finds it cut)
            else if (st == TbkInflate::NEED_OUTPUT) r.status = TBK_GZ_NO_ROOM;
            else if (st == TbkInflate::ERROR && strcmp(d->error(), "truncated gzip file") == 0) r.status = TBK_GZ_NO_INPUT;
            res[i] = r;
        });
        return TBK_OK;
    }
    int resolve(size_t n_acc, const TbkGzResult *res, const uint64_t *text_off, uint64_t text_total, uint8_t **out, uint32_t *crc, uint8_t *bad) override {
        // the windows, front to back: chunk i's from chunk i-1's window and the last 32 Ki of its symbols
        for (size_t i = 1; i < n_acc; i++) {
            const uint16_t *before = sym[i - 1].data(), *src = before + TBK_GZ_HIST;
            uint16_t *w = sym[i].data();
            const size_t n = res[i - 1].n_sym, take = std::min<size_t>(TBK_GZ_HIST, n), keep = TBK_GZ_HIST - take;
            for (size_t k = 0; k < keep; k++) w[k] = before[take + k];
            for (size_t k = 0; k < take; k++) { const uint16_t v = src[n - take + k]; w[keep + k] = v >= 0x8000u ? before[v - 0x8000u] : v; }
        }
        text.resize((size_t)text_total + 8);
        run_threads(threads, n_acc, [&](size_t i) {
            const uint16_t *w = sym[i].data(), *s = w + TBK_GZ_HIST;
            uint8_t *o = text.data() + text_off[i];
            uint32_t seen = 0;
            for (size_t k = 0; k < res[i].n_sym; k++) { const uint16_t v = s[k] >= 0x8000u ? w[s[k] - 0x8000u] : s[k]; seen |= v; o[k] = (uint8_t)v; }
            bad[i] = seen > 0xFFu;
            crc[i] = tbk_crc32(0, o, res[i].n_sym);
        });
        *out = text.data();
        return TBK_OK;
    }
};
}  // namespace

TbkGzBackend *tbk_gz_host_backend(int threads) { return new HostBackend(threads); }

static int run_to_buffer(TbkGzBackend &be, const uint8_t *data, uint64_t size, uint8_t *dst, uint64_t cap, uint64_t *text_len, const TbkGzOptions &opt) {
    uint64_t n = 0;
    const int rc = tbk_gz_run(be, data, (size_t)size, opt, [&](const uint8_t *p, size_t len, bool) {
        if (len && dst && n + len <= cap) memcpy(dst + n, p, len);
        n += len;
        return true;
    }, nullptr, nullptr);
    if (rc == TBK_OK || n) *text_len = n;
    if (rc != TBK_OK) return rc;
    if (n && (!dst || n > cap)) { tbk_set_error_(TBK_ERR_NOMEM, "gzip inflate: dst too small"); return TBK_ERR_NOMEM; }
    return TBK_OK;
}
int tbk_gz_run_to_buffer(TbkGzBackend &be, const uint8_t *data, uint64_t size, uint8_t *dst, uint64_t cap, uint64_t *text_len, const TbkGzOptions &opt) {
    return run_to_buffer(be, data, size, dst, cap, text_len, opt);
}

// C-ABI (include/tbk.h)
extern "C" int tbk_gzip_inflate_host(const uint8_t *data, uint64_t size, uint8_t *dst, uint64_t cap, uint64_t *text_len, uint64_t chunk, uint64_t window) {
    if ((!data && size) || !text_len) { tbk_set_error_(TBK_ERR_INVALID, "tbk_gzip_inflate_host: NULL argument"); return TBK_ERR_INVALID; }
    *text_len = 0;
    TbkGzOptions opt = tbk_gz_options_from_env(4);
    if (chunk) opt.chunk = std::max<size_t>((size_t)chunk, 1024);
    if (window) opt.window = (size_t)window;
    opt.window = std::max(opt.window, opt.chunk);
    std::unique_ptr<TbkGzBackend> be(tbk_gz_host_backend(opt.threads));
    return run_to_buffer(*be, data, size, dst, cap, text_len, opt);
}

extern "C" void tbk_gzip_inflate_stats(uint64_t out[6]) {
    out[0] = last_stats.windows; out[1] = last_stats.guessed; out[2] = last_stats.accepted; out[3] = last_stats.redecoded;
    out[4] = last_stats.handed_back; out[5] = last_stats.most_accepted;
}

// C-ABI (include/tbk.h; tests): the first member decoded by one decoder up to the first block header at or past stop_bit, and from
// that bit on by a second one that knows nothing but the bit (TbkInflate::position_at_bit) and the text so far.
extern "C" int tbk_inflate_resume_at_bit(const uint8_t *data, uint64_t size, uint64_t stop_bit, uint8_t *dst, uint64_t cap, uint64_t *text_len, uint64_t *boundary_bit) {
    if (!data || !dst || !text_len || !boundary_bit) { tbk_set_error_(TBK_ERR_INVALID, "tbk_inflate_resume_at_bit: NULL argument"); return TBK_ERR_INVALID; }
    *text_len = 0; *boundary_bit = 0;
    std::unique_ptr<TbkInflate> a(new TbkInflate()), b(new TbkInflate());
    bool at_end = false;
    if (!a->open_member_at(data, (size_t)size, 0, &at_end) || at_end) { tbk_set_error_(TBK_ERR_FORMAT, at_end ? "no gzip member" : a->error()); return TBK_ERR_FORMAT; }
    std::vector<uint16_t> sym((size_t)TBK_GZ_HIST + cap + 512);
    std::fill(sym.begin(), sym.begin() + TBK_GZ_HIST, TBK_GZ_NOTHING);
    size_t pos = TBK_GZ_HIST;
    const size_t room = sym.size();   // (the decoder wants 320 elements of slack behind the text)
    TbkInflate::Status st = a->run16(sym.data(), &pos, room, stop_bit);
    if (st == TbkInflate::BOUNDARY) {
        *boundary_bit = a->bit_position();
        b->position_at_bit(data, (size_t)size, *boundary_bit);
        st = b->run16(sym.data(), &pos, room, ~0ull);
    }
    if (st != TbkInflate::MEMBER_DONE) {
        tbk_set_error_(st == TbkInflate::NEED_OUTPUT ? TBK_ERR_NOMEM : TBK_ERR_FORMAT, st == TbkInflate::ERROR ? (*boundary_bit ? b->error() : a->error()) : "tbk_inflate_resume_at_bit: dst too small");
        return st == TbkInflate::NEED_OUTPUT ? TBK_ERR_NOMEM : TBK_ERR_FORMAT;
    }
    const size_t n = pos - TBK_GZ_HIST;
    if (n > cap) { tbk_set_error_(TBK_ERR_NOMEM, "tbk_inflate_resume_at_bit: dst too small"); return TBK_ERR_NOMEM; }
    for (size_t k = 0; k < n; k++) {
        if (sym[TBK_GZ_HIST + k] > 0xFFu) { tbk_set_error_(TBK_ERR_FORMAT, "inflate: distance too far back"); return TBK_ERR_FORMAT; }
        dst[k] = (uint8_t)sym[TBK_GZ_HIST + k];
    }
    *text_len = n;
    return TBK_OK;
}
