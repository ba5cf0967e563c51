// tbk_dump_host.cpp — host side of the counted-dump importer and exporter (kernels: tbk_dump.hip; the contract: include/tbk.h;
// the pieces that need no device: tbk_dump_text.h).
// Import: the files are mapped, cut into windows that end behind a newline, and staged through two pinned buffers - the host
// copies window i + 1 while the device works on window i - on a stream the call owns.  Every window is three launches (newline
// bits, the scan of the tile counts, the parse); after the last one the pairs are checked, sorted and folded only when they
// do not ascend strictly, brought to the floor asked for and tallied.  Export: selection on the device, the entries home in
// pieces, the text formatted by the host's threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <ctime>
#include <fcntl.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_compact_host.h"
#include "tbk_dump_text.h"

extern "C" void tbk_set_error_(int code, const char *msg);
extern "C" void *tbk_pin_alloc_(size_t bytes);
extern "C" void tbk_pin_free_(void *p);
extern "C" uint32_t tbk_dump_tile(void);
extern "C" hipError_t tbk_launch_dump_lines(const uint8_t *, uint64_t, uint64_t *, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_dump_parse(const uint8_t *, uint64_t, const uint64_t *, const unsigned long long *, int, int, uint64_t, uint64_t, uint64_t *,
                                            uint8_t *, unsigned long long *, hipStream_t);
extern "C" hipError_t tbk_launch_sort_u64_u8(const uint64_t *, uint64_t *, const uint8_t *, uint8_t *, uint64_t, int, hipStream_t);
extern "C" int tbk_kmerdb_make_(uint64_t *, uint8_t *, uint64_t, int, int, int, int, const uint64_t *, uint64_t, uint64_t, tbk_kmerdb **);
extern "C" int tbk_kmerdb_arrays_(const tbk_kmerdb *, const uint64_t **, const uint8_t **);

static int dfail(int code, const char *fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    tbk_set_error_(code, buf);
    return code;
}

constexpr uint64_t TBK_DUMP_WINDOW = (uint64_t)64 << 20;  // text per device window when the caller names none
constexpr uint64_t TBK_DUMP_MIN_WINDOW = 4096;            // a window always holds a whole line (k + 36 bytes at most)
constexpr unsigned long long TBK_DUMP_NO_BAD = ~0ull;

// the words for tbk_dump.hip's reasons, by their numbers
static const char *const TBK_DUMP_REASONS[] = {
    "",
    "line too long",
    "empty line",
    "the k-mer is shorter than k",
    "a byte of the k-mer is not one of ACGT (upper case)",
    "no separator and no counter behind the k-mer",
    "the k-mer is longer than k",
    "no tab or space behind the k-mer",
    "the counter is empty",
    "the counter is not a decimal number (digits only: no sign, no second separator, no carriage return)",
    "the counter has more than 32 digits",
    "the counter is 0",
    "the k-mer holds two equal adjacent bases: it is not homopolymer-compressed",
};

// ---- what the importer has done so far, for tools/measure_dump.py and the tests (tbk_dump_import_stats) ------------------
static std::atomic<uint64_t> g_imports{0}, g_sorts{0}, g_windows{0}, g_lines{0}, g_parse_us{0};
static std::atomic<uint64_t> g_alloc_limit{0};  // (test hook: device bytes one import may take; 0 = what HBM gives)

extern "C" int tbk_dump_import_stats(uint64_t *imports, uint64_t *sorts, uint64_t *windows, uint64_t *lines, double *parse_ms) {
    if (imports) *imports = g_imports.load();
    if (sorts) *sorts = g_sorts.load();
    if (windows) *windows = g_windows.load();
    if (lines) *lines = g_lines.load();
    if (parse_ms) *parse_ms = (double)g_parse_us.load() / 1000.0;
    return TBK_OK;
}

// (test hook, not in tbk.h: an import that would take more device memory than this fails as if HBM were full)
extern "C" void tbk_dump_set_alloc_limit_(uint64_t bytes) { g_alloc_limit.store(bytes); }

extern "C" void tbk_dump_options_init(tbk_dump_options *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->size = sizeof *o;
}

namespace {
struct MappedFile {
    std::string path;
    const uint8_t *text = nullptr;
    uint64_t size = 0;
    uint64_t lines = 0;  // lines of this file in the windows launched so far
};

struct Window {
    uint32_t file;
    uint64_t begin, end;  // end == begin: no newline within a window's bytes - a line too long
};

// Everything one import holds; freed in one place whatever way the call ends.
struct Import {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<MappedFile> files;
    uint8_t *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
    std::vector<void *> dev;  // device allocations still owned
    uint64_t dev_bytes = 0;

    hipError_t alloc(void **p, size_t bytes) {
        *p = nullptr;
        const uint64_t limit = g_alloc_limit.load();
        if (limit && dev_bytes + bytes > limit) return hipErrorOutOfMemory;
        const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e != hipSuccess) { *p = nullptr; return e; }
        dev.push_back(*p);
        dev_bytes += bytes;
        return hipSuccess;
    }
    hipError_t reserve(Compaction &c, uint64_t n) {  // (c frees its own two buffers; their bytes count all the same)
        const uint64_t limit = g_alloc_limit.load();
        if (limit && dev_bytes + Compaction::bytes(n) > limit) return hipErrorOutOfMemory;
        const hipError_t e = c.reserve(n, stream);
        if (e == hipSuccess) dev_bytes += Compaction::bytes(n);
        return e;
    }
    void release(void *p) {  // free now
        if (!p) return;
        disown(p);
        (void)hipFree(p);
    }
    void disown(void *p) {  // the database takes it over
        dev.erase(std::remove(dev.begin(), dev.end(), p), dev.end());
    }
    ~Import() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void *p : dev) (void)hipFree(p);
        for (uint8_t *p : pin)
            if (p) tbk_pin_free_(p);
        for (auto &set : ev)
            for (hipEvent_t e : set)
                if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        for (MappedFile &f : files)
            if (f.text) munmap((void *)f.text, (size_t)f.size);
    }
};

int hip_fail(const char *what, hipError_t e) {
    (void)hipGetLastError();
    return dfail(e == hipErrorOutOfMemory ? TBK_ERR_NOMEM : TBK_ERR_HIP, "k-mer dump: %s: %s", what, hipGetErrorString(e));
}
}  // namespace

#define DHIP(expr)                                 \
    do {                                           \
        const hipError_t e_ = (expr);              \
        if (e_ != hipSuccess) return hip_fail(#expr, e_); \
    } while (0)

static int map_file(const char *path, MappedFile *f) {
    f->path = path;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return dfail(TBK_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) {
        const int err = errno;
        ::close(fd);
        return dfail(TBK_ERR_IO, "%s: %s", path, strerror(err));
    }
    if (!S_ISREG(st.st_mode)) {
        ::close(fd);
        return dfail(TBK_ERR_IO, "%s: not a regular file", path);
    }
    f->size = (uint64_t)st.st_size;
    if (f->size) {
        void *m = mmap(nullptr, (size_t)f->size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) {
            const int err = errno;
            ::close(fd);
            return dfail(TBK_ERR_IO, "cannot map %s: %s", path, strerror(err));
        }
        (void)madvise(m, (size_t)f->size, MADV_SEQUENTIAL);
        f->text = (const uint8_t *)m;
    }
    ::close(fd);
    return TBK_OK;
}

extern "C" int tbk_dump_file_k(const char *path, int *k) {
    if (!path || !k) return dfail(TBK_ERR_INVALID, "NULL argument");
    *k = 0;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return dfail(TBK_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    uint8_t head[4096];
    size_t got = 0;
    for (;;) {
        const ssize_t r = ::read(fd, head + got, sizeof head - got);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0) {
            const int err = errno;
            ::close(fd);
            return dfail(TBK_ERR_IO, "%s: %s", path, strerror(err));
        }
        got += (size_t)r;
        if (r == 0 || got == sizeof head) break;
    }
    ::close(fd);
    if (!got) return dfail(TBK_ERR_FORMAT, "%s: an empty dump has no line to take k from", path);
    const int64_t first = tbk_dump_first_k(head, got);
    if (first < 0) return dfail(TBK_ERR_FORMAT, "%s: line 1: no tab or space behind the k-mer", path);
    if (first < 1 || first > 32) return dfail(TBK_ERR_FORMAT, "%s: line 1: a k-mer of %lld bases (k must lie in 1..32)", path, (long long)first);
    *k = (int)first;
    return TBK_OK;
}

extern "C" int tbk_kmerdb_import_text(const char *const *paths, int n_paths, const tbk_dump_options *opts, int device, tbk_kmerdb **out) {
    if (out) *out = nullptr;
    if (!out || !paths || n_paths < 1) return dfail(TBK_ERR_INVALID, "tbk_kmerdb_import_text: NULL argument or no file");
    tbk_dump_options o;
    tbk_dump_options_init(&o);
    if (opts) {
        if (opts->size < offsetof(tbk_dump_options, floor) + sizeof(int) || opts->size > 4096)
            return dfail(TBK_ERR_INVALID, "tbk_dump_options.size = %zu: set it with tbk_dump_options_init", (size_t)opts->size);
        memcpy(&o, opts, std::min<size_t>(opts->size, sizeof o));
        o.size = sizeof o;
    }
    if (o.k < 0 || o.k > 32) return dfail(TBK_ERR_INVALID, "k = %d out of range (1..32, or 0: taken from the first line)", o.k);
    if (o.floor < 0 || o.floor > 2) return dfail(TBK_ERR_INVALID, "floor = %d (0: auto, 1: keep the k-mers seen once, 2: leave them out)", o.floor);
    if (o.window_bytes && o.window_bytes < TBK_DUMP_MIN_WINDOW)
        return dfail(TBK_ERR_INVALID, "window_bytes = %llu: a window takes at least %llu bytes", (unsigned long long)o.window_bytes, (unsigned long long)TBK_DUMP_MIN_WINDOW);
    Import im;
    im.device = device;
    im.files.resize((size_t)n_paths);
    uint64_t largest = 0;
    for (int i = 0; i < n_paths; i++) {
        if (!paths[i]) return dfail(TBK_ERR_INVALID, "tbk_kmerdb_import_text: path %d is NULL", i);
        const int rc = map_file(paths[i], &im.files[(size_t)i]);
        if (rc) return rc;
        largest = std::max(largest, im.files[(size_t)i].size);
    }
    int k = o.k;
    for (size_t i = 0; !k && i < im.files.size(); i++) {
        const MappedFile &f = im.files[i];
        if (!f.size) continue;
        const int64_t first = tbk_dump_first_k(f.text, std::min<uint64_t>(f.size, 4096));
        if (first < 0) return dfail(TBK_ERR_FORMAT, "%s: line 1: %s", f.path.c_str(), TBK_DUMP_REASONS[7]);
        if (first < 1 || first > 32) return dfail(TBK_ERR_FORMAT, "%s: line 1: a k-mer of %lld bases (k must lie in 1..32)", f.path.c_str(), (long long)first);
        k = (int)first;
    }
    if (!k) return dfail(TBK_ERR_FORMAT, "%s: k = 0 and every dump is empty: no line to take k from", im.files[0].path.c_str());

    // the windows, and the most pairs a sound text can hold: a line takes k + 3 bytes or more, a file's last one k + 2
    const uint64_t window = std::min(o.window_bytes ? o.window_bytes : TBK_DUMP_WINDOW, std::max(largest, TBK_DUMP_MIN_WINDOW));
    std::vector<Window> windows;
    uint64_t capacity = 0;
    for (size_t i = 0; i < im.files.size(); i++) {
        const MappedFile &f = im.files[i];
        capacity += (f.size + 1) / (uint64_t)(k + 3);
        for (uint64_t pos = 0; pos < f.size;) {
            const uint64_t end = tbk_dump_window_end(f.text, f.size, pos, window);
            windows.push_back(Window{(uint32_t)i, pos, end});
            if (end == pos) break;
            pos = end;
        }
        if (!windows.empty() && windows.back().end == windows.back().begin) break;  // (nothing behind a line too long is looked at)
    }

    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return dfail(TBK_ERR_NO_DEVICE, "no HIP device visible; libtbk_hip has no CPU fallback");
    DHIP(hipSetDevice(device));
    g_imports.fetch_add(1);

    uint64_t n = 0;                  // lines so far = pairs so far
    uint64_t *d_keys = nullptr;
    uint8_t *d_counts = nullptr;
    unsigned long long *d_words = nullptr;  // [0] the bad-line minimum, [1 .. 259] the check's tally, [260 .. 515] a histogram
    unsigned long long bad = TBK_DUMP_NO_BAD;
    struct Placed { uint64_t first_line; uint32_t file; uint64_t file_line; };  // where a launched window's first line lies
    std::vector<Placed> placed;
    const Window *too_long = nullptr;

    if (!windows.empty()) {
        const uint32_t tile = tbk_dump_tile();
        const uint64_t max_tiles = (window + tile - 1) / tile;
        uint8_t *d_text = nullptr;
        uint64_t *d_nl = nullptr;
        unsigned long long *d_tiles = nullptr;
        DHIP(hipStreamCreateWithFlags(&im.stream, hipStreamNonBlocking));
        for (auto &set : im.ev)
            for (hipEvent_t &e : set) DHIP(hipEventCreate(&e));
        DHIP(im.alloc((void **)&d_words, 516 * sizeof(unsigned long long)));
        DHIP(im.alloc((void **)&d_text, (size_t)(max_tiles * tile + 64)));
        DHIP(im.alloc((void **)&d_nl, (size_t)(max_tiles * 64 * sizeof(uint64_t))));
        DHIP(im.alloc((void **)&d_tiles, (size_t)(2 * (max_tiles + 1) * sizeof(unsigned long long))));
        DHIP(im.alloc((void **)&d_keys, (size_t)capacity * sizeof(uint64_t)));
        DHIP(im.alloc((void **)&d_counts, (size_t)capacity));
        for (uint8_t *&p : im.pin)
            if (!(p = (uint8_t *)tbk_pin_alloc_((size_t)window))) return dfail(TBK_ERR_NOMEM, "tbk_kmerdb_import_text: no pinned memory for a window of %llu bytes", (unsigned long long)window);
        DHIP(hipMemsetAsync(d_words, 0xFF, sizeof(unsigned long long), im.stream));
        DHIP(hipMemsetAsync(d_words + 1, 0, 515 * sizeof(unsigned long long), im.stream));

        auto stage = [&](size_t w) {
            const Window &win = windows[w];
            if (win.end > win.begin) memcpy(im.pin[w & 1], im.files[win.file].text + win.begin, (size_t)(win.end - win.begin));
        };
        auto timed = [&](size_t w) {  // the two kernels of window w, which has completed
            float a = 0, b = 0;
            if (hipEventElapsedTime(&a, im.ev[w & 1][0], im.ev[w & 1][1]) == hipSuccess && hipEventElapsedTime(&b, im.ev[w & 1][2], im.ev[w & 1][3]) == hipSuccess)
                g_parse_us.fetch_add((uint64_t)((double)(a + b) * 1000.0));
            else
                (void)hipGetLastError();
        };
        stage(0);
        for (size_t w = 0; w < windows.size(); w++) {
            const Window &win = windows[w];
            if (win.end == win.begin) {  // a line longer than a window: the first damage unless an earlier window holds one
                too_long = &win;
                break;
            }
            const uint64_t len = win.end - win.begin, tiles = (len + tile - 1) / tile;
            MappedFile &f = im.files[win.file];
            DHIP(hipMemcpyAsync(d_text, im.pin[w & 1], (size_t)len, hipMemcpyHostToDevice, im.stream));
            DHIP(hipEventRecord(im.ev[w & 1][0], im.stream));
            DHIP(tbk_launch_dump_lines(d_text, len, d_nl, d_tiles, im.stream));
            DHIP(hipEventRecord(im.ev[w & 1][1], im.stream));
            DHIP(hipMemsetAsync(d_tiles + tiles, 0, sizeof(unsigned long long), im.stream));
            if (w + 1 < windows.size()) stage(w + 1);  // (beside the copy and the launch above; its buffer's last copy completed a window ago)
            unsigned long long home[2] = {0, 0};       // newlines of the window; the bad-line minimum of the windows before it
            DHIP(tbk_launch_kmerdb_scan(d_tiles, d_tiles + tiles + 1, tiles + 1, im.stream));
            DHIP(hipMemcpyAsync(&home[0], d_tiles + 2 * tiles + 1, sizeof home[0], hipMemcpyDeviceToHost, im.stream));
            DHIP(hipMemcpyAsync(&home[1], d_words, sizeof home[1], hipMemcpyDeviceToHost, im.stream));
            DHIP(hipStreamSynchronize(im.stream));
            if (w) timed(w - 1);
            if (home[1] != TBK_DUMP_NO_BAD) {  // (windows complete in order: no later one holds an earlier line)
                bad = home[1];
                break;
            }
            const uint64_t lines = home[0] + (f.text[win.end - 1] != '\n' ? 1 : 0);
            placed.push_back(Placed{n, win.file, f.lines});
            DHIP(hipEventRecord(im.ev[w & 1][2], im.stream));
            DHIP(tbk_launch_dump_parse(d_text, len, d_nl, d_tiles + tiles + 1, k, o.compressed != 0, n, capacity, d_keys, d_counts, d_words, im.stream));
            DHIP(hipEventRecord(im.ev[w & 1][3], im.stream));
            n += lines;
            f.lines += lines;
            g_windows.fetch_add(1);
        }
        if (bad == TBK_DUMP_NO_BAD) {
            DHIP(hipMemcpyAsync(&bad, d_words, sizeof bad, hipMemcpyDeviceToHost, im.stream));
            DHIP(hipStreamSynchronize(im.stream));
            if (!placed.empty() && (too_long || placed.size() == windows.size())) timed(placed.size() - 1);
        }
        im.release(d_text);
        im.release(d_nl);
        im.release(d_tiles);
        for (uint8_t *&p : im.pin) { tbk_pin_free_(p); p = nullptr; }
    }
    g_lines.fetch_add(n);
    if (bad != TBK_DUMP_NO_BAD) {
        const uint64_t line = bad >> 8, reason = bad & 0xFF;
        size_t w = placed.size();
        while (w > 1 && placed[w - 1].first_line > line) w--;
        if (!w || reason == 0 || reason >= sizeof TBK_DUMP_REASONS / sizeof *TBK_DUMP_REASONS)
            return dfail(TBK_ERR_HIP, "tbk_kmerdb_import_text: the device reports line %llu, reason %llu", (unsigned long long)line, (unsigned long long)reason);
        const Placed &p = placed[w - 1];
        return dfail(TBK_ERR_FORMAT, "%s: line %llu: %s", im.files[p.file].path.c_str(), (unsigned long long)(p.file_line + (line - p.first_line) + 1),
                     TBK_DUMP_REASONS[reason]);
    }
    if (too_long) {
        const MappedFile &f = im.files[too_long->file];
        return dfail(TBK_ERR_FORMAT, "%s: line %llu: %s", f.path.c_str(), (unsigned long long)(f.lines + 1), TBK_DUMP_REASONS[1]);
    }
    if (n > capacity) return dfail(TBK_ERR_HIP, "tbk_kmerdb_import_text: %llu lines in a text that holds %llu at most", (unsigned long long)n, (unsigned long long)capacity);

    // ---- the pairs: in order? else sorted and folded; then the floor and the header ---------------------------------------------
    uint64_t hist[256] = {0};
    unsigned long long words[516];
    if (n) {
        DHIP(tbk_launch_kmerdb_check(d_keys, d_counts, n, k, 1, d_words + 1, im.stream));
        DHIP(hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, im.stream));
        DHIP(hipStreamSynchronize(im.stream));
        if (words[2] || words[3]) return dfail(TBK_ERR_HIP, "tbk_kmerdb_import_text: %llu keys above 2k bits, %llu counters of 0 among the parsed pairs", words[2], words[3]);
        if (words[1]) {  // some key does not exceed the one before it
            uint64_t *d_k2 = nullptr;
            uint8_t *d_c2 = nullptr;
            DHIP(im.alloc((void **)&d_k2, (size_t)n * sizeof(uint64_t)));
            DHIP(im.alloc((void **)&d_c2, (size_t)n));
            DHIP(tbk_launch_sort_u64_u8(d_keys, d_k2, d_counts, d_c2, n, 2 * k, im.stream));
            g_sorts.fetch_add(1);
            im.release(d_keys);
            im.release(d_counts);
            d_keys = nullptr;
            d_counts = nullptr;
            Compaction heads;
            unsigned long long m = 0;
            DHIP(im.reserve(heads, n));
            DHIP(tbk_launch_dump_heads(d_k2, n, heads.d_flags, heads.counts(), im.stream));
            DHIP(heads.total(&m));
            if (!m || m > n) return dfail(TBK_ERR_HIP, "tbk_kmerdb_import_text: %llu distinct keys among %llu pairs", m, (unsigned long long)n);
            DHIP(im.alloc((void **)&d_keys, (size_t)m * sizeof(uint64_t)));
            DHIP(im.alloc((void **)&d_counts, (size_t)m));
            DHIP(tbk_launch_dump_fold(d_k2, d_c2, n, heads.d_flags, heads.offsets(), d_keys, d_counts, m, im.stream));
            DHIP(tbk_launch_kmerdb_tally(d_counts, m, d_words + 260, im.stream));
            DHIP(hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, im.stream));
            DHIP(hipStreamSynchronize(im.stream));
            heads.release();
            im.release(d_k2);
            im.release(d_c2);
            n = m;
            for (int c = 0; c < 256; c++) hist[c] = words[260 + c];
        } else {
            for (int c = 0; c < 256; c++) hist[c] = words[4 + c];
        }
    }
    uint64_t tallied = 0;
    for (int c = 1; c < 256; c++) tallied += hist[c];
    if (hist[0] || tallied != n) return dfail(TBK_ERR_HIP, "tbk_kmerdb_import_text: %llu of %llu counters tallied, %llu of them 0", (unsigned long long)tallied, (unsigned long long)n, (unsigned long long)hist[0]);
    hist[0] = n;  // all distinct k-mers
    const int floor = o.floor ? o.floor : (hist[1] ? 1 : 2);
    if (floor == 2 && hist[1]) {  // the k-mers seen once leave the entries and stay in row 1
        const uint64_t want = n - hist[1];
        Compaction solid;
        unsigned long long total = 0;
        uint64_t *d_k2 = nullptr;
        uint8_t *d_c2 = nullptr;
        DHIP(im.reserve(solid, n));
        DHIP(tbk_launch_kmerdb_flag(d_keys, d_counts, n, nullptr, 0, 2, 255, solid.d_flags, solid.counts(), im.stream));
        DHIP(solid.total(&total));
        if (total != want) return dfail(TBK_ERR_HIP, "tbk_kmerdb_import_text: %llu counters of 2 or more, the tally states %llu", total, (unsigned long long)want);
        if (want) {
            DHIP(im.alloc((void **)&d_k2, (size_t)want * sizeof(uint64_t)));
            DHIP(im.alloc((void **)&d_c2, (size_t)want));
            DHIP(tbk_launch_kmerdb_scatter_pairs(d_keys, d_counts, n, solid.d_flags, solid.offsets(), d_k2, d_c2, want, im.stream));
            DHIP(hipStreamSynchronize(im.stream));
        }
        solid.release();
        im.release(d_keys);
        im.release(d_counts);
        d_keys = d_k2;
        d_counts = d_c2;
        n = want;
    }
    if (!n) {
        im.release(d_keys);
        im.release(d_counts);
        d_keys = nullptr;
        d_counts = nullptr;
    }
    if (im.stream) DHIP(hipStreamSynchronize(im.stream));
    const int rc = tbk_kmerdb_make_(d_keys, d_counts, n, k, device, floor, o.compressed != 0, hist, o.reads, o.bases, out);
    if (rc) return rc;
    im.disown(d_keys);
    im.disown(d_counts);
    return TBK_OK;
}

// ---- export ---------------------------------------------------------------------------------------------------------------
constexpr uint64_t TBK_DUMP_COPY_PIECE = (uint64_t)1 << 22;   // entries per copy home
constexpr uint64_t TBK_DUMP_TEXT_PIECE = (uint64_t)1 << 16;   // entries per piece of text

static double g_dump_ms[3] = {0, 0, 0};  // the last export: selection, copy home, format + write (tools/measure_dump.py)
extern "C" int tbk_dump_export_timing_(double ms[3]) {
    if (!ms) return dfail(TBK_ERR_INVALID, "NULL argument");
    memcpy(ms, g_dump_ms, sizeof g_dump_ms);
    return TBK_OK;
}

static double now_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec / 1e6;
}

// `KMER\tCOUNT\n` for n entries in host memory to path + ".tmp", renamed when complete.  Lines vary in length: every piece's
// bytes are counted first and the pieces placed by the prefix sum of those, then formatted and written by the host's threads.
static int write_counted(const char *path, const uint64_t *keys, const uint8_t *counts, uint64_t n, int k) {
    const std::string tmp = std::string(path) + ".tmp";
    const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return dfail(TBK_ERR_IO, "cannot create %s: %s", tmp.c_str(), strerror(errno));
    const uint64_t pieces = (n + TBK_DUMP_TEXT_PIECE - 1) / TBK_DUMP_TEXT_PIECE;
    std::vector<uint64_t> bytes((size_t)pieces), at((size_t)pieces + 1);
    std::atomic<uint64_t> next{0};
    std::atomic<bool> ok{true};
    const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)tbk_host_threads(), pieces));
    auto run = [&](auto &&work) {
        next.store(0);
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(work);
        work();
        for (std::thread &t : pool) t.join();
    };
    run([&]() {
        for (uint64_t p; (p = next.fetch_add(1)) < pieces;) {
            const uint64_t lo = p * TBK_DUMP_TEXT_PIECE, hi = std::min(n, lo + TBK_DUMP_TEXT_PIECE);
            bytes[(size_t)p] = tbk_dump_piece_bytes(counts + lo, hi - lo, k);
        }
    });
    tbk_dump_piece_offsets(bytes.data(), pieces, at.data());
    run([&]() {
        std::vector<char> buf;
        for (uint64_t p; (p = next.fetch_add(1)) < pieces && ok.load();) {
            const uint64_t lo = p * TBK_DUMP_TEXT_PIECE, hi = std::min(n, lo + TBK_DUMP_TEXT_PIECE);
            buf.resize((size_t)bytes[(size_t)p]);
            tbk_dump_format_piece(keys + lo, counts + lo, hi - lo, k, buf.data());
            size_t done = 0;
            while (done < buf.size()) {
                const ssize_t r = ::pwrite(fd, buf.data() + done, buf.size() - done, (off_t)(at[(size_t)p] + done));
                if (r < 0 && errno == EINTR) continue;
                if (r <= 0) { ok.store(false); break; }
                done += (size_t)r;
            }
        }
    });
    const int werr = errno;
    const bool closed = ::close(fd) == 0;
    if (!ok.load() || !closed || ::rename(tmp.c_str(), path) != 0) {
        const int rerr = errno;
        (void)::unlink(tmp.c_str());
        return dfail(TBK_ERR_IO, "cannot write %s: %s", path, strerror(!ok.load() ? werr : rerr));
    }
    return TBK_OK;
}

extern "C" int tbk_kmerdb_dump_text(const tbk_kmerdb *db, uint32_t min_count, uint32_t max_count, const char *out_path, uint64_t *n_written) {
    if (!db || !out_path || !n_written) return dfail(TBK_ERR_INVALID, "NULL argument");
    *n_written = 0;
    int k = 0, device = 0, floor = 2;
    uint64_t n = 0, hist[256];
    const uint64_t *db_keys = nullptr;
    const uint8_t *db_counts = nullptr;
    int rc = tbk_kmerdb_info(db, &k, &n, &device, nullptr);
    if (!rc) rc = tbk_kmerdb_floor(db, &floor);
    if (!rc) rc = tbk_kmerdb_histogram(db, hist);
    if (!rc) rc = tbk_kmerdb_arrays_(db, &db_keys, &db_counts);
    if (rc) return rc;
    const uint32_t lo = std::max<uint32_t>((uint32_t)floor, min_count), hi = std::min<uint32_t>(255, max_count);
    uint64_t want = 0;
    for (uint32_t c = lo; c <= hi; c++) want += hist[c];
    want = std::min(want, n);
    std::vector<uint64_t> keys((size_t)want);
    std::vector<uint8_t> counts((size_t)want);
    double t0 = now_ms(), t1 = t0, t2 = t0;
    if (want) {
        Import im;  // (the owner of what this call allocates)
        im.device = device;
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return dfail(TBK_ERR_NO_DEVICE, "no HIP device visible; libtbk_hip has no CPU fallback");
        DHIP(hipSetDevice(device));
        DHIP(hipStreamCreateWithFlags(&im.stream, hipStreamNonBlocking));
        const uint64_t *d_keys = db_keys;
        const uint8_t *d_counts = db_counts;
        if (want < n) {  // flag, scan, scatter: the selected entries in their order
            Compaction sel;
            unsigned long long total = 0;
            uint64_t *d_k2 = nullptr;
            uint8_t *d_c2 = nullptr;
            DHIP(im.reserve(sel, n));
            DHIP(tbk_launch_dump_select(db_counts, n, lo, hi, sel.d_flags, sel.counts(), im.stream));
            DHIP(sel.total(&total));
            if (total != want) return dfail(TBK_ERR_HIP, "tbk_kmerdb_dump_text: %llu entries selected, the histogram states %llu", total, (unsigned long long)want);
            DHIP(im.alloc((void **)&d_k2, (size_t)want * sizeof(uint64_t)));
            DHIP(im.alloc((void **)&d_c2, (size_t)want));
            DHIP(tbk_launch_kmerdb_scatter_pairs(db_keys, db_counts, n, sel.d_flags, sel.offsets(), d_k2, d_c2, want, im.stream));
            DHIP(hipStreamSynchronize(im.stream));
            sel.release();
            d_keys = d_k2;
            d_counts = d_c2;
        }
        t1 = now_ms();
        for (uint64_t at = 0; at < want; at += TBK_DUMP_COPY_PIECE) {
            const uint64_t m = std::min(TBK_DUMP_COPY_PIECE, want - at);
            DHIP(hipMemcpyAsync(keys.data() + at, d_keys + at, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost, im.stream));
            DHIP(hipMemcpyAsync(counts.data() + at, d_counts + at, (size_t)m, hipMemcpyDeviceToHost, im.stream));
        }
        DHIP(hipStreamSynchronize(im.stream));
    }
    t2 = now_ms();
    rc = write_counted(out_path, keys.data(), counts.data(), want, k);
    if (rc) return rc;
    g_dump_ms[0] = t1 - t0;
    g_dump_ms[1] = t2 - t1;
    g_dump_ms[2] = now_ms() - t2;
    *n_written = want;
    return TBK_OK;
}
