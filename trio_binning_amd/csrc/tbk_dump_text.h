// tbk_dump_text.h — the host pieces of the counted-dump importer and exporter that need no device: where a window of text
// ends, k from a dump's first line, and the text of a piece of entries.  Plain C++ without a HIP header, so that
// tests/native/dump_text_check.cpp can run them under AddressSanitizer and UBSan on the CPU.
#ifndef TBK_DUMP_TEXT_H
#define TBK_DUMP_TEXT_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

// The end (exclusive) of the window that begins at `pos` of a text of `size` bytes and takes at most `window` bytes: the
// end of the text when it is that near, else just behind the last newline of those bytes.  Returns `pos` when they hold no
// newline: a line longer than a window.
static inline uint64_t tbk_dump_window_end(const uint8_t *text, uint64_t size, uint64_t pos, uint64_t window) {
    if (pos >= size) return size;
    if (size - pos <= window) return size;
    const void *nl = memrchr(text + pos, '\n', (size_t)window);
    return nl ? (uint64_t)((const uint8_t *)nl - text) + 1 : pos;
}

// The bytes before the first tab or space of line 1; -1 when line 1 has neither (or the text is empty).
static inline int64_t tbk_dump_first_k(const uint8_t *text, uint64_t size) {
    for (uint64_t i = 0; i < size && text[i] != '\n'; i++)
        if (text[i] == '\t' || text[i] == ' ') return (int64_t)i;
    return -1;
}

static inline uint32_t tbk_dump_digits(uint32_t count) { return count >= 100 ? 3u : count >= 10 ? 2u : 1u; }

// bytes of the lines `KMER\tCOUNT\n` of n entries
static inline uint64_t tbk_dump_piece_bytes(const uint8_t *counts, uint64_t n, int k) {
    uint64_t bytes = n * (uint64_t)(k + 2);
    for (uint64_t i = 0; i < n; i++) bytes += tbk_dump_digits(counts[i]);
    return bytes;
}

// Those lines, from lexicographic ranks (base 0 in the top bits of the 2k); `out` has tbk_dump_piece_bytes room.  Returns
// the bytes written.
static inline uint64_t tbk_dump_format_piece(const uint64_t *keys, const uint8_t *counts, uint64_t n, int k, char *out) {
    char *w = out;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t v = keys[i];
        for (int b = 0; b < k; b++) *w++ = "ACGT"[(v >> (2 * (k - 1 - b))) & 3u];
        *w++ = '\t';
        const uint32_t c = counts[i];
        if (c >= 100) *w++ = (char)('0' + c / 100);
        if (c >= 10) *w++ = (char)('0' + c / 10 % 10);
        *w++ = (char)('0' + c % 10);
        *w++ = '\n';
    }
    return (uint64_t)(w - out);
}

// out[i] = lengths[0] + ... + lengths[i - 1] for i in 0..n (n + 1 values): where every piece of a dump begins
static inline void tbk_dump_piece_offsets(const uint64_t *lengths, uint64_t n, uint64_t *out) {
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) {
        out[i] = sum;
        sum += lengths[i];
    }
    out[n] = sum;
}
#endif /* TBK_DUMP_TEXT_H */
