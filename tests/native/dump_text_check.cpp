// The host pieces of the counted-dump importer and exporter that need no device (trio_binning_amd/csrc/tbk_dump_text.h),
// run against a mapped file: window cutting, k from the first line, the export's length prefix sum and formatter.
// Stand-alone so that it can be built with -fsanitize=address,undefined on the CPU.  Prints "ok" and exits 0, or says what
// differs and exits 1.
#include <cstdio>
#include <cstdlib>
#include <fcntl.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "tbk_dump_text.h"

static int fail(const char *what, unsigned long long a, unsigned long long b) {
    fprintf(stderr, "dump_text_check: %s: %llu != %llu\n", what, a, b);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: dump_text_check scratch-file\n"); return 2; }
    const int k = 21;
    // entries with every counter 1..255 in turn, ranks spread over the 2k bits; formatted in pieces placed by the prefix sum
    const uint64_t n = 5000, per = 333;
    std::vector<uint64_t> keys(n);
    std::vector<uint8_t> counts(n);
    uint64_t x = 88172645463325252ull;
    for (uint64_t i = 0; i < n; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        keys[i] = x & ((1ull << (2 * k)) - 1);
        counts[i] = (uint8_t)(1 + i % 255);
    }
    const uint64_t pieces = (n + per - 1) / per;
    std::vector<uint64_t> bytes(pieces), at(pieces + 1);
    for (uint64_t p = 0; p < pieces; p++) {
        const uint64_t lo = p * per, hi = lo + per < n ? lo + per : n;
        bytes[p] = tbk_dump_piece_bytes(counts.data() + lo, hi - lo, k);
    }
    tbk_dump_piece_offsets(bytes.data(), pieces, at.data());
    std::vector<char> text(at[pieces]);  // (exactly the bytes stated: one byte more written is the sanitizer's to find)
    for (uint64_t p = pieces; p-- > 0;) {  // (last piece first: a piece's place does not depend on the others being there)
        const uint64_t lo = p * per, hi = lo + per < n ? lo + per : n;
        std::vector<char> piece(bytes[p]);
        const uint64_t wrote = tbk_dump_format_piece(keys.data() + lo, counts.data() + lo, hi - lo, k, piece.data());
        if (wrote != bytes[p]) return fail("bytes of a piece", wrote, bytes[p]);
        memcpy(text.data() + at[p], piece.data(), piece.size());
    }
    // the same text line by line with snprintf
    std::string want;
    for (uint64_t i = 0; i < n; i++) {
        char line[64];
        for (int b = 0; b < k; b++) line[b] = "ACGT"[(keys[i] >> (2 * (k - 1 - b))) & 3];
        const int m = snprintf(line + k, sizeof line - k, "\t%u\n", (unsigned)counts[i]);
        want.append(line, (size_t)(k + m));
    }
    if (want.size() != text.size()) return fail("bytes of the text", text.size(), want.size());
    if (memcmp(want.data(), text.data(), text.size()) != 0) return fail("the text differs", 0, 1);
    // through a file and a mapping: k of line 1, and windows of every size from 64 on that tile the text exactly at newlines
    const int fd = open(argv[1], O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0 || write(fd, text.data(), text.size()) != (ssize_t)text.size()) { perror(argv[1]); return 2; }
    const uint64_t size = text.size();
    const uint8_t *map = (const uint8_t *)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) { perror("mmap"); return 2; }
    if (tbk_dump_first_k(map, size) != k) return fail("k of line 1", (unsigned long long)tbk_dump_first_k(map, size), k);
    if (tbk_dump_first_k(map, 0) != -1 || tbk_dump_first_k((const uint8_t *)"ACGT\nAC 1\n", 10) != -1) return fail("a first line without a separator", 0, 1);
    for (uint64_t window : {64ull, 65ull, 100ull, 4096ull, 4097ull, (unsigned long long)size - 1, (unsigned long long)size, (unsigned long long)size + 1}) {
        uint64_t pos = 0, lines = 0;
        while (pos < size) {
            const uint64_t end = tbk_dump_window_end(map, size, pos, window);
            if (end <= pos || end - pos > window || end > size) return fail("a window's end", end, pos);
            if (map[end - 1] != '\n') return fail("a window does not end behind a newline", end, window);
            for (uint64_t i = pos; i < end; i++) lines += map[i] == '\n';
            pos = end;
        }
        if (lines != n) return fail("lines over all windows", lines, n);
    }
    // a window too small for a line says so; a text without a last newline ends at its size
    if (tbk_dump_window_end(map, size, 0, 10) != 0) return fail("a line longer than the window", tbk_dump_window_end(map, size, 0, 10), 0);
    if (tbk_dump_window_end(map, size - 1, size - 20, 4096) != size - 1) return fail("the end of a text without a last newline", 0, 1);
    if (tbk_dump_window_end(map, size, size, 4096) != size) return fail("a window at the end", 0, 1);
    munmap((void *)map, size);
    close(fd);
    unlink(argv[1]);
    puts("ok");
    return 0;
}
