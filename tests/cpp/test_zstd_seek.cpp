// The seek-table walk and writer (compu_amd/csrc/zstd_seek_core.h) as a stand-alone host program, for the address and
// undefined-behaviour sanitizers:
//   test_zstd_seek DIR N [K ...]
// reads DIR/0.tail .. DIR/(N-1).tail with DIR/i.want (file_len as u64, the summary's 48 bytes, then the five arrays of the rows one
// after the other) and compares the walk from a heap buffer of exactly the tail's size, at an odd address as well, into arrays of
// exactly the rows' size, counting first; a table that is OK is written again from its rows into a buffer of exactly its size and
// compared with the tail's bytes.  Of the cases K it also walks every single-byte mutation (all 255 values) of the last 17 + 24
// bytes, where only the sanitizers judge.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../compu_amd/csrc/zstd_seek_core.h"

static std::vector<uint8_t> slurp(const std::string &path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        exit(2);
    }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

struct Rows {
    uint64_t *in_off, *out_off;
    uint32_t *in_len, *out_cap, *checksum;
    size_t n;
    explicit Rows(size_t k) : n(k)
    {
        // (exact sizes, so that an entry too many is a heap overflow the sanitizer sees)
        in_off = (uint64_t *)malloc(k ? k * 8 : 1), out_off = (uint64_t *)malloc(k ? k * 8 : 1);
        in_len = (uint32_t *)malloc(k ? k * 4 : 1), out_cap = (uint32_t *)malloc(k ? k * 4 : 1), checksum = (uint32_t *)malloc(k ? k * 4 : 1);
    }
    ~Rows() { free(in_off), free(out_off), free(in_len), free(out_cap), free(checksum); }
    std::vector<uint8_t> bytes() const
    {
        std::vector<uint8_t> v;
        auto put = [&](const void *p, size_t b) { v.insert(v.end(), (const uint8_t *)p, (const uint8_t *)p + b); };
        put(in_off, n * 8), put(in_len, n * 4), put(out_off, n * 8), put(out_cap, n * 4), put(checksum, n * 4);
        return v;
    }
};

// the walk over a copy of exactly `len` bytes, `shift` bytes behind the start of its allocation: counts, then fills
static chip_zstd_seek_summary walk(const uint8_t *data, size_t len, uint64_t file_len, size_t shift, std::vector<uint8_t> *rows_out, bool with_checksum)
{
    uint8_t *heap = (uint8_t *)malloc(len + shift ? len + shift : 1);
    if (len) memcpy(heap + shift, data, len);
    chip_zstd_seek_summary s, s2;
    chip::zseek::plan_host(heap + shift, len, file_len, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &s);
    const size_t k = s.status == CHIP_ZSEEK_OK ? (size_t)s.n_frames : 0;
    Rows r(k);
    chip::zseek::plan_host(heap + shift, len, file_len, k, r.in_off, r.in_len, r.out_off, r.out_cap, with_checksum ? r.checksum : nullptr, &s2);
    if (memcmp(&s, &s2, sizeof s)) {
        fprintf(stderr, "counting and filling disagree\n");
        exit(1);
    }
    if (!with_checksum) memset(r.checksum, 0, k * 4);
    if (rows_out) *rows_out = r.bytes();
    if (s.status == CHIP_ZSEEK_OK && with_checksum && (heap[shift + len - 5] & 3u) == 0) {  // the writer gives the table's bytes back
        uint64_t size = 0;
        uint8_t *dst = (uint8_t *)malloc((size_t)s.table_bytes);
        chip::zseek::write_host(k, r.in_len, r.out_cap, s.checksums ? r.checksum : nullptr, dst, s.table_bytes, &size);
        if (size != s.table_bytes || memcmp(dst, heap + shift + len - s.table_bytes, (size_t)size)) {
            fprintf(stderr, "the writer does not give the table back\n");
            exit(1);
        }
        chip::zseek::write_host(k, r.in_len, r.out_cap, s.checksums ? r.checksum : nullptr, dst, s.table_bytes - 1, &size);  // one short: nothing written
        if (size != s.table_bytes) exit(1);
        free(dst);
    }
    free(heap);
    return s;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int n = atoi(argv[2]);
    static_assert(sizeof(chip_zstd_seek_summary) == 48, "layout");
    std::vector<uint8_t> rows;
    for (int i = 0; i < n; i++) {
        const std::vector<uint8_t> tail = slurp(dir + "/" + std::to_string(i) + ".tail"), want = slurp(dir + "/" + std::to_string(i) + ".want");
        if (want.size() < 8 + sizeof(chip_zstd_seek_summary)) return 2;
        uint64_t file_len;
        memcpy(&file_len, want.data(), 8);
        for (size_t shift = 0; shift < 2; shift++) {
            const chip_zstd_seek_summary s = walk(tail.data(), tail.size(), file_len, shift, &rows, true);
            if (want.size() != 8 + sizeof s + rows.size() || memcmp(want.data() + 8, &s, sizeof s) ||
                (rows.size() && memcmp(want.data() + 8 + sizeof s, rows.data(), rows.size()))) {
                fprintf(stderr, "case %d: the walk differs from the reference\n", i);
                return 1;
            }
            walk(tail.data(), tail.size(), file_len, shift, nullptr, false);  // checksum == NULL
        }
    }
    size_t walks = 0;
    for (int a = 3; a < argc; a++) {
        std::vector<uint8_t> tail = slurp(dir + "/" + argv[a] + ".tail");
        const std::vector<uint8_t> want = slurp(dir + "/" + argv[a] + ".want");
        uint64_t file_len;
        memcpy(&file_len, want.data(), 8);
        const size_t span = tail.size() < 17 + 24 ? tail.size() : 17 + 24;
        for (size_t at = tail.size() - span; at < tail.size(); at++) {
            const uint8_t keep = tail[at];
            for (int v = 0; v < 256; v++) {
                if (v == keep) continue;
                tail[at] = (uint8_t)v;
                walk(tail.data(), tail.size(), file_len, at & 1, nullptr, true);
                walks++;
            }
            tail[at] = keep;
        }
    }
    printf("test result: ok. %d cases, %zu mutations\n", n, walks);
    return 0;
}
