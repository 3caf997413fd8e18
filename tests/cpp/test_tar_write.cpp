// The host assembly of a tar image (compu_amd/csrc/tar_write_core.h) in a stand-alone program, for the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o test_tar_write test_tar_write.cpp
//   test_tar_write DIR N
// DIR holds K.in and K.want for K = 0 .. N.  K.in is one case: eight u64 (n, names_len, content bytes, stated content_len, flags,
// record_bytes, arithmetic, 0) | n sources | names | content.  K.want is what the reference (tests/tar_write_ref.py) made of it:
// the 56 bytes of the summary | u64 rows | the 72-byte rows | the image.
// Every case is written from heap buffers of exactly their lengths into a heap buffer of exactly out_len bytes and a heap array of
// exactly n entries, planned again by tar::plan_host, then written once more with one byte less room (nothing may be written) and
// without an entries array.  An arithmetic case is run with no room only; its content is never touched.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../compu_amd/csrc/tar_write_core.h"

using namespace chip;

static int failures = 0;
#define CHECK(cond, ...)                \
    do {                                \
        if (!(cond)) {                  \
            failures++;                 \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");      \
        }                               \
    } while (0)

static std::vector<uint8_t> read_file(const std::string &path)
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

// exactly `count` items on the heap (NULL for none), so that one byte too far is the sanitizer's
template <class T>
static T *exact(const uint8_t *from, size_t count)
{
    if (!count) return nullptr;
    T *p = (T *)malloc(count * sizeof(T));
    memcpy(p, from, count * sizeof(T));
    return p;
}

struct Case {
    uint64_t n = 0, names_len = 0, content_bytes = 0, content_len = 0, flags = 0, record_bytes = 0, arith = 0;
    chip_tar_source *src = nullptr;
    uint8_t *names = nullptr, *content = nullptr;
    void load(const std::vector<uint8_t> &in)
    {
        uint64_t head[8];
        memcpy(head, in.data(), sizeof head);
        n = head[0], names_len = head[1], content_bytes = head[2], content_len = head[3], flags = head[4], record_bytes = head[5], arith = head[6];
        const uint8_t *p = in.data() + sizeof head;
        src = exact<chip_tar_source>(p, n), p += n * sizeof(chip_tar_source);
        names = exact<uint8_t>(p, names_len), p += names_len;
        content = exact<uint8_t>(p, content_bytes), p += content_bytes;
        if (p != in.data() + in.size()) {
            fprintf(stderr, "a case file of %zu bytes, its header says %zu\n", in.size(), (size_t)(p - in.data()));
            exit(2);
        }
    }
    void write(uint8_t *out, uint64_t out_cap, chip_tar_entry *entries, chip_tar_write_summary *s) const
    {
        tarw::write_host(n, src, names, names_len, content, content_len, (uint32_t)flags, (uint32_t)record_bytes, out, out_cap, entries, s);
    }
    ~Case() { free(src), free(names), free(content); }
};

int main(int argc, char **argv)
{
    static_assert(sizeof(chip_tar_source) == 64 && sizeof(chip_tar_write_summary) == 56 && sizeof(chip_tar_entry) == 72, "layout");
    if (argc < 3) {
        fprintf(stderr, "usage: test_tar_write DIR N\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int n_cases = atoi(argv[2]);
    uint64_t runs = 0;
    for (int k = 0; k < n_cases; k++) {
        const std::string what = "case " + std::to_string(k);
        const char *w = what.c_str();
        Case c;
        c.load(read_file(dir + "/" + std::to_string(k) + ".in"));
        const std::vector<uint8_t> want = read_file(dir + "/" + std::to_string(k) + ".want");
        chip_tar_write_summary ws;
        uint64_t n_rows;
        memcpy(&ws, want.data(), sizeof ws);
        memcpy(&n_rows, want.data() + sizeof ws, 8);
        const uint8_t *want_rows = want.data() + sizeof ws + 8, *want_data = want_rows + n_rows * sizeof(chip_tar_entry);
        const uint64_t want_len = want.size() - (sizeof ws + 8 + n_rows * sizeof(chip_tar_entry));

        // sizes first: no room, no entries
        chip_tar_write_summary s;
        memset(&s, 0xee, sizeof s);
        c.write(nullptr, 0, nullptr, &s);
        runs++;
        if (ws.status == CHIP_TARW_BAD_SOURCE) {
            CHECK(memcmp(&s, &ws, sizeof s) == 0, "%s: the summary of a bad source differs", w);
            chip_tar_entry *rows = c.n ? (chip_tar_entry *)malloc(c.n * sizeof(chip_tar_entry)) : nullptr;
            if (rows) memset(rows, 0xa7, c.n * sizeof(chip_tar_entry));
            c.write(nullptr, 0, rows, &s);
            for (uint64_t i = 0; i < c.n * sizeof(chip_tar_entry); i++) CHECK(((uint8_t *)rows)[i] == 0xa7, "%s: an entry was written for a bad source", w);
            free(rows);
            continue;
        }
        CHECK(s.out_len == ws.out_len && s.end_off == ws.end_off && s.n_ext == ws.n_ext && s.total_size == ws.total_size && s.n_entries == ws.n_entries &&
                  s.status == CHIP_TARW_NEED_OUTPUT,
              "%s: the sizing call differs from the reference", w);
        CHECK(n_rows == c.n, "%s: %llu rows in the reference", w, (unsigned long long)n_rows);
        uint64_t names_total = 0, content_total = 0;
        for (uint64_t i = 0; i < c.n; i++) names_total += (uint64_t)c.src[i].name_len + c.src[i].link_len, content_total += c.src[i].size;
        CHECK(tarw::write_bound(c.n, names_total, content_total, (uint32_t)c.record_bytes) >= s.out_len, "%s: the bound", w);
        chip_tar_entry *rows = c.n ? (chip_tar_entry *)malloc(c.n * sizeof(chip_tar_entry)) : nullptr;
        if (c.arith) {
            c.write(nullptr, 0, rows, &s);
            runs++;
            CHECK(memcmp(&s, &ws, sizeof s) == 0, "%s: the summary differs from the reference", w);
            CHECK(!c.n || memcmp(rows, want_rows, c.n * sizeof(chip_tar_entry)) == 0, "%s: the entries differ from the reference", w);
            free(rows);
            continue;
        }
        // exactly out_len bytes
        const uint64_t len = s.out_len;
        uint8_t *out = (uint8_t *)malloc(len);
        memset(out, 0xa7, len);
        memset(&s, 0xee, sizeof s);
        c.write(out, len, rows, &s);
        runs++;
        CHECK(memcmp(&s, &ws, sizeof s) == 0, "%s: the summary differs from the reference", w);
        CHECK(len == want_len && memcmp(out, want_data, len) == 0, "%s: the image differs from the reference", w);
        CHECK(!c.n || memcmp(rows, want_rows, c.n * sizeof(chip_tar_entry)) == 0, "%s: the entries differ from the reference", w);
        // what it wrote is what the plan reads
        chip_tar_plan_summary ps;
        chip_tar_entry *planned = c.n ? (chip_tar_entry *)malloc(c.n * sizeof(chip_tar_entry)) : nullptr;
        tar::plan_host(out, len, c.n, planned, &ps);
        CHECK(ps.status == CHIP_TAR_OK && ps.n_entries == c.n && ps.zero_blocks == 2 && ps.stop_off == s.end_off && ps.total_size == s.total_size,
              "%s: the plan of the image", w);
        CHECK(!c.n || memcmp(planned, rows, c.n * sizeof(chip_tar_entry)) == 0, "%s: the plan's entries differ from the answered ones", w);
        free(planned);
        // one byte less room: a buffer of that size, which must stay as it is; and no entries array
        uint8_t *small = (uint8_t *)malloc(len - 1);
        memset(small, 0xa7, len - 1);
        chip_tar_write_summary s2;
        c.write(small, len - 1, nullptr, &s2);
        runs++;
        bool intact = true;
        for (uint64_t i = 0; i + 1 < len; i++) intact = intact && small[i] == 0xa7;
        CHECK(intact && s2.status == CHIP_TARW_NEED_OUTPUT && s2.out_len == len, "%s: one byte too little room", w);
        free(small);
        memset(out, 0xa7, len);
        c.write(out, len, nullptr, &s2);
        runs++;
        CHECK(memcmp(out, want_data, len) == 0 && memcmp(&s2, &ws, sizeof s2) == 0, "%s: without an entries array", w);
        free(out);
        free(rows);
    }
    printf("%llu runs, %d failures\n", (unsigned long long)runs, failures);
    if (failures == 0) printf("test result: ok\n");
    return failures ? 1 : 0;
}
