// The host walk of a ZIP directory (compu_amd/csrc/zip_plan_core.h) in a stand-alone program, for the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o test_zip_plan test_zip_plan.cpp
//   test_zip_plan DIR N SMALL...
// DIR holds K.zip and K.want for K = 0 .. N: an archive and the plan the reference walk (tests/zip_ref.py) made of it, the 64 bytes of
// the summary followed by the 56-byte records.  Every archive is planned from a heap buffer of exactly its length into a heap array
// of exactly n_entries records (count, then fill, then fill a part) and compared with the reference.  Of the archives numbered
// SMALL... every prefix and every single-byte corruption is planned as well: no read outside the buffer, no write outside the
// array, and the counting call and the filling call agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../compu_amd/csrc/zip_plan_core.h"

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

static bool same_summary(const chip_zip_plan_summary &a, const chip_zip_plan_summary &b) { return memcmp(&a, &b, sizeof a) == 0; }

// the plan of exactly `len` bytes on the heap: count, fill exactly, fill a part; returns the records
static std::vector<chip_zip_entry> plan_exact(const uint8_t *src, size_t len, chip_zip_plan_summary &s, const char *what)
{
    uint8_t *in = len ? (uint8_t *)malloc(len) : nullptr;
    if (len) memcpy(in, src, len);
    chip_zip_plan_summary counted;
    memset(&counted, 0xee, sizeof counted);
    zip::plan_host(in, len, 0, nullptr, &counted);
    const uint64_t n = counted.n_entries;
    chip_zip_entry *rows = n ? (chip_zip_entry *)malloc(n * sizeof(chip_zip_entry)) : nullptr;
    memset(&s, 0xee, sizeof s);
    zip::plan_host(in, len, n, rows, &s);
    CHECK(same_summary(s, counted), "%s: the counting and the filling call differ", what);
    std::vector<chip_zip_entry> out(rows, rows + n);
    if (n > 1) {
        const uint64_t part = n / 2;
        chip_zip_entry *some = (chip_zip_entry *)malloc(part * sizeof(chip_zip_entry));
        chip_zip_plan_summary s2;
        zip::plan_host(in, len, part, some, &s2);
        CHECK(same_summary(s2, counted) && memcmp(some, rows, part * sizeof(chip_zip_entry)) == 0, "%s: a part of the records differs", what);
        free(some);
    }
    CHECK(s.n_ok <= s.n_entries && (s.status == CHIP_ZIP_OK || s.n_entries == s.bad_index || s.status != CHIP_ZIP_BAD_DIRECTORY), "%s: summary", what);
    for (uint64_t i = 0; i < n; i++) {
        const chip_zip_entry &e = out[i];
        CHECK(e.pad == 0, "%s: pad of entry %llu", what, (unsigned long long)i);
        if (e.status == CHIP_ZIPENT_OK)
            CHECK(e.data_off >= 30 && e.data_off <= s.cd_off && e.comp_size <= s.cd_off - e.data_off, "%s: entry %llu is OK out of range", what,
                  (unsigned long long)i);
        CHECK(e.name_off >= s.cd_off + 46 && e.name_off + e.name_len <= s.cd_off + s.cd_size, "%s: name of entry %llu", what, (unsigned long long)i);
    }
    free(rows);
    free(in);
    return out;
}

int main(int argc, char **argv)
{
    static_assert(sizeof(chip_zip_entry) == 56 && sizeof(chip_zip_plan_summary) == 64, "layout");
    if (argc < 3) {
        fprintf(stderr, "usage: test_zip_plan DIR N SMALL...\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int n_cases = atoi(argv[2]);
    uint64_t plans = 0;
    for (int k = 0; k < n_cases; k++) {
        const std::vector<uint8_t> data = read_file(dir + "/" + std::to_string(k) + ".zip"), want = read_file(dir + "/" + std::to_string(k) + ".want");
        const std::string what = "case " + std::to_string(k);
        chip_zip_plan_summary s;
        const std::vector<chip_zip_entry> rows = plan_exact(data.data(), data.size(), s, what.c_str());
        plans++;
        CHECK(want.size() == sizeof s + rows.size() * sizeof(chip_zip_entry), "%s: %zu records, the reference has %zu bytes", what.c_str(), rows.size(),
              want.size());
        if (want.size() != sizeof s + rows.size() * sizeof(chip_zip_entry)) continue;
        CHECK(memcmp(want.data(), &s, sizeof s) == 0, "%s: the summary differs from the reference", what.c_str());
        CHECK(rows.empty() || memcmp(want.data() + sizeof s, rows.data(), rows.size() * sizeof(chip_zip_entry)) == 0,
              "%s: the records differ from the reference", what.c_str());
    }
    for (int a = 3; a < argc; a++) {
        const std::vector<uint8_t> data = read_file(dir + "/" + argv[a] + ".zip");
        const std::string what = std::string("small case ") + argv[a];
        chip_zip_plan_summary s;
        for (size_t len = 0; len < data.size(); len++, plans++) plan_exact(data.data(), len, s, (what + " prefix").c_str());
        std::vector<uint8_t> d = data;
        const uint8_t masks[3] = {0xff, 0x01, 0x80};
        for (size_t i = 0; i < d.size(); i++) {
            for (uint8_t m : masks) {
                d[i] ^= m;
                plan_exact(d.data(), d.size(), s, (what + " corrupted").c_str());
                d[i] ^= m;
                plans++;
            }
            const uint8_t keep = d[i];  // the two values lengths and offsets are most sensitive to
            d[i] = 0, plan_exact(d.data(), d.size(), s, (what + " zeroed").c_str());
            d[i] = 0xff, plan_exact(d.data(), d.size(), s, (what + " ff").c_str());
            d[i] = keep;
            plans += 2;
        }
    }
    printf("%llu plans, %d failures\n", (unsigned long long)plans, failures);
    if (failures == 0) printf("test result: ok\n");
    return failures ? 1 : 0;
}
