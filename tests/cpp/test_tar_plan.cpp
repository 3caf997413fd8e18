// The tar walk (compu_amd/csrc/tar_plan_core.h) as a stand-alone host program, for the address and undefined-behaviour sanitizers:
//   test_tar_plan DIR N [K ...]
// reads DIR/0.tar .. DIR/(N-1).tar with DIR/i.want (the summary as 5 u64 and 2 i32, then the records) and compares the walk from a
// heap buffer of exactly the image's size, at an odd address as well, into an array of exactly n_entries records; of the images K
// it also walks every prefix and every single-byte corruption (three values per byte), where only the sanitizers judge.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../compu_amd/csrc/tar_plan_core.h"

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

// the walk over a copy of exactly `len` bytes, `shift` bytes behind the start of its allocation
static chip_tar_plan_summary walk(const uint8_t *data, size_t len, size_t shift, std::vector<chip_tar_entry> &rows)
{
    uint8_t *heap = (uint8_t *)malloc(len + shift ? len + shift : 1);
    if (len) memcpy(heap + shift, data, len);
    chip_tar_plan_summary s;
    chip::tar::plan_host(heap + shift, len, 0, nullptr, &s);
    rows.assign((size_t)s.n_entries, chip_tar_entry{});
    chip_tar_plan_summary s2;
    chip::tar::plan_host(heap + shift, len, s.n_entries, rows.data(), &s2);
    if (memcmp(&s, &s2, sizeof s)) {
        fprintf(stderr, "counting and filling disagree\n");
        exit(1);
    }
    free(heap);
    return s;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int n = atoi(argv[2]);
    static_assert(sizeof(chip_tar_entry) == 72 && sizeof(chip_tar_plan_summary) == 48, "layout");
    std::vector<chip_tar_entry> rows;
    for (int i = 0; i < n; i++) {
        const std::vector<uint8_t> img = slurp(dir + "/" + std::to_string(i) + ".tar"), want = slurp(dir + "/" + std::to_string(i) + ".want");
        for (size_t shift = 0; shift < 2; shift++) {
            const chip_tar_plan_summary s = walk(img.data(), img.size(), shift, rows);
            const size_t bytes = rows.size() * sizeof(chip_tar_entry);
            if (want.size() != sizeof s + bytes || memcmp(want.data(), &s, sizeof s) || (bytes && memcmp(want.data() + sizeof s, rows.data(), bytes))) {
                fprintf(stderr, "image %d: the walk differs from the reference\n", i);
                return 1;
            }
        }
    }
    size_t walks = 0;
    for (int a = 3; a < argc; a++) {
        std::vector<uint8_t> img = slurp(dir + "/" + argv[a] + ".tar");
        for (size_t cut = 0; cut <= img.size(); cut++, walks++) walk(img.data(), cut, cut & 1, rows);
        for (size_t at = 0; at < img.size(); at++) {
            const uint8_t keep = img[at];
            for (uint8_t v : {(uint8_t)(keep ^ 1), (uint8_t)(keep ^ 0x80), (uint8_t)0}) {
                img[at] = v;
                walk(img.data(), img.size(), 0, rows);
                walks++;
            }
            img[at] = keep;
        }
    }
    printf("test result: ok. %d images, %zu prefixes and corruptions\n", n, walks);
    return 0;
}
