// compu_amd/csrc/snappy_core.h on its own (no HIP, no GPU): the host walk over a framed stream's chunk headers, the host block
// decoder and CRC-32C, from exact-size heap buffers, so that the address and undefined-behaviour sanitizers see every byte they
// touch.  Built and run by tests/test_snappy_cpu.py:
//   test_snappy_core DIR N_BLOCKS N_FRAMES SMALL...
// DIR holds b<k>.bin / b<k>.want for k < N_BLOCKS (a raw block; want = cap u64, out_len u64, in_used u64, status i32, then the
// content) and f<k>.bin / f<k>.want for k < N_FRAMES (a framed stream; want = the summary as 3 x u64, i32, u32, then the records),
// all written from tests/snappy_ref.py.  Every case must answer exactly that.  SMALL names files ("b3", "f7") whose every truncation
// and every single-byte change is run as well (blocks through the decoder, streams through the walk and, chunk by chunk, the
// decoder and the CRC): those only have to stay inside their buffers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../compu_amd/csrc/snappy_core.h"

using namespace chip;

static std::vector<uint8_t> slurp(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        exit(2);
    }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

struct BlockAnswer {
    std::vector<uint8_t> out;
    uint64_t out_len = 0, in_used = 0;
    int32_t status = 0;
};

// input and output in heap buffers of exactly their sizes
static BlockAnswer decode_block(const uint8_t *data, size_t len, uint64_t cap)
{
    uint8_t *in = (uint8_t *)malloc(len ? len : 1), *out = (uint8_t *)malloc(cap ? cap : 1);
    if (len) memcpy(in, data, len);
    BlockAnswer a;
    a.status = snappy::block_decode_host(in, (uint32_t)len, out, cap, a.out_len, a.in_used);
    if (a.out_len > cap) {
        fprintf(stderr, "out_len %llu beyond cap %llu\n", (unsigned long long)a.out_len, (unsigned long long)cap);
        exit(1);
    }
    a.out.assign(out, out + a.out_len);
    free(in);
    free(out);
    return a;
}

struct WalkAnswer {
    chip_snappy_chunks_summary s;
    std::vector<chip_snappy_chunk> rows;
};

static WalkAnswer walk(const uint8_t *data, size_t len)
{
    uint8_t *in = (uint8_t *)malloc(len ? len : 1);
    if (len) memcpy(in, data, len);
    snappy::MemReader rd{in, len};
    WalkAnswer a;
    a.s = snappy::walk_chunks(rd, len, 0, (chip_snappy_chunk *)nullptr);  // count, then fill into exactly that many records
    const uint64_t n = a.s.n_chunks;
    chip_snappy_chunk *rows = (chip_snappy_chunk *)malloc(n ? n * sizeof(chip_snappy_chunk) : 1);
    const chip_snappy_chunks_summary again = snappy::walk_chunks(rd, len, n, rows);
    if (memcmp(&again, &a.s, sizeof again) != 0) {
        fprintf(stderr, "count and fill disagree\n");
        exit(1);
    }
    a.rows.assign(rows, rows + n);
    free(rows);
    free(in);
    return a;
}

// a stream that need not be sound: the walk, then every chunk it found through the decoder or, uncompressed, the CRC
static void exercise_stream(const uint8_t *data, size_t len)
{
    const WalkAnswer w = walk(data, len);
    for (const chip_snappy_chunk &c : w.rows) {
        if (c.type == 0) {
            decode_block(data + c.offset + 8, c.size - 4, 4096);
        } else {
            std::vector<uint8_t> body(data + c.offset + 8, data + c.offset + 4 + c.size);
            snappy::MemReader rd{body.data(), body.size()};
            (void)snappy::crc32c(rd, 0, body.size());
        }
    }
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::string dir = argv[1];
    const int n_blocks = atoi(argv[2]), n_frames = atoi(argv[3]);
    int failed = 0;
    {
        const uint8_t check[] = "123456789";
        snappy::MemReader rd{check, 9};
        if (snappy::crc32c(rd, 0, 9) != 0xE3069283u || snappy::crc32c(rd, 0, 0) != 0 || snappy::mask(0) != 0xa282ead8u) {
            printf("CRC-32C check value differs\n");
            failed++;
        }
    }
    for (int k = 0; k < n_blocks; k++) {
        const std::vector<uint8_t> data = slurp(dir + "/b" + std::to_string(k) + ".bin"), want = slurp(dir + "/b" + std::to_string(k) + ".want");
        uint64_t w[3];
        int32_t st;
        memcpy(w, want.data(), 24);
        memcpy(&st, want.data() + 24, 4);
        const BlockAnswer a = decode_block(data.data(), data.size(), w[0]);
        if (a.out_len != w[1] || a.in_used != w[2] || a.status != st || want.size() != 28 + a.out_len ||
            (a.out_len && memcmp(a.out.data(), want.data() + 28, a.out_len) != 0)) {
            printf("block case %d differs: got (%llu, %llu, %d)\n", k, (unsigned long long)a.out_len, (unsigned long long)a.in_used, a.status);
            failed++;
        }
    }
    for (int k = 0; k < n_frames; k++) {
        const std::vector<uint8_t> data = slurp(dir + "/f" + std::to_string(k) + ".bin"), want = slurp(dir + "/f" + std::to_string(k) + ".want");
        const WalkAnswer a = walk(data.data(), data.size());
        static_assert(sizeof(chip_snappy_chunks_summary) == 32 && sizeof(chip_snappy_chunk) == 24, "the records tests/snappy_ref.py writes");
        if (want.size() != 32 + a.rows.size() * 24 || memcmp(&a.s, want.data(), 32) != 0 ||
            (a.rows.size() && memcmp(a.rows.data(), want.data() + 32, a.rows.size() * 24) != 0)) {
            printf("stream case %d differs: n_chunks %llu status %d\n", k, (unsigned long long)a.s.n_chunks, a.s.status);
            failed++;
        }
    }
    long runs = 0;
    for (int j = 4; j < argc; j++) {
        const std::vector<uint8_t> data = slurp(dir + "/" + argv[j] + ".bin");
        const bool stream = argv[j][0] == 'f';
        for (size_t cut = 0; cut <= data.size(); cut++, runs++) {
            if (stream) exercise_stream(data.data(), cut);
            else decode_block(data.data(), cut, 4096);
        }
        std::vector<uint8_t> m = data;
        for (size_t i = 0; i < m.size(); i++) {
            for (int v = 0; v < 256; v++, runs++) {
                if (v == data[i]) continue;
                m[i] = (uint8_t)v;
                if (stream) exercise_stream(m.data(), m.size());
                else {
                    decode_block(m.data(), m.size(), 4096);
                    decode_block(m.data(), m.size(), 7);
                }
            }
            m[i] = data[i];
        }
    }
    printf("%d block cases, %d stream cases, %ld truncations and single-byte changes\n", n_blocks, n_frames, runs);
    printf(failed ? "test result: FAILED\n" : "test result: ok\n");
    return failed ? 1 : 0;
}
