// compu_amd/csrc/lz4_enc_core.h on the host, for a sanitizer build (tests/test_lz4_encoder_cpu.py compiles and runs it):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o test_lz4_enc_core test_lz4_enc_core.cpp
//   test_lz4_enc_core DIR N
// DIR holds e0.bin .. e{N-1}.bin, the built inputs of tests/lz4_enc_cases.py; seeded random inputs are added here.  Every input
// is encoded at one level of each finder group (and both skip rates of the first) into a heap buffer of exactly the bound, then of
// exactly the size (the same bytes) and of one byte less (CHIP_ENC_NEED_OUTPUT); the block is walked sequence by sequence for the
// duties of the format, and decoded by lz4_core.h's host decoder into a buffer of exactly the content's size.  Frames of every
// option are walked with lz4_core.h's walk_blocks, their blocks decoded and their checksums compared.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../compu_amd/csrc/lz4_enc_core.h"

using namespace chip;
typedef std::vector<uint8_t> Bytes;

static int failures = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            failures++;                                 \
            return;                                     \
        }                                               \
    } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static bool read_file(const std::string &path, Bytes &b)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    b.resize((size_t)n);
    const bool ok = n == 0 || fread(b.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

// the duties: sequences of the block, offsets within 1 .. 65535 and the bytes produced, the last match starts 12 and ends 5 bytes
// before the end, a block of fewer than 13 bytes is one run
static void check_duties(const uint8_t *blk, uint32_t len, uint32_t n, const char *name)
{
    uint32_t p = 0, o = 0, n_match = 0;
    for (;;) {
        CHECK(p < len, "%s: token beyond the block", name);
        const uint32_t token = blk[p++];
        uint32_t ll = token >> 4, b;
        if (ll == 15) do { CHECK(p < len, "%s: cut extension", name); b = blk[p++]; ll += b; } while (b == 255);
        CHECK(ll <= len - p, "%s: literals beyond the block", name);
        p += ll;
        o += ll;
        if (p == len) break;
        CHECK(len - p >= 2, "%s: cut offset", name);
        const uint32_t off = blk[p] | (blk[p + 1] << 8);
        p += 2;
        CHECK(off >= 1 && off <= 65535 && off <= o, "%s: offset %u with %u bytes produced", name, off, o);
        uint32_t ml = token & 15;
        if (ml == 15) do { CHECK(p < len, "%s: cut extension", name); b = blk[p++]; ml += b; } while (b == 255);
        ml += 4;
        CHECK((uint64_t)o + 12 <= n, "%s: a match starts at %u of %u", name, o, n);
        CHECK((uint64_t)o + ml + 5 <= n, "%s: a match ends at %u of %u", name, o + ml, n);
        o += ml;
        n_match++;
    }
    CHECK(o == n, "%s: %u bytes for %u", name, o, n);
    CHECK(n >= 13 || n_match == 0, "%s: a match in a block of %u bytes", name, n);
}

static void one_block(const Bytes &in, int level, const char *name)
{
    lz4enc::Cfg c;
    CHECK(lz4enc::level_cfg(level, c), "level");
    const uint64_t bound = lz4enc::block_bound(in.size());
    uint8_t *room = (uint8_t *)malloc(bound);
    uint64_t n = 0;
    int32_t st = lz4enc::block_encode_host(in.data(), in.size(), c, room, bound, n);
    CHECK(st == CHIP_ENC_FINISHED && n >= 1 && n <= bound, "%s level %d: status %d, %llu of %llu", name, level, st, (unsigned long long)n, (unsigned long long)bound);
    check_duties(room, (uint32_t)n, (uint32_t)in.size(), name);
    // exact room, and one byte less
    uint8_t *exact = (uint8_t *)malloc(n);
    uint64_t m = 0;
    st = lz4enc::block_encode_host(in.data(), in.size(), c, exact, n, m);
    CHECK(st == CHIP_ENC_FINISHED && m == n && memcmp(exact, room, n) == 0, "%s level %d: exact room", name, level);
    st = lz4enc::block_encode_host(in.data(), in.size(), c, exact, n - 1, m);
    CHECK(st == CHIP_ENC_NEED_OUTPUT && m == 0, "%s level %d: room - 1 is %d", name, level, st);
    // back through the host decoder, into exactly the content's size
    uint8_t *back = (uint8_t *)malloc(in.size() ? in.size() : 1);
    uint64_t ol = 0, used = 0;
    const int32_t ds = lz4::block_decode_host(room, (uint32_t)n, back, in.size(), ol, used);
    CHECK(ds == CHIP_FINISHED && ol == in.size() && used == n && (in.empty() || memcmp(back, in.data(), in.size()) == 0), "%s level %d: decode %d", name,
          level, ds);
    free(back);
    free(exact);
    free(room);
}

static void one_frame(const Bytes &in, int level, uint32_t opts, const char *name)
{
    lz4enc::Cfg c;
    CHECK(lz4enc::level_cfg(level, c) && lz4enc::frame_opts_ok((int)opts), "arguments");
    const uint64_t bound = lz4enc::frame_bound(in.size());
    uint8_t *room = (uint8_t *)malloc(bound);
    uint64_t n = 0;
    int32_t st = lz4enc::frame_encode_host(in.data(), in.size(), c, opts, room, bound, n);
    CHECK(st == CHIP_ENC_FINISHED && n <= bound, "%s opts %#x: status %d", name, opts, st);
    uint8_t *exact = (uint8_t *)malloc(n);
    uint64_t m = 0;
    st = lz4enc::frame_encode_host(in.data(), in.size(), c, opts, exact, n, m);
    CHECK(st == CHIP_ENC_FINISHED && m == n && memcmp(exact, room, n) == 0, "%s opts %#x: exact room", name, opts);
    st = lz4enc::frame_encode_host(in.data(), in.size(), c, opts, exact, n - 1, m);
    CHECK(st == CHIP_ENC_NEED_OUTPUT && m == 0, "%s opts %#x: room - 1 is %d", name, opts, st);
    free(exact);
    // the walk, then every block
    lz4::MemReader rd{room};
    chip_lz4_blocks_summary s = lz4::walk_blocks(rd, n, 0, nullptr);
    CHECK(s.status == CHIP_ZPLAN_OK && s.in_used == n && s.content_size == in.size(), "%s opts %#x: walk status %d", name, opts, s.status);
    std::vector<chip_lz4_block> blocks(s.n_blocks);
    s = lz4::walk_blocks(rd, n, blocks.size(), blocks.data());
    const uint32_t id = lz4enc::opts_block_id(opts);
    CHECK(s.block_max == (1u << (8 + 2 * id)) && ((s.flg >> 4) & 1u) == (opts & 1u) && ((s.flg >> 2) & 1u) == ((opts & 2u) ? 0u : 1u) && ((s.flg >> 5) & 1u),
          "%s opts %#x: header flg %#x bd %#x", name, opts, s.flg, s.bd);
    CHECK(s.n_blocks == (in.size() + s.block_max - 1) / s.block_max, "%s opts %#x: %llu blocks", name, opts, (unsigned long long)s.n_blocks);
    Bytes back(in.size());
    uint64_t o = 0;
    for (const chip_lz4_block &b : blocks) {
        const uint8_t *body = room + b.offset + 4;
        if (b.flags & CHIP_LZ4BLOCK_STORED) {
            CHECK(o + b.size <= in.size(), "%s: stored block too long", name);
            memcpy(back.data() + o, body, b.size);
            o += b.size;
        } else {
            uint64_t ol = 0, used = 0;
            const int32_t ds = lz4::block_decode_host(body, b.size, back.data() + o, in.size() - o, ol, used);
            CHECK(ds == CHIP_FINISHED && used == b.size && ol <= s.block_max && b.size < ol, "%s: block decode %d", name, ds);
            o += ol;
        }
        if (opts & 1u) {
            lz4::MemReader br{body};
            CHECK(b.checksum == lz4::xxh32(br, 0, b.size, 0), "%s: block checksum", name);
        }
    }
    CHECK(o == in.size() && (in.empty() || memcmp(back.data(), in.data(), in.size()) == 0), "%s opts %#x: content", name, opts);
    if (!(opts & 2u)) {
        lz4::MemReader cr{in.data()};
        CHECK(s.content_checksum == lz4::xxh32(cr, 0, in.size(), 0), "%s: content checksum", name);
    }
    free(room);
}

static Bytes random_input()
{
    Bytes b;
    const uint32_t parts = 1 + rnd() % 6;
    for (uint32_t k = 0; k < parts; k++) {
        const uint32_t n = rnd() % 900, kind = rnd() % 4;
        const size_t at = b.size();
        for (uint32_t i = 0; i < n; i++) {
            if (kind == 0) b.push_back((uint8_t)rnd());
            else if (kind == 1) b.push_back((uint8_t)('a' + rnd() % 3));
            else if (kind == 2 && at + i >= 7) b.push_back(b[at + i - 7]);
            else if (b.size() > 40 && (i % 23)) b.push_back(b[b.size() - 1 - rnd() % 40]);
            else b.push_back((uint8_t)(rnd() % 16));
        }
    }
    return b;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int n_files = atoi(argv[2]);
    const int levels[4] = {1, 2, 4, 9};
    const uint32_t frame_opts[6] = {0, 1, 2, 3, 5u << 4, (7u << 4) | 3};
    int blocks = 0, frames = 0;
    for (int k = 0; k < n_files + 300; k++) {
        Bytes in;
        char name[64];
        if (k < n_files) {
            snprintf(name, sizeof name, "e%d.bin", k);
            if (!read_file(dir + "/" + name, in)) {
                printf("cannot read %s\n", name);
                return 2;
            }
        } else {
            snprintf(name, sizeof name, "random%d", k - n_files);
            in = random_input();
        }
        for (int level : levels) {
            one_block(in, level, name);
            blocks++;
        }
        if (in.size() <= 300000 || k % 4 == 0)
            for (uint32_t opts : frame_opts) {
                one_frame(in, levels[k % 4], opts, name);
                frames++;
            }
    }
    printf("%d blocks, %d frames, %d failures\n", blocks, frames, failures);
    if (failures) return 1;
    printf("test result: ok\n");
    return 0;
}
