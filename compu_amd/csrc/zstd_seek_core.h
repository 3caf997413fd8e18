// The seek table of zstd's seekable format as include/compu_hip.h defines its walk (chip_zstd_seek_plan_host):
// the footer and the skippable header (what is known before one entry is read), one entry, the verdict on the sums, the serial walk
// over them, and the table's writer.  Plain C++ without a device call, so that a stand-alone program can run it under the
// sanitizers; zstd_seek.hip compiles everything but the two serial loops for the device as well (ZSEEK_HD), so host and device
// judge a table with the same code.  Every read is checked against tail_len first: tail[0 .. tail_len) is all that is ever looked at.
#pragma once
#include <stdint.h>

#include "../../include/compu_hip.h"

#if defined(__HIPCC__)
#define ZSEEK_HD __host__ __device__ inline
#else
#define ZSEEK_HD inline
#endif

namespace chip {

namespace zseek {

constexpr uint32_t FOOTER_MAGIC = 0x8F92EAB1u, SKIP_MAGIC = 0x184D2A5Eu, MAX_FRAMES = 0x8000000u, UNSIZED = 0xFFFFFFFFu;
constexpr uint64_t FIXED = 17;  // skippable header (8) + Number_Of_Frames (4) + descriptor (1) + magic (4)

// four bytes, little endian, at any alignment.  On the device two aligned dword loads at most, both of which hold bytes of the value.
ZSEEK_HD uint32_t le32(const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t *a = (const uint32_t *)(p - mis);
    const uint32_t lo = a[0];
    if (mis == 0) return lo;
    return (lo >> (8u * mis)) | (a[1] << (32u - 8u * mis));
#else
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
#endif
}

ZSEEK_HD void put_le32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

// What the walk knows before it reads an entry.  status CHIP_ZSEEK_OK: the table's n entries of es bytes start at
// tail[tail_len - T + 8]; any other status is the walk's answer.  `known`: n, T and cs go into the summary.
struct Head {
    uint64_t n, T;
    uint32_t cs, es;
    int32_t status;
    bool known;
};

ZSEEK_HD Head head(const uint8_t *tail, uint64_t tail_len, uint64_t file_len)
{
    Head h{0, 0, 0, 8, CHIP_ZSEEK_NO_TABLE, false};
    if (file_len < FIXED) return h;
    if (tail_len < FIXED) {
        h.status = CHIP_ZSEEK_NEED_TAIL, h.T = FIXED;
        return h;
    }
    if (le32(tail + tail_len - 4) != FOOTER_MAGIC) return h;
    h.status = CHIP_ZSEEK_BAD_TABLE;
    const uint32_t desc = tail[tail_len - 5];
    if (desc & 0x7Cu) return h;
    h.cs = desc >> 7, h.es = 8u + 4u * h.cs;
    const uint64_t n = le32(tail + tail_len - 9);
    if (n > MAX_FRAMES) return h;
    const uint64_t T = FIXED + (uint64_t)h.es * n;
    if (T > file_len) return h;
    h.n = n, h.T = T, h.known = true;
    if (tail_len < T) {
        h.status = CHIP_ZSEEK_NEED_TAIL;
        return h;
    }
    if (le32(tail + tail_len - T) != SKIP_MAGIC || le32(tail + tail_len - T + 4) != (uint32_t)(T - 8)) return h;
    h.status = CHIP_ZSEEK_OK;
    return h;
}

struct Entry {
    uint32_t c, d, x;
};
// entry i of a table whose head() is OK
ZSEEK_HD Entry entry(const uint8_t *tail, uint64_t tail_len, const Head &h, uint64_t i)
{
    const uint8_t *e = tail + (tail_len - h.T + 8 + (uint64_t)h.es * i);
    return Entry{le32(e), le32(e + 4), h.cs ? le32(e + 8) : 0u};
}

// the summary of a walk that stopped at the head
ZSEEK_HD chip_zstd_seek_summary head_summary(const Head &h)
{
    chip_zstd_seek_summary s{};
    s.status = h.status;
    if (h.known) s.n_frames = h.n, s.table_bytes = h.T, s.checksums = h.cs;
    else if (h.status == CHIP_ZSEEK_NEED_TAIL) s.table_bytes = h.T;
    return s;
}

// the verdict behind the entries: lowest_unsized = the lowest i with d_i == 0xFFFFFFFF (n: none), C and D the sums
ZSEEK_HD chip_zstd_seek_summary sums_summary(const Head &h, uint64_t file_len, uint64_t lowest_unsized, uint64_t C, uint64_t D)
{
    chip_zstd_seek_summary s = head_summary(h);
    if (lowest_unsized < h.n) s.status = CHIP_ZSEEK_TOO_LARGE, s.bad_index = lowest_unsized;
    else if (C > file_len - h.T) s.status = CHIP_ZSEEK_BAD_LAYOUT;
    else s.frames_bytes = C, s.total_out = D;
    return s;
}

inline bool plan_args_ok(const uint8_t *tail, uint64_t tail_len, uint64_t file_len, uint64_t max_frames, const uint64_t *in_off, const uint32_t *in_len,
                         const uint64_t *out_off, const uint32_t *out_cap, const chip_zstd_seek_summary *summary)
{
    if (!summary || (tail_len && !tail) || tail_len > file_len || file_len > ((uint64_t)1 << 40)) return false;
    return !(max_frames && (!in_off || !in_len || !out_off || !out_cap));
}

// the serial walk (arguments in order)
inline void plan_host(const uint8_t *tail, uint64_t tail_len, uint64_t file_len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len,
                      uint64_t *out_off, uint32_t *out_cap, uint32_t *checksum, chip_zstd_seek_summary *summary)
{
    const Head h = head(tail, tail_len, file_len);
    if (h.status != CHIP_ZSEEK_OK) {
        *summary = head_summary(h);
        return;
    }
    uint64_t C = 0, D = 0, lowest = h.n;
    for (uint64_t i = 0; i < h.n; i++) {
        const Entry e = entry(tail, tail_len, h, i);
        if (e.d == UNSIZED && lowest == h.n) lowest = i;
        if (i < max_frames) {
            in_off[i] = C, in_len[i] = e.c, out_off[i] = D, out_cap[i] = e.d;
            if (checksum) checksum[i] = e.x;
        }
        C += e.c, D += e.d;
    }
    *summary = sums_summary(h, file_len, lowest, C, D);
}

// ---- the writer --------------------------------------------------------------------------------------------------------------
ZSEEK_HD uint64_t table_bytes(uint64_t n, bool cs) { return FIXED + (cs ? 12u : 8u) * n; }

// What thread i of max(n, 1) writes: its entry, the first the skippable header in front, the last the footer behind.  Every byte of
// the table is written once, by a byte store.
ZSEEK_HD void write_part(uint8_t *dst, uint64_t n, const uint32_t *c_len, const uint32_t *d_len, const uint32_t *checksum, uint64_t i)
{
    const uint32_t es = checksum ? 12u : 8u;
    if (i == 0) {
        put_le32(dst, SKIP_MAGIC);
        put_le32(dst + 4, (uint32_t)(table_bytes(n, checksum != nullptr) - 8));
    }
    uint8_t *e = dst + 8 + (uint64_t)es * i;
    if (i < n) {
        put_le32(e, c_len[i]);
        put_le32(e + 4, d_len[i]);
        if (checksum) put_le32(e + 8, checksum[i]);
        e += es;
    }
    if (i + 1 >= n) {
        put_le32(e, (uint32_t)n);
        e[4] = checksum ? 0x80 : 0;  // Seek_Table_Descriptor: the checksum flag, no reserved bit
        put_le32(e + 5, FOOTER_MAGIC);
    }
}

inline bool write_args_ok(uint64_t n, const uint32_t *c_len, const uint32_t *d_len, const void *dst, uint64_t dst_cap, const uint64_t *bytes)
{
    return bytes && n <= MAX_FRAMES && !(n && (!c_len || !d_len)) && !(dst_cap && !dst);
}

inline void write_host(uint64_t n, const uint32_t *c_len, const uint32_t *d_len, const uint32_t *checksum, uint8_t *dst, uint64_t dst_cap, uint64_t *bytes)
{
    *bytes = table_bytes(n, checksum != nullptr);
    if (*bytes > dst_cap) return;
    for (uint64_t i = 0; i < (n ? n : 1); i++) write_part(dst, n, c_len, d_len, checksum, i);
}

}  // namespace zseek

}  // namespace chip
