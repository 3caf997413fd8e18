// The walk of a tar image as include/compu_hip.h defines it (chip_tar_plan_host): a number field, the header
// test, the records of a pax extension header, one group (a run of extension headers and the member header they modify), what the
// walk answers where no group starts, and the serial walk over them.  Plain C++ without a device call, so that a stand-alone program
// can run it under the sanitizers; tar.hip compiles everything but the serial walk for the device as well (TAR_HD), so host and
// device read a group with the same code.  Every read is checked against the image's length first: b[0 .. len) is all that is ever
// looked at, and a header is looked at only once its 512 bytes are known to lie in front of `len`.
// A global pax header (typeflag g) is stepped over and counted; its records are neither parsed nor applied to the members behind it.
#pragma once
#include <stdint.h>

#include "../../include/compu_hip.h"

#if defined(__HIPCC__)
#define TAR_HD __host__ __device__ inline
#else
#define TAR_HD inline
#endif

namespace chip {

namespace tar {

constexpr uint64_t BLOCK = 512;
constexpr uint32_t O_NAME = 0, O_MODE = 100, O_SIZE = 124, O_MTIME = 136, O_CHKSUM = 148, O_TYPE = 156, O_LINK = 157, O_MAGIC = 257, O_PREFIX = 345;
constexpr uint32_t N_NAME = 100, N_MODE = 8, N_SIZE = 12, N_MTIME = 12, N_CHKSUM = 8, N_LINK = 100, N_PREFIX = 155;
constexpr uint32_t KIND_MEMBER = 0, KIND_GLOBAL = 1;  // what a whole group is

TAR_HD uint64_t roundup512(uint64_t v) { return (v + (BLOCK - 1)) & ~(BLOCK - 1); }

// a number field of n bytes at f
struct Number {
    uint64_t v;
    bool ok, base256;
};
TAR_HD Number number(const uint8_t *f, uint32_t n)
{
    Number r{0, false, false};
    if (f[0] == 0x80) {
        r.base256 = true;
        for (uint32_t k = 1; k < n; k++) {
            if (r.v >> 55) return r;  // the next byte would reach 2^63
            r.v = (r.v << 8) | f[k];
        }
        r.ok = true;
        return r;
    }
    if (f[0] == 0xFF) return r;
    uint32_t k = 0;
    while (k < n && f[k] == ' ') k++;
    while (k < n && f[k] >= '0' && f[k] <= '7') r.v = (r.v << 3) | (uint64_t)(f[k++] - '0');  // (at most 12 digits: 36 bits)
    r.ok = k == n || f[k] == 0 || f[k] == ' ';
    return r;
}

// the length of the string in f[0 .. n): up to the first NUL, or all n bytes
TAR_HD uint64_t str_len(const uint8_t *f, uint64_t n)
{
    uint64_t k = 0;
    while (k < n && f[k]) k++;
    return k;
}

// four bytes of a header, little endian.  On the device the image is 4-byte aligned and a header sits at a multiple of 512.
TAR_HD uint32_t ld32(const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const uint32_t *)p;
#else
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
#endif
}

TAR_HD bool zero_block(const uint8_t *h)
{
    uint32_t any = 0;
    for (uint32_t k = 0; k < BLOCK; k += 4) any |= ld32(h + k);
    return any == 0;
}

// is_header(p)
TAR_HD bool is_header(const uint8_t *b, uint64_t len, uint64_t p)
{
    if ((p & (BLOCK - 1)) || p > len || len - p < BLOCK) return false;
    const uint8_t *h = b + p;
    if (h[O_MAGIC] != 'u' || h[O_MAGIC + 1] != 's' || h[O_MAGIC + 2] != 't' || h[O_MAGIC + 3] != 'a' || h[O_MAGIC + 4] != 'r') return false;
    const Number chk = number(h + O_CHKSUM, N_CHKSUM);
    if (!chk.ok || !number(h + O_SIZE, N_SIZE).ok) return false;
    uint32_t sum = 0, high = 0;  // the bytes unsigned; signed, each byte above 127 counts 256 less
    for (uint32_t k = 0; k < BLOCK; k += 4) {
        const uint32_t w = (k >= O_CHKSUM && k < O_CHKSUM + N_CHKSUM) ? 0x20202020u : ld32(h + k);
        sum += (w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24);
        high += (uint32_t)__builtin_popcount(w & 0x80808080u);
    }
    return chk.v == sum || (int64_t)chk.v == (int64_t)sum - 256 * (int64_t)high;
}

// what the walk answers at e where no group starts (e <= len): the end, a cut block, the zero blocks, bytes that are no header
struct Stop {
    int32_t status, zero_blocks;
};
TAR_HD Stop stop_at(const uint8_t *b, uint64_t len, uint64_t e)
{
    if (e == len) return Stop{CHIP_TAR_OK, 0};
    if (len - e < BLOCK) return Stop{CHIP_TAR_TRUNCATED, 0};
    if (!zero_block(b + e)) return Stop{CHIP_TAR_BAD_HEADER, 0};
    return Stop{CHIP_TAR_OK, (len - e >= 2 * BLOCK && zero_block(b + e + BLOCK)) ? 2 : 1};
}

// what the extension headers of a group have set so far
struct Overrides {
    uint64_t name_off, link_off, size;
    uint32_t name_len, link_len;
    uint8_t flags;  // CHIP_TARF_* of what is set
};

TAR_HD bool key_is(const uint8_t *k, uint64_t n, const char *want, uint64_t want_n)
{
    if (n != want_n) return false;
    for (uint64_t i = 0; i < n; i++)
        if (k[i] != (uint8_t)want[i]) return false;
    return true;
}

// the pax records in b[d .. d + s): CHIP_TAR_OK, CHIP_TAR_BAD_HEADER (a malformed record or size value) or CHIP_TAR_UNSUPPORTED (a
// GNU.sparse. key), whichever the first record that is not in order gives
TAR_HD int32_t pax_records(const uint8_t *b, uint64_t d, uint64_t s, Overrides &o)
{
    uint64_t r = 0;
    while (r < s) {
        uint64_t n = 0, k = r;
        while (k < s && k - r < 10 && b[d + k] >= '0' && b[d + k] <= '9') n = n * 10 + (uint64_t)(b[d + k++] - '0');
        if (k == r || k == s || b[d + k] != ' ') return CHIP_TAR_BAD_HEADER;  // no digit, more than ten, or no space behind them
        if (n > s - r || n < k - r + 2 || b[d + r + n - 1] != '\n') return CHIP_TAR_BAD_HEADER;
        const uint64_t key = k + 1, end = r + n - 1;  // key=value lies in [key, end)
        uint64_t eq = key;
        while (eq < end && b[d + eq] != '=') eq++;
        if (eq == end) return CHIP_TAR_BAD_HEADER;
        const uint8_t *kp = b + d + key;
        const uint64_t kn = eq - key, v = eq + 1, vn = end - v;
        if (kn >= 11 && key_is(kp, 11, "GNU.sparse.", 11)) return CHIP_TAR_UNSUPPORTED;
        if (key_is(kp, kn, "path", 4)) {
            o.name_off = d + v, o.name_len = (uint32_t)vn;
            o.flags = (uint8_t)((o.flags & ~CHIP_TARF_NAME_GNU) | CHIP_TARF_NAME_PAX);
        } else if (key_is(kp, kn, "linkpath", 8)) {
            o.link_off = d + v, o.link_len = (uint32_t)vn;
            o.flags = (uint8_t)((o.flags & ~CHIP_TARF_LINK_GNU) | CHIP_TARF_LINK_PAX);
        } else if (key_is(kp, kn, "size", 4)) {
            if (vn < 1 || vn > 19) return CHIP_TAR_BAD_HEADER;
            uint64_t size = 0;
            for (uint64_t i = 0; i < vn; i++) {
                const uint8_t c = b[d + v + i];
                if (c < '0' || c > '9') return CHIP_TAR_BAD_HEADER;
                size = size * 10 + (uint64_t)(c - '0');
            }
            o.size = size;
            o.flags |= CHIP_TARF_SIZE_PAX;
        }
        r += n;
    }
    return CHIP_TAR_OK;
}

// one group
struct Group {
    uint64_t end;      // verdict CHIP_TAR_OK: the position behind the group
    uint64_t bad_off;  // else: the offending header
    int32_t verdict;   // CHIP_TAR_OK a whole group, else what the walk stops with at e
    uint32_t kind;     // KIND_MEMBER (ent is its record) or KIND_GLOBAL
    chip_tar_entry ent;
};

// the group that starts at e, where is_header(b, len, e) holds
TAR_HD void read_group(const uint8_t *b, uint64_t len, uint64_t e, Group &g)
{
    Overrides o{0, 0, 0, 0, 0, 0};
    uint64_t q = e;
    uint32_t n_ext = 0;
    g.end = 0, g.bad_off = e, g.verdict = CHIP_TAR_OK, g.kind = KIND_MEMBER;
    g.ent = chip_tar_entry{};
    auto stop = [&](int32_t verdict, uint64_t bad) { g.verdict = verdict, g.bad_off = bad; };
    for (;;) {
        const uint8_t *h = b + q;
        const uint8_t type = h[O_TYPE];
        const Number size = number(h + O_SIZE, N_SIZE);  // (valid: is_header(q))
        if (type == 'L' || type == 'K' || type == 'x') {
            const uint64_t s = size.v;
            if (++n_ext > CHIP_TAR_EXT_MAX || s > CHIP_TAR_EXT_BYTES) return stop(CHIP_TAR_UNSUPPORTED, q);
            const uint64_t d = q + BLOCK, q2 = d + roundup512(s);
            if (q2 > len || len - q2 < BLOCK) return stop(CHIP_TAR_TRUNCATED, q);
            if (!is_header(b, len, q2)) return stop(CHIP_TAR_BAD_HEADER, q2);
            if (type == 'L') {
                o.name_off = d, o.name_len = (uint32_t)str_len(b + d, s);
                o.flags = (uint8_t)((o.flags & ~CHIP_TARF_NAME_PAX) | CHIP_TARF_NAME_GNU);
            } else if (type == 'K') {
                o.link_off = d, o.link_len = (uint32_t)str_len(b + d, s);
                o.flags = (uint8_t)((o.flags & ~CHIP_TARF_LINK_PAX) | CHIP_TARF_LINK_GNU);
            } else {
                const int32_t v = pax_records(b, d, s, o);
                if (v != CHIP_TAR_OK) return stop(v, q);
            }
            q = q2;
            continue;
        }
        if (type == 'g') {
            if (q != e) return stop(CHIP_TAR_BAD_HEADER, q);
            if (size.v > len) return stop(CHIP_TAR_TRUNCATED, q);
            g.end = q + BLOCK + roundup512(size.v);
            if (g.end > len) return stop(CHIP_TAR_TRUNCATED, q);
            g.kind = KIND_GLOBAL;
            return;
        }
        if (type == 'S' || type == 'M') return stop(CHIP_TAR_UNSUPPORTED, q);
        chip_tar_entry &t = g.ent;
        t.flags = o.flags;
        if (!(o.flags & CHIP_TARF_SIZE_PAX) && size.base256) t.flags |= CHIP_TARF_SIZE_BASE256;
        t.size = (type >= '1' && type <= '6') ? 0 : (o.flags & CHIP_TARF_SIZE_PAX) ? o.size : size.v;
        t.group_off = e, t.header_off = q, t.data_off = q + BLOCK;
        if (t.size > len) return stop(CHIP_TAR_TRUNCATED, q);
        g.end = t.data_off + roundup512(t.size);
        if (g.end > len) return stop(CHIP_TAR_TRUNCATED, q);
        if (o.flags & (CHIP_TARF_NAME_GNU | CHIP_TARF_NAME_PAX)) {
            t.name_off = o.name_off, t.name_len = o.name_len, t.prefix_len = 0;
        } else {
            t.name_off = q + O_NAME, t.name_len = (uint32_t)str_len(h + O_NAME, N_NAME);
            t.prefix_len = (uint16_t)str_len(h + O_PREFIX, N_PREFIX);
        }
        if (o.flags & (CHIP_TARF_LINK_GNU | CHIP_TARF_LINK_PAX)) t.link_off = o.link_off, t.link_len = o.link_len;
        else t.link_off = q + O_LINK, t.link_len = (uint32_t)str_len(h + O_LINK, N_LINK);
        const Number mtime = number(h + O_MTIME, N_MTIME), mode = number(h + O_MODE, N_MODE);
        t.mtime = mtime.ok ? (int64_t)mtime.v : 0;
        t.mode = mode.ok ? (uint32_t)mode.v : 0;
        t.typeflag = type;
        return;
    }
}

// the whole walk, serial.  entries may be null with max_entries == 0.
inline void plan_host(const uint8_t *b, uint64_t len, uint64_t max_entries, chip_tar_entry *entries, chip_tar_plan_summary *s)
{
    *s = chip_tar_plan_summary{0, 0, 0, 0, 0, CHIP_TAR_OK, 0};
    uint64_t e = 0;
    for (;;) {
        s->stop_off = s->bad_off = e;
        if (!is_header(b, len, e)) {
            const Stop st = stop_at(b, len, e);
            s->status = st.status, s->zero_blocks = st.zero_blocks;
            return;
        }
        Group g;
        read_group(b, len, e, g);
        if (g.verdict != CHIP_TAR_OK) {
            s->status = g.verdict, s->bad_off = g.bad_off;
            return;
        }
        if (g.kind == KIND_GLOBAL) {
            s->n_global++;
        } else {
            if (s->n_entries < max_entries) entries[s->n_entries] = g.ent;
            s->n_entries++, s->total_size += g.ent.size;
        }
        e = g.end;
    }
}

}  // namespace tar

}  // namespace chip
