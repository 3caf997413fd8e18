// Writing a ZIP archive as include/compu_hip.h defines it ("ZIP archives: writing"): the check of one source
// record, the stored-or-deflated choice, the lengths of the records, the bytes of every generated record, and the whole assembly
// on the host (chip_zip_assemble_host).  Plain C++ without a device call, so that a stand-alone program can run it under the
// sanitizers (tests/cpp/test_zip_write.cpp); zip_write.hip compiles everything but the host assembly for the device as well
// (ZIP_HD), so host and device lay out and format a record with the same code.  A formatter hands its bytes one by one to a
// `put(k, byte)` of the caller: k counts from the record's first byte, and each k is handed over exactly once.
#pragma once
#include <stdint.h>
#include <string.h>

#include "zip_plan_core.h"

namespace chip {

namespace zipw {

constexpr uint64_t M32 = 0xFFFFFFFFull;
constexpr uint32_t LOCAL_X64 = 20;                   // the local header's id-1 subfield: both sizes
constexpr uint64_t END_ALL = zip::END64_BYTES + zip::LOC64_BYTES + zip::END_BYTES;  // 98
constexpr uint32_t FLAGS_KNOWN = CHIP_ZW_ZIP64 | CHIP_ZW_UTF8;
constexpr uint64_t N_MAX = 0x7fffffffull;

// chip_encode_bound(CHIP_FMT_DEFLATE, n), restated for the device (zip_write.hip compares the two once per process)
ZIP_HD uint64_t deflate_bound(uint64_t n) { return n + 5 * (n ? (n + 65534) / 65535 : 1) + 6 * (n / 65472 + 1) + 5; }

// the arguments alone say whether the archive's length stays below 2^63: every local part is at most content_len + 65 585 bytes
// and every central record at most 65 609
ZIP_HD bool fits_63_bits(uint64_t n, uint64_t content_len)
{
    if (content_len >= ((uint64_t)1 << 62)) return false;
    const uint64_t per = content_len + 2 * 65535 + 30 + 20 + 46 + 28;
    return n == 0 || per <= (((uint64_t)1 << 63) - END_ALL) / n;
}

ZIP_HD uint64_t write_bound(uint64_t n, uint64_t names_total, uint64_t content_total)
{
    // content_total + 2 * names_total + 124 * n + 98 without wrapping, else 0
    if (names_total > (~(uint64_t)0) / 2 || n > (~(uint64_t)0) / 124) return 0;
    uint64_t r = content_total;
    const uint64_t add[3] = {2 * names_total, 124 * n, END_ALL};
    for (uint32_t k = 0; k < 3; k++) {
        if (r > ~(uint64_t)0 - add[k]) return 0;
        r += add[k];
    }
    return r;
}

// what the check keeps of one source record: later passes never read the caller's record again
struct Kept {
    uint64_t size, c;      // the content's length, the length of the data as written
    uint64_t name_off;     // in `names`
    uint64_t data_src;     // in `content` (stored) or in `comp` (deflated)
    uint32_t crc;
    uint16_t name_len, method, dos_time, dos_date;  // method: as written
    uint32_t zs;           // the sizes go into id-1 subfields
};

// a record the rules refuse (CHIP_ZIPW_BAD_SOURCE); have_comp: the three comp arrays are given
ZIP_HD bool source_bad(const chip_zip_source &s, uint64_t names_len, uint64_t content_len)
{
    return (s.method != CHIP_ZIP_STORE && s.method != CHIP_ZIP_DEFLATE) || s.data_off > content_len || s.size > content_len - s.data_off ||
           s.name_off > names_len || s.name_len > names_len - s.name_off;
}
ZIP_HD bool writes_deflated(const chip_zip_source &s, bool have_comp, uint32_t comp_len)
{
    return s.method == CHIP_ZIP_DEFLATE && have_comp && comp_len > 0 && comp_len < s.size;
}
ZIP_HD bool stream_bad(uint64_t comp_off, uint32_t comp_len, uint64_t comp_all) { return comp_off > comp_all || comp_len > comp_all - comp_off; }

// The check and the choice of entry i: false = a bad record.  comp_off / comp_len are entry i's (0 without the arrays).
ZIP_HD bool keep(const chip_zip_source &s, uint64_t names_len, uint64_t content_len, bool have_comp, uint64_t comp_off, uint32_t comp_len,
                 uint64_t comp_all, uint32_t crc, uint32_t flags, Kept &k)
{
    if (source_bad(s, names_len, content_len)) return false;
    const bool defl = writes_deflated(s, have_comp, comp_len);
    if (defl && stream_bad(comp_off, comp_len, comp_all)) return false;
    k.size = s.size, k.c = defl ? comp_len : s.size;
    k.name_off = s.name_off, k.data_src = defl ? comp_off : s.data_off;
    k.crc = crc, k.name_len = s.name_len, k.method = defl ? CHIP_ZIP_DEFLATE : CHIP_ZIP_STORE, k.dos_time = s.dos_time, k.dos_date = s.dos_date;
    k.zs = ((flags & CHIP_ZW_ZIP64) || k.size >= M32 || k.c >= M32) ? 1u : 0u;
    return true;
}

ZIP_HD uint32_t local_extra(const Kept &k) { return k.zs ? LOCAL_X64 : 0u; }
ZIP_HD uint64_t local_len(const Kept &k) { return zip::LOCAL_BYTES + k.name_len + local_extra(k) + k.c; }  // header, name, extra, data
ZIP_HD bool lho_in_extra(uint64_t header_off, uint32_t flags) { return (flags & CHIP_ZW_ZIP64) || header_off >= M32; }
ZIP_HD uint32_t central_extra(const Kept &k, bool zl) { return (k.zs || zl) ? 4u + (k.zs ? 16u : 0u) + (zl ? 8u : 0u) : 0u; }
ZIP_HD uint64_t central_len(const Kept &k, bool zl) { return zip::CENTRAL_BYTES + k.name_len + central_extra(k, zl); }
ZIP_HD uint16_t version_of(const Kept &k, bool zl) { return (k.zs || zl) ? 45 : k.method == CHIP_ZIP_DEFLATE ? 20 : 10; }
ZIP_HD uint16_t gp_flags(uint32_t flags) { return (flags & CHIP_ZW_UTF8) ? 0x0800 : 0; }

// the end of the archive: z, and the bytes behind the directory
ZIP_HD bool end_zip64(uint64_t n, uint64_t cd_off, uint64_t cd_size, uint32_t flags)
{
    return (flags & CHIP_ZW_ZIP64) || n >= 0xFFFF || cd_size >= M32 || cd_off >= M32;
}
ZIP_HD uint64_t end_len(bool z) { return z ? END_ALL : zip::END_BYTES; }

template <class Put>
ZIP_HD void put16(Put &put, uint32_t k, uint32_t v)
{
    put(k, (uint8_t)v), put(k + 1, (uint8_t)(v >> 8));
}
template <class Put>
ZIP_HD void put32(Put &put, uint32_t k, uint32_t v)
{
    put16(put, k, v & 0xFFFFu), put16(put, k + 2, v >> 16);
}
template <class Put>
ZIP_HD void put64(Put &put, uint32_t k, uint64_t v)
{
    put32(put, k, (uint32_t)v), put32(put, k + 4, (uint32_t)(v >> 32));
}

// the seven fields the local header and the central record share (gp flags .. usize), 22 bytes from k
template <class Put>
ZIP_HD void put_shared(Put &put, uint32_t k, const Kept &e, uint32_t flags)
{
    put16(put, k, gp_flags(flags)), put16(put, k + 2, e.method), put16(put, k + 4, e.dos_time), put16(put, k + 6, e.dos_date);
    put32(put, k + 8, e.crc);
    put32(put, k + 12, e.zs ? (uint32_t)M32 : (uint32_t)e.c), put32(put, k + 16, e.zs ? (uint32_t)M32 : (uint32_t)e.size);
}

// the 30 bytes of a local header
template <class Put>
ZIP_HD void format_local(Put &put, const Kept &e, bool zl, uint32_t flags)
{
    put32(put, 0, zip::SIG_LOCAL), put16(put, 4, version_of(e, zl));
    put_shared(put, 6, e, flags);
    put16(put, 26, e.name_len), put16(put, 28, local_extra(e));
}
// its extra field behind the name: LOCAL_X64 bytes, only with e.zs
template <class Put>
ZIP_HD void format_local_extra(Put &put, const Kept &e)
{
    put16(put, 0, 1), put16(put, 2, 16), put64(put, 4, e.size), put64(put, 12, e.c);
}
// the 46 bytes of a central record
template <class Put>
ZIP_HD void format_central(Put &put, const Kept &e, uint64_t header_off, bool zl, uint32_t flags)
{
    const uint32_t v = version_of(e, zl);
    put32(put, 0, zip::SIG_CENTRAL), put16(put, 4, v), put16(put, 6, v);
    put_shared(put, 8, e, flags);
    put16(put, 28, e.name_len), put16(put, 30, central_extra(e, zl)), put16(put, 32, 0), put16(put, 34, 0), put16(put, 36, 0), put32(put, 38, 0);
    put32(put, 42, zl ? (uint32_t)M32 : (uint32_t)header_off);
}
// its extra field behind the name: central_extra(e, zl) bytes
template <class Put>
ZIP_HD void format_central_extra(Put &put, const Kept &e, uint64_t header_off, bool zl)
{
    if (!e.zs && !zl) return;
    put16(put, 0, 1), put16(put, 2, central_extra(e, zl) - 4u);
    uint32_t k = 4;
    if (e.zs) put64(put, 4, e.size), put64(put, 12, e.c), k = 20;
    if (zl) put64(put, k, header_off);
}
// the end records, end_len(z) bytes; at = where they start (the directory's end)
template <class Put>
ZIP_HD void format_end(Put &put, uint64_t n, uint64_t cd_off, uint64_t cd_size, bool z)
{
    uint32_t k = 0;
    if (z) {
        put32(put, 0, zip::SIG_END64), put64(put, 4, 44), put16(put, 12, 45), put16(put, 14, 45), put32(put, 16, 0), put32(put, 20, 0);
        put64(put, 24, n), put64(put, 32, n), put64(put, 40, cd_size), put64(put, 48, cd_off);
        put32(put, 56, zip::SIG_LOC64), put32(put, 60, 0), put64(put, 64, cd_off + cd_size), put32(put, 72, 1);
        k = (uint32_t)(zip::END64_BYTES + zip::LOC64_BYTES);
    }
    const uint32_t n16 = n < 0xFFFF ? (uint32_t)n : 0xFFFFu;
    put32(put, k, zip::SIG_END), put16(put, k + 4, 0), put16(put, k + 6, 0), put16(put, k + 8, n16), put16(put, k + 10, n16);
    put32(put, k + 12, cd_size < M32 ? (uint32_t)cd_size : (uint32_t)M32), put32(put, k + 16, cd_off < M32 ? (uint32_t)cd_off : (uint32_t)M32);
    put16(put, k + 20, 0);
}

// entries[i]: what chip_zip_plan makes of entry i of the written archive
ZIP_HD chip_zip_entry entry_of(const Kept &e, uint64_t header_off, uint64_t record_off, uint32_t flags)
{
    chip_zip_entry r{};
    r.header_off = header_off, r.data_off = header_off + zip::LOCAL_BYTES + e.name_len + local_extra(e);
    r.comp_size = e.c, r.size = e.size, r.name_off = record_off + zip::CENTRAL_BYTES;
    r.crc32 = e.crc, r.name_len = e.name_len, r.method = e.method, r.flags = gp_flags(flags), r.pad = 0;
    r.status = (e.method == CHIP_ZIP_DEFLATE && (e.c > zip::UNIT_IN_MAX || e.size > zip::UNIT_OUT_MAX)) ? CHIP_ZIPENT_TOO_LARGE : CHIP_ZIPENT_OK;
    return r;
}

struct BytePut {  // the bytes go to p[k]
    uint8_t *p;
    ZIP_HD void operator()(uint32_t k, uint8_t v) const { p[k] = v; }
};

inline chip_zip_write_summary no_archive(uint64_t n, int32_t status, uint64_t bad_index)
{
    return chip_zip_write_summary{n, 0, 0, 0, 0, 0, bad_index, status, 0};
}

// chip_zip_assemble_host behind its argument checks: two passes over the records (the lengths; the records, the entries and the
// bytes), no allocation.
inline void assemble_host(uint64_t n, const chip_zip_source *src, const uint8_t *names, uint64_t names_len, const uint8_t *content,
                          uint64_t content_len, const uint8_t *comp, uint64_t comp_all, const uint64_t *comp_off, const uint32_t *comp_len,
                          const uint32_t *crc, uint32_t flags, uint8_t *out, uint64_t out_cap, chip_zip_entry *entries, chip_zip_write_summary *summary)
{
    const bool have_comp = comp_len != nullptr;
    auto kept = [&](uint64_t i, Kept &k) {
        return keep(src[i], names_len, content_len, have_comp, have_comp ? comp_off[i] : 0, have_comp ? comp_len[i] : 0, comp_all, crc[i], flags, k);
    };
    uint64_t cd_off = 0, cd_size = 0, n_deflated = 0;
    for (uint64_t i = 0; i < n; i++) {
        Kept k;
        if (!kept(i, k)) {
            *summary = no_archive(n, CHIP_ZIPW_BAD_SOURCE, i);
            return;
        }
        cd_size += central_len(k, lho_in_extra(cd_off, flags));
        cd_off += local_len(k);
        n_deflated += k.method == CHIP_ZIP_DEFLATE;
    }
    const bool z = end_zip64(n, cd_off, cd_size, flags);
    chip_zip_write_summary s{n, n_deflated, cd_off + cd_size + end_len(z), cd_off, cd_size, cd_off + cd_size + end_len(z) - zip::END_BYTES, 0, CHIP_ZIPW_OK, z};
    const bool room = s.out_len <= out_cap;
    if (!room) s.status = CHIP_ZIPW_NEED_OUTPUT;
    uint64_t h = 0, r = cd_off;
    for (uint64_t i = 0; i < n && (room || entries); i++) {
        Kept k;
        (void)kept(i, k);
        const bool zl = lho_in_extra(h, flags);
        if (entries) entries[i] = entry_of(k, h, r, flags);
        if (room) {
            BytePut lp{out + h}, lx{out + h + zip::LOCAL_BYTES + k.name_len}, cp{out + r}, cx{out + r + zip::CENTRAL_BYTES + k.name_len};
            format_local(lp, k, zl, flags);
            if (k.zs) format_local_extra(lx, k);
            format_central(cp, k, h, zl, flags);
            format_central_extra(cx, k, h, zl);
            if (k.name_len) {
                memcpy(out + h + zip::LOCAL_BYTES, names + k.name_off, k.name_len);
                memcpy(out + r + zip::CENTRAL_BYTES, names + k.name_off, k.name_len);
            }
            if (k.c) memcpy(out + h + zip::LOCAL_BYTES + k.name_len + local_extra(k), (k.method == CHIP_ZIP_DEFLATE ? comp : content) + k.data_src, k.c);
        }
        h += local_len(k), r += central_len(k, zl);
    }
    if (room) {
        BytePut ep{out + cd_off + cd_size};
        format_end(ep, n, cd_off, cd_size, z);
    }
    *summary = s;
}

}  // namespace zipw

}  // namespace chip
