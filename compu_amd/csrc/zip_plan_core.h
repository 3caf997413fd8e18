// The walk of a ZIP archive's directory as include/compu_hip.h defines it (chip_zip_plan_host): the end
// record, the ZIP64 records, one directory record, the local header of one entry, and the serial walk over them.  Plain C++
// without a device call, so that a stand-alone program can run it under the sanitizers (tests/cpp/test_zip_plan.cpp); zip.hip
// compiles the per-record parts for the device as well (ZIP_HD), so host and device read a record with the same code.  Every read is
// checked against the buffer's length first: b[0 .. len) is all that is ever looked at.
#pragma once
#include <stdint.h>

#include "../../include/compu_hip.h"

#if defined(__HIPCC__)
#define ZIP_HD __host__ __device__ inline
#else
#define ZIP_HD inline
#endif

namespace chip {

namespace zip {

constexpr uint32_t SIG_LOCAL = 0x04034b50u, SIG_CENTRAL = 0x02014b50u, SIG_END = 0x06054b50u, SIG_END64 = 0x06064b50u, SIG_LOC64 = 0x07064b50u;
constexpr uint64_t END_BYTES = 22, COMMENT_MAX = 65535, LOC64_BYTES = 20, END64_BYTES = 56, CENTRAL_BYTES = 46, LOCAL_BYTES = 30;
constexpr uint64_t UNIT_IN_MAX = ((uint64_t)1 << 29) - 64, UNIT_OUT_MAX = 0xFFFFFFFEull;  // the limits of a unit of chip_decode_batch
constexpr uint16_t FLAG_ENCRYPTED = (1u << 0) | (1u << 6) | (1u << 13);

ZIP_HD uint32_t le16(const uint8_t *b, uint64_t p) { return (uint32_t)b[p] | ((uint32_t)b[p + 1] << 8); }
ZIP_HD uint32_t le32(const uint8_t *b, uint64_t p) { return le16(b, p) | (le16(b, p + 2) << 16); }
ZIP_HD uint64_t le64(const uint8_t *b, uint64_t p) { return (uint64_t)le32(b, p) | ((uint64_t)le32(b, p + 4) << 32); }

// does an end record sit at p?  (p + 22 <= len)
ZIP_HD bool end_record_at(const uint8_t *b, uint64_t len, uint64_t p) { return le32(b, p) == SIG_END && p + END_BYTES + le16(b, p + 20) == len; }

// the lowest position the end record may have
ZIP_HD uint64_t end_search_from(uint64_t len) { return len > END_BYTES + COMMENT_MAX ? len - END_BYTES - COMMENT_MAX : 0; }

// what the end record at p (and the ZIP64 records in front of it) says
struct End {
    uint64_t n, cd_off, cd_size, eocd_off;
    int32_t status;  // CHIP_ZIP_OK, CHIP_ZIP_BAD_DIRECTORY, CHIP_ZIP_UNSUPPORTED
    int32_t zip64;
};

ZIP_HD End read_end(const uint8_t *b, uint64_t p)
{
    End r{0, 0, 0, p, CHIP_ZIP_OK, 0};
    uint64_t limit = p;  // the directory ends in front of this
    bool spanned = le16(b, p + 4) != 0 || le16(b, p + 6) != 0 || le16(b, p + 8) != le16(b, p + 10);
    if (p >= LOC64_BYTES && le32(b, p - LOC64_BYTES) == SIG_LOC64) {
        const uint64_t loc = p - LOC64_BYTES, e = le64(b, loc + 8);
        if (e > loc || loc - e < END64_BYTES || le32(b, e) != SIG_END64) {
            r.status = CHIP_ZIP_BAD_DIRECTORY;
            return r;
        }
        r.zip64 = 1;
        r.n = le64(b, e + 32), r.cd_size = le64(b, e + 40), r.cd_off = le64(b, e + 48);
        limit = e;
        spanned = spanned || le32(b, loc + 4) != 0 || le32(b, loc + 16) != 1 || le32(b, e + 16) != 0 || le32(b, e + 20) != 0 || le64(b, e + 24) != r.n;
    } else {
        r.n = le16(b, p + 10), r.cd_size = le32(b, p + 12), r.cd_off = le32(b, p + 16);
    }
    if (spanned) r.status = CHIP_ZIP_UNSUPPORTED;
    else if (r.cd_off > limit || r.cd_size > limit - r.cd_off || r.n > 0xFFFFFFFFull) r.status = CHIP_ZIP_BAD_DIRECTORY;
    return r;
}

// one directory record
struct Record {
    uint64_t csize, usize, lho, rec_len;
    uint32_t crc;
    uint16_t flags, method, nlen, disk;
    bool has64;  // a subfield with id 1 is present
};

// the record at q of the directory [cd_off, cd_end): false where the walk stops
ZIP_HD bool read_record(const uint8_t *b, uint64_t cd_off, uint64_t cd_end, uint64_t q, Record &r)
{
    if (q < cd_off || q > cd_end || cd_end - q < CENTRAL_BYTES || le32(b, q) != SIG_CENTRAL) return false;
    r.flags = (uint16_t)le16(b, q + 8), r.method = (uint16_t)le16(b, q + 10), r.crc = le32(b, q + 16);
    r.csize = le32(b, q + 20), r.usize = le32(b, q + 24);
    r.nlen = (uint16_t)le16(b, q + 28);
    const uint64_t xlen = le16(b, q + 30), clen = le16(b, q + 32);
    r.disk = (uint16_t)le16(b, q + 34), r.lho = le32(b, q + 42);
    r.rec_len = CENTRAL_BYTES + r.nlen + xlen + clen;
    r.has64 = false;
    if (cd_end - q < r.rec_len) return false;
    const bool need_u = r.usize == 0xFFFFFFFFull, need_c = r.csize == 0xFFFFFFFFull, need_l = r.lho == 0xFFFFFFFFull;
    const uint64_t x = q + CENTRAL_BYTES + r.nlen;
    uint64_t at = 0;
    while (xlen - at >= 4) {
        const uint64_t id = le16(b, x + at), size = le16(b, x + at + 2);
        if (id != 1) {
            at += 4 + size;
            if (at > xlen) break;  // (a subfield that reaches out of the extra field ends the chain)
            continue;
        }
        r.has64 = true;
        uint64_t v = x + at + 4, room = xlen - at - 4 < size ? xlen - at - 4 : size;
        if (need_u) {
            if (room < 8) return false;
            r.usize = le64(b, v), v += 8, room -= 8;
        }
        if (need_c) {
            if (room < 8) return false;
            r.csize = le64(b, v), v += 8, room -= 8;
        }
        if (need_l) {
            if (room < 8) return false;
            r.lho = le64(b, v);
        }
        break;
    }
    return r.has64 || !(need_u || need_c || need_l);
}

// entry = the record at q, its local header looked at
ZIP_HD chip_zip_entry make_entry(const uint8_t *b, uint64_t cd_off, uint64_t q, const Record &r)
{
    chip_zip_entry e{};
    e.header_off = r.lho, e.comp_size = r.csize, e.size = r.usize, e.name_off = q + CENTRAL_BYTES;
    e.crc32 = r.crc, e.name_len = r.nlen, e.method = r.method, e.flags = r.flags;
    bool local = r.lho <= cd_off && cd_off - r.lho >= LOCAL_BYTES && le32(b, r.lho) == SIG_LOCAL;
    uint64_t data = 0;
    if (local) {
        data = r.lho + LOCAL_BYTES + le16(b, r.lho + 26) + le16(b, r.lho + 28);
        local = data <= cd_off && r.csize <= cd_off - data && (r.method != 0 || r.csize == r.usize);
    }
    e.data_off = local ? data : 0;
    if ((r.disk != 0 && !(r.disk == 0xFFFF && r.has64)) || (r.method != 0 && r.method != 8)) e.status = CHIP_ZIPENT_UNSUPPORTED;
    else if (r.flags & FLAG_ENCRYPTED) e.status = CHIP_ZIPENT_ENCRYPTED;
    else if (!local) e.status = CHIP_ZIPENT_BAD_LOCAL;
    else if (r.method == 8 && (r.csize > UNIT_IN_MAX || r.usize > UNIT_OUT_MAX)) e.status = CHIP_ZIPENT_TOO_LARGE;
    else e.status = CHIP_ZIPENT_OK;
    return e;
}

// the whole walk, serial.  entries may be null with max_entries == 0.
inline void plan_host(const uint8_t *b, uint64_t len, uint64_t max_entries, chip_zip_entry *entries, chip_zip_plan_summary *s)
{
    *s = chip_zip_plan_summary{0, 0, 0, 0, 0, 0, 0, CHIP_ZIP_NO_EOCD, 0};
    if (len < END_BYTES) return;
    uint64_t p = len - END_BYTES;
    const uint64_t from = end_search_from(len);
    for (;; p--) {
        if (end_record_at(b, len, p)) break;
        if (p == from) return;
    }
    const End end = read_end(b, p);
    s->eocd_off = p, s->cd_off = end.cd_off, s->cd_size = end.cd_size, s->zip64 = end.zip64, s->status = end.status;
    if (end.status != CHIP_ZIP_OK) return;
    const uint64_t cd_end = end.cd_off + end.cd_size;
    uint64_t q = end.cd_off;
    for (uint64_t i = 0; i < end.n; i++) {
        Record r;
        if (!read_record(b, end.cd_off, cd_end, q, r)) {
            s->status = CHIP_ZIP_BAD_DIRECTORY;
            s->bad_index = i;
            return;
        }
        const chip_zip_entry e = make_entry(b, end.cd_off, q, r);
        if (i < max_entries) entries[i] = e;
        s->n_entries = i + 1;
        if (e.status == CHIP_ZIPENT_OK) s->n_ok++, s->total_size += e.size;
        q += r.rec_len;
    }
}

}  // namespace zip

}  // namespace chip
