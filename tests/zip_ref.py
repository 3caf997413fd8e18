"""The directory walk of include/compu_hip.h ("ZIP archives"), restated in Python: plan(data) -> (rows, summary) with the tuples
that the tests compare with chip_zip_plan_host and chip_zip_plan.
  row      (header_off, data_off, comp_size, size, name_off, crc32, name_len, method, flags, pad, status)
  summary  (n_entries, n_ok, total_size, cd_off, cd_size, eocd_off, bad_index, status, zip64)"""
import struct

OK, NO_EOCD, BAD_DIRECTORY, UNSUPPORTED = 0, 1, 2, 3
ENT_OK, ENT_UNSUPPORTED, ENT_ENCRYPTED, ENT_BAD_LOCAL, ENT_TOO_LARGE, ENT_BAD_SIZE, ENT_BAD_CRC, ENT_BAD_INDEX = 0, 16, 17, 18, 19, 20, 21, 22
UNIT_IN_MAX, UNIT_OUT_MAX = (1 << 29) - 64, (1 << 32) - 2
M32 = 0xFFFFFFFF


def u16(d, p):
    return struct.unpack_from("<H", d, p)[0]


def u32(d, p):
    return struct.unpack_from("<I", d, p)[0]


def u64(d, p):
    return struct.unpack_from("<Q", d, p)[0]


def find_end(d):
    n = len(d)
    if n < 22:
        return None
    for p in range(n - 22, max(0, n - 22 - 65535) - 1, -1):
        if d[p:p + 4] == b"PK\x05\x06" and p + 22 + u16(d, p + 20) == n:
            return p
    return None


def plan(data, max_entries=None):
    d = bytes(data)
    p = find_end(d)
    if p is None:
        return [], (0, 0, 0, 0, 0, 0, 0, NO_EOCD, 0)
    zip64, limit = 0, p
    spanned = u16(d, p + 4) != 0 or u16(d, p + 6) != 0 or u16(d, p + 8) != u16(d, p + 10)
    if p >= 20 and d[p - 20:p - 16] == b"PK\x06\x07":
        e = u64(d, p - 12)
        if e + 56 > p - 20 or d[e:e + 4] != b"PK\x06\x06":
            return [], (0, 0, 0, 0, 0, p, 0, BAD_DIRECTORY, 0)
        zip64, limit = 1, e
        n, cd_size, cd_off = u64(d, e + 32), u64(d, e + 40), u64(d, e + 48)
        spanned = spanned or u32(d, p - 16) != 0 or u32(d, p - 4) != 1 or u32(d, e + 16) != 0 or u32(d, e + 20) != 0 or u64(d, e + 24) != n
    else:
        n, cd_size, cd_off = u16(d, p + 10), u32(d, p + 12), u32(d, p + 16)

    def summary(n_entries, n_ok, total, bad_index, status):
        return (n_entries, n_ok, total % (1 << 64), cd_off, cd_size, p, bad_index, status, zip64)

    if spanned:
        return [], summary(0, 0, 0, 0, UNSUPPORTED)
    if cd_off + cd_size > limit or n > M32:
        return [], summary(0, 0, 0, 0, BAD_DIRECTORY)
    cd_end = cd_off + cd_size
    rows, n_ok, total, q = [], 0, 0, cd_off
    for i in range(n):
        stop = ([r for r in rows[:max_entries]] if max_entries is not None else rows), summary(i, n_ok, total, i, BAD_DIRECTORY)
        if q + 46 > cd_end or d[q:q + 4] != b"PK\x01\x02":
            return stop
        flags, method, crc, csize, usize = u16(d, q + 8), u16(d, q + 10), u32(d, q + 16), u32(d, q + 20), u32(d, q + 24)
        nlen, xlen, clen, disk, lho = u16(d, q + 28), u16(d, q + 30), u16(d, q + 32), u16(d, q + 34), u32(d, q + 42)
        if q + 46 + nlen + xlen + clen > cd_end:
            return stop
        need = [k for k, v in (("usize", usize), ("csize", csize), ("lho", lho)) if v == M32]
        x, at, has64 = q + 46 + nlen, 0, False
        got = {}
        while xlen - at >= 4:
            ident, size = u16(d, x + at), u16(d, x + at + 2)
            if ident == 1:
                has64 = True
                body = d[x + at + 4:x + at + 4 + min(size, xlen - at - 4)]
                for j, k in enumerate(need):
                    if 8 * j + 8 <= len(body):
                        got[k] = u64(body, 8 * j)
                break
            at += 4 + size  # (behind the extra field: the loop ends)
        if any(k not in got for k in need):
            return stop
        usize, csize, lho = got.get("usize", usize), got.get("csize", csize), got.get("lho", lho)
        data_off = 0
        if lho + 30 <= cd_off and d[lho:lho + 4] == b"PK\x03\x04":
            at = lho + 30 + u16(d, lho + 26) + u16(d, lho + 28)
            if at + csize <= cd_off and (method != 0 or csize == usize):
                data_off = at
        local_ok = data_off != 0  # (a data offset is at least 30)
        if (disk != 0 and not (disk == 0xFFFF and has64)) or method not in (0, 8):
            status = ENT_UNSUPPORTED
        elif flags & ((1 << 0) | (1 << 6) | (1 << 13)):
            status = ENT_ENCRYPTED
        elif not local_ok:
            status = ENT_BAD_LOCAL
        elif method == 8 and (csize > UNIT_IN_MAX or usize > UNIT_OUT_MAX):
            status = ENT_TOO_LARGE
        else:
            status = ENT_OK
        rows.append((lho, data_off, csize, usize, q + 46, crc, nlen, method, flags, 0, status))
        if status == ENT_OK:
            n_ok, total = n_ok + 1, total + usize
        q += 46 + nlen + xlen + clen
    return (rows if max_entries is None else rows[:max_entries]), summary(n, n_ok, total, 0, OK)
