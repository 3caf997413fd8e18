"""The independent reference of the seek-table tests, pure Python: the walk over a table as include/compu_hip.h defines it
(chip_zstd_seek_plan_host), the table's writer, and XXH64 on Python integers."""
import struct

OK, NO_TABLE, NEED_TAIL, BAD_TABLE, TOO_LARGE, BAD_LAYOUT = range(6)
FOOTER_MAGIC, SKIP_MAGIC, MAX_FRAMES = 0x8F92EAB1, 0x184D2A5E, 0x8000000
M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
XXH64_EMPTY = 0xEF46DB3751D8E999


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _round(acc, lane):
    return _rotl((acc + lane * P2) & M64, 31) * P1 & M64


def xxh64(data, seed=0):
    """XXH64 of `data` (the specification's steps, one after the other)"""
    data, n, p = bytes(data), len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M64, (seed + P2) & M64, seed, (seed - P1) & M64]
        while p + 32 <= n:
            v = [_round(a, lane) for a, lane in zip(v, struct.unpack_from("<4Q", data, p))]
            p += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
        for a in v:
            h = ((h ^ _round(0, a)) * P1 + P4) & M64
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, p)[0]), 27) * P1 + P4) & M64
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, p)[0] * P1 & M64), 23) * P2 + P3) & M64
        p += 4
    while p < n:
        h = _rotl(h ^ (data[p] * P5 & M64), 11) * P1 & M64
        p += 1
    h = ((h ^ (h >> 33)) * P2) & M64
    h = ((h ^ (h >> 29)) * P3) & M64
    return h ^ (h >> 32)


def table(c_len, d_len, checksum=None, desc_low=0):
    """the bytes of a seek table: skippable header, entries, footer"""
    n = len(c_len)
    assert len(d_len) == n and (checksum is None or len(checksum) == n)
    body = b"".join(struct.pack("<II", c, d) + (b"" if checksum is None else struct.pack("<I", x))
                    for c, d, x in zip(c_len, d_len, checksum if checksum is not None else [0] * n))
    foot = struct.pack("<IBI", n, (0x80 if checksum is not None else 0) | desc_low, FOOTER_MAGIC)
    return struct.pack("<II", SKIP_MAGIC, len(body) + len(foot)) + body + foot


def plan(tail, file_len=None, max_frames=None):
    """(rows, summary): rows = the first min(n, max_frames) (in_off, in_len, out_off, out_cap, checksum); summary = (n_frames,
    table_bytes, frames_bytes, total_out, bad_index, status, checksums).  rows is [] unless the status is OK."""
    tail = bytes(tail)
    tl = len(tail)
    file_len = tl if file_len is None else file_len
    le32 = lambda at: struct.unpack_from("<I", tail, at)[0]  # noqa: E731
    if file_len < 17:
        return [], (0, 0, 0, 0, 0, NO_TABLE, 0)
    if tl < 17:
        return [], (0, 17, 0, 0, 0, NEED_TAIL, 0)
    if le32(tl - 4) != FOOTER_MAGIC:
        return [], (0, 0, 0, 0, 0, NO_TABLE, 0)
    desc = tail[tl - 5]
    if desc & 0x7C:
        return [], (0, 0, 0, 0, 0, BAD_TABLE, 0)
    cs = desc >> 7
    es = 8 + 4 * cs
    n = le32(tl - 9)
    if n > MAX_FRAMES:
        return [], (0, 0, 0, 0, 0, BAD_TABLE, 0)
    T = 17 + es * n
    if T > file_len:
        return [], (0, 0, 0, 0, 0, BAD_TABLE, 0)
    if tl < T:
        return [], (n, T, 0, 0, 0, NEED_TAIL, cs)
    if le32(tl - T) != SKIP_MAGIC or le32(tl - T + 4) != T - 8:
        return [], (n, T, 0, 0, 0, BAD_TABLE, cs)
    rows, C, D, bad = [], 0, 0, None
    for i in range(n):
        at = tl - T + 8 + es * i
        c, d = le32(at), le32(at + 4)
        x = le32(at + 8) if cs else 0
        if d == 0xFFFFFFFF and bad is None:
            bad = i
        rows.append((C, c, D, d, x))
        C += c
        D += d
    if bad is not None:
        return [], (n, T, 0, 0, bad, TOO_LARGE, cs)
    if C > file_len - T:
        return [], (n, T, 0, 0, 0, BAD_LAYOUT, cs)
    return rows[: n if max_frames is None else max_frames], (n, T, C, D, 0, OK, cs)
