"""BGZF files built in Python for the plan, decode and encoder tests: bodies from zlib.compressobj(wbits=-15) (level 0: one
hand-written stored block, so that the payload sits at a known offset), hand-written headers and trailers, and the serial walk
of include/compu_hip.h restated -- the expectation of every BGZF test."""
import ctypes as C
import functools
import random
import struct
import zlib

import numpy as np

OK, TRUNCATED, BAD_HEADER = 0, 1, 2
MAGIC, BC = b"\x1f\x8b\x08\x04", b"\x06\x00BC\x02\x00"
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")  # htslib's marker
STORED_AT = 18 + 5  # offset of the payload in a level-0 block


def walk(d, max_blocks=None):
    """The plan of `d` by definition: (rows of (in_off, in_len, out_off, out_cap) cut to max_blocks,
    (n_blocks, total_out, in_used, status, eof))."""
    p, total, rows, status = 0, 0, [], OK
    while p != len(d) and status == OK:
        h = d[p:p + 18]
        bs = int.from_bytes(h[16:18], "little") + 1
        if len(d) - p < 18:
            status = TRUNCATED
        elif h[:4] != MAGIC or h[10:16] != BC or bs < 28:
            status = BAD_HEADER
        elif p + bs > len(d):
            status = TRUNCATED
        elif int.from_bytes(d[p + bs - 4:p + bs], "little") > 65536:
            status = BAD_HEADER
        else:
            isize = int.from_bytes(d[p + bs - 4:p + bs], "little")
            rows.append((p, bs, total, isize))
            total, p = total + isize, p + bs
    eof = int(bool(rows) and rows[-1][3] == 0)
    return rows[:len(rows) if max_blocks is None else max_blocks], (len(rows), total, p, status, eof)


def header(bsize, mtime=0, xfl=0, os_=0xFF):
    return MAGIC + struct.pack("<IBB", mtime, xfl, os_) + BC + struct.pack("<H", bsize)


def body(payload, level):
    if level == 0:  # one stored block, final
        assert len(payload) <= 65535
        return b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(payload) + c.flush()


def block(payload, level=6, **hdr):
    b = body(payload, level)
    size = 18 + len(b) + 8
    assert size <= 65536
    return header(size - 1, **hdr) + b + struct.pack("<II", zlib.crc32(payload), len(payload))


def bgzf(payloads, level=6, eof=True):
    return b"".join(block(p, level) for p in payloads) + (EOF if eof else b"")


def _patch(d, at, new):
    return d[:at] + new + d[at + len(new):]


def _text(n, seed):
    r = random.Random(seed)
    return bytes(r.choice(b"ACGTN\n") for _ in range(n))


@functools.lru_cache(maxsize=None)
def fault_files():
    """(name, bytes) of every file of the CPU list; each fault once in block 0 and once in a later block."""
    pay = [_text(300, 1), _text(1, 2), b"", _text(2000, 3)]
    three = [block(p) for p in pay[:3]]
    out = [("empty", b""), ("eof_only", EOF), ("three_eof", b"".join(three) + EOF), ("no_eof", three[0] + three[2] + three[1]),
           ("five_eof", bgzf(pay + [_text(40, 4)]))]
    victim = block(pay[3], mtime=0x01020304, xfl=2, os_=3)  # MTIME, XFL and OS may hold anything
    out.append(("any_mtime_xfl_os", victim + EOF))
    long_extra = MAGIC + victim[4:10] + b"\x08\x00BC\x02\x00" + struct.pack("<H", len(victim) + 2 - 1) + b"XY" + victim[18:]
    faults = {
        "cut_in_block": victim[:len(victim) - 5],
        "cut_after_header": victim[:18],
        "wrong_magic": _patch(victim, 1, b"\x8c"),
        "not_deflate": _patch(victim, 2, b"\x07"),
        "no_fextra": _patch(victim, 3, b"\x00"),
        "xlen_8_second_subfield": long_extra,
        "wrong_subfield_id": _patch(victim, 12, b"BD"),
        "wrong_slen": _patch(victim, 14, b"\x04"),
        "bsize_27": _patch(victim, 16, struct.pack("<H", 26)),
        "bsize_past_end": _patch(victim, 16, struct.pack("<H", 0xFFFF)),
        "isize_65537": _patch(victim, len(victim) - 4, struct.pack("<I", 65537)),
    }
    for k in range(1, 18):
        faults[f"cut_in_header_{k}"] = victim[:k]
    for name, f in faults.items():
        tail = b"" if name.startswith("cut") or name == "bsize_past_end" else EOF
        out.append((name + "@0", f + tail))
        out.append((name + "@3", b"".join(three) + f + tail))
    assert walk(dict(out)["isize_65537@3"])[1][3] == BAD_HEADER and walk(dict(out)["three_eof"])[1] == (4, 301, len(b"".join(three)) + 28, OK, 1)
    return out


def _decoy_block(parts):
    """A level-0 block whose payload is the concatenation of `parts`; returns (block, [offset of each part in the block])."""
    offs, at = [], STORED_AT
    for p in parts:
        offs.append(at)
        at += len(p)
    return block(b"".join(parts), level=0), offs


@functools.lru_cache(maxsize=None)
def decoy_files():
    """Files whose stored bodies hold complete BGZF headers (GPU test 2): name -> bytes."""
    fill, z4 = _text(120, 7), b"\x00" * 4  # z4 in front of a decoy: a small ISIZE for whatever block ends there
    real1, real2 = block(_text(500, 8)), block(_text(90, 9))
    out = {}
    # (a) a chain of three decoys, each leading to the next, the last one ending exactly at the end of the file
    def chain_a(b1, b2, b3):
        parts = [fill, z4, header(b1, mtime=1), fill, z4, header(b2, mtime=2), fill[:50], z4, header(b3, mtime=3), fill]
        return _decoy_block(parts)
    _, o = chain_a(0, 0, 0)
    total = len(chain_a(0, 0, 0)[0]) + len(real1) + len(EOF)
    host, _ = chain_a(o[5] - o[2] - 1, o[8] - o[5] - 1, total - o[8] - 1)
    out["a_chain_to_end"] = host + real1 + EOF
    assert o[5] - o[2] >= 28 and o[8] - o[5] >= 28
    # (b) a decoy that leads exactly to the start of a true block (that block has two predecessors)
    host, o = _decoy_block([fill, header(0, mtime=4), fill])
    host, _ = _decoy_block([fill, header(len(host) - o[1] - 1, mtime=4), fill])
    out["b_joins_true_block"] = real2 + host + real1 + EOF
    # (c) a decoy whose block would run past the end of the file
    host, _ = _decoy_block([fill, header(0xFFFF, mtime=5), fill])
    out["c_past_end"] = host + real1 + EOF
    # (d) two candidates 6 bytes apart: the second header starts in the MTIME field of the first, whose BSIZE field is the
    # second one's XLEN (so the first is a block of 7 bytes: a bad header); the second leads to the next true block
    def overlap(b2):
        first = MAGIC + b"\x00\x00" + MAGIC[:2] + MAGIC[2:] + BC  # 0..3 magic, 6..9 magic again, 10..15 XLEN + BC
        return _decoy_block([fill, first + BC + struct.pack("<H", b2), fill])
    host, o = overlap(0)
    host, _ = overlap(len(host) - (o[1] + 6) - 1)
    out["d_overlap_6"] = host + real1 + EOF
    out["d_overlap_6_at_0"] = host[o[1]:] + real1 + EOF  # the same bytes where the walk meets them: a bad header at once
    return out


@functools.lru_cache(maxsize=None)
def deep_file():
    """5000 blocks of 0..40 payload bytes (GPU test 3): (file, concatenated payloads); the length is no multiple of 4."""
    r = random.Random(20240)
    pay = [bytes(r.randrange(256) for _ in range(r.choice((0, 0, r.randrange(41))))) for _ in range(5000)]
    data = bgzf(pay)
    while len(data) % 4 == 0:
        pay[-1] += b"x"
        data = bgzf(pay)
    return data, b"".join(pay)


@functools.lru_cache(maxsize=None)
def large_file():
    """40 stored blocks of 65 280 random bytes, 65 311 bytes each (GPU test 4): (file, payload)."""
    r = random.Random(5)
    pay = [r.randbytes(65280) for _ in range(40)]
    return bgzf(pay, level=0), b"".join(pay)


def _lead(size, seed):
    """One block of exactly `size` bytes: the header behind it sits at `size`.  A stored block (31 bytes and up: header 18,
    stored-block header 5, trailer 8); the two shorter ones, which no stored block reaches, are zlib's fixed-Huffman bodies of 1
    and 2 payload bytes."""
    b = block(_text(size - 31, seed), level=0) if size >= 31 else block(b"AC"[:size - 28], level=6)
    assert len(b) == size
    return b


@functools.lru_cache(maxsize=None)
def geometry_files():
    """name -> bytes: headers that straddle the tile (16 KiB) and chunk (16 bytes) boundaries of the candidate search, lengths
    that are no multiple of 4, and a file of more than 1 024 tiles.  Block 0 places the header of block 1; every file is a whole
    BGZF file with the EOF block."""
    out, second = {}, block(_text(300, 21))
    for k in (1, 2, 3):  # the magic straddles the tile boundary
        out[f"tile_magic_straddle_{k}"] = _lead(16384 - k, 30 + k) + second + EOF
    for k in (16, 17):  # BSIZE (header bytes 16, 17) is the first two bytes of the next tile / straddles the boundary
        out[f"tile_bsize_straddle_{k}"] = _lead(16384 - k, 30 + k) + second + EOF
    for k in (1, 2, 3):  # the magic straddles a chunk boundary
        out[f"chunk_magic_straddle_{k}"] = _lead(32 - k, 50 + k) + second + EOF
    for r in (1, 2, 3):
        d = _lead(31 + (r - len(second) - 31 - len(EOF)) % 4 + 40, 60 + r) + second + EOF
        assert len(d) % 4 == r
        out[f"len_mod_4_is_{r}"] = d
    # more than 1 024 tiles (16 MiB): headers on both sides of tile 1 024, whose scan partial of the tile counts is not 0
    rnd = random.Random(1024)
    big = b"".join(block(rnd.randbytes(65280), level=0) for _ in range(260)) + second + EOF
    assert len(big) > 1024 * 16384 + 65536 + 28
    out["past_1024_tiles"] = big
    for name, d in out.items():
        rows, summ = walk(d)
        assert summ[2:] == (len(d), OK, 1) and len(rows) == (262 if name == "past_1024_tiles" else 3), name
    return out


def plan_files():
    """(name, bytes) of every file the host plan is held against the walk on, and the GPU plan against the host plan"""
    return fault_files() + sorted(geometry_files().items())


def cut(data, size=65280):
    return [data[i:i + size] for i in range(0, len(data), size)]


# ---- calling the library into poisoned arrays ------------------------------------------------------

POISON64, POISON32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def host_plan(lib, data, max_blocks, room):
    """chip_bgzf_plan_host into poisoned arrays of `room` entries: (rows written, summary tuple, arrays)."""
    from compu_amd.api import _BgzfSummary

    buf = np.frombuffer(data, np.uint8)
    arrs = [np.full(room, POISON64, np.uint64), np.full(room, POISON32, np.uint32), np.full(room, POISON64, np.uint64), np.full(room, POISON32, np.uint32)]
    s = _BgzfSummary(7, 7, 7, 7, 7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.chip_bgzf_plan_host(ptr(buf) if len(data) else None, len(data), max_blocks, *[ptr(a) if max_blocks else None for a in arrs], C.byref(s))
    assert rc == 0
    return check_arrays(arrs, s, max_blocks)


def check_arrays(arrs, s, max_blocks):
    """Nothing behind min(n_blocks, max_blocks) is written; returns (rows, summary tuple)."""
    k = min(int(s.n_blocks), max_blocks)
    assert k <= len(arrs[0])
    for a, poison in zip(arrs, (POISON64, POISON32, POISON64, POISON32)):
        assert (a[k:] == poison).all(), "entries behind min(n_blocks, max_blocks) were written"
    rows = [tuple(int(a[i]) for a in arrs) for i in range(k)]
    return rows, (int(s.n_blocks), int(s.total_out), int(s.in_used), int(s.status), int(s.eof))
