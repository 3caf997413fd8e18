"""Buffers of gzip members for the member-index tests (chip_gzip_plan): member bodies by Python's zlib, headers and trailers written
by hand.  A case holds the file and its twin: the same bytes with every deliberately wrong CRC-32 repaired, which is what the
size pass sees of the file (it makes every check but the CRC comparison).  The reference plan of a case (gzip_plan_ref.py) is the
walk of include/compu_hip.h over the twin.  Shared by tests/test_gzip_plan_cpu.py and tests/test_gzip_plan_gpu.py."""
import functools
import random
import struct
import zlib
from collections import namedtuple

OK, TRUNCATED, BAD_HEADER, TOO_LARGE, BAD_MEMBER = 0, 1, 2, 3, 4
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
TILE = 16384

# name; the file; its twin; contents: the decoded bytes of every member of the plan, in order, or None where a member is too large
# to hold (the 2^32 cases); bad_crc: indices of the members whose CRC-32 is wrong in the file
Case = namedtuple("Case", "name data twin contents bad_crc")


def text(n, seed=0):
    """n bytes that compress to literals and matches"""
    r = random.Random(seed)
    words = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(2, 9))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + b" "
    return bytes(out[:n])


def noise(n, seed=0):
    return random.Random(seed).randbytes(n)


def deflate(content, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(content) + co.flush()


def header(flg=0, mtime=0, xfl=0, os_=3, extra=None, name=None, comment=None, hcrc_xor=0):
    """the gzip header of RFC 1952 sec. 2.3 with the optional fields the arguments ask for"""
    flg |= (FEXTRA if extra is not None else 0) | (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<IBB", mtime, xfl, os_)
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if flg & FHCRC:
        h += struct.pack("<H", ((zlib.crc32(h) & 0xFFFF) ^ hcrc_xor))
    return h


def trailer(content, crc_xor=0, isize_add=0):
    return struct.pack("<II", (zlib.crc32(content) ^ crc_xor) & 0xFFFFFFFF, (len(content) + isize_add) & 0xFFFFFFFF)


def member(content, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, body=None, **hdr):
    """one whole, valid member"""
    return header(**hdr) + (deflate(content, level, strategy) if body is None else body) + trailer(content)


def padded_to(content, start, want_end, **kw):
    """a valid member of `content` that, starting at `start`, ends exactly at `want_end`: an FNAME field takes up the slack"""
    base = len(member(content, name=b"", **kw))
    slack = want_end - start - base
    assert slack >= 0, (start, want_end, base)
    m = member(content, name=b"n" * slack, **kw)
    assert start + len(m) == want_end
    return m


def far_match_block():
    """a final fixed block: the literal 'a', then a match of length 3 at distance 5 -- in front of the member's first byte"""
    bits = []
    put = lambda v, n: bits.extend((v >> k) & 1 for k in range(n))  # noqa: E731 - fields go in LSB first
    code = lambda v, n: bits.extend((v >> k) & 1 for k in reversed(range(n)))  # noqa: E731 - Huffman codes MSB first
    put(1, 1), put(1, 2)
    code(0x30 + ord("a"), 8), code(257 - 256, 7), code(4, 5), put(0, 1), code(0, 7)
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))


class File:
    """members and other bytes laid end to end, with the twin and the plan's contents kept alongside"""

    def __init__(self):
        self.data, self.twin, self.contents, self.bad_crc = bytearray(), bytearray(), [], set()

    def add(self, content, **kw):
        m = member(content, **kw)
        self.data += m
        self.twin += m
        self.contents.append(content)
        return self

    def add_to(self, content, want_end, **kw):
        m = padded_to(content, len(self.data), want_end, **kw)
        self.data += m
        self.twin += m
        self.contents.append(content)
        return self

    def add_bad_crc(self, content, **kw):
        m = member(content, **kw)
        self.bad_crc.add(len(self.contents))
        self.data += m[:-8] + struct.pack("<I", zlib.crc32(content) ^ 0x5A5A5A5A) + m[-4:]
        self.twin += m
        self.contents.append(content)
        return self

    def raw(self, b):
        """bytes that are no member of the plan: where the walk stops"""
        self.data += b
        self.twin += b
        return self

    def case(self, name):
        return Case(name, bytes(self.data), bytes(self.twin), list(self.contents), frozenset(self.bad_crc))


def good2():
    return File().add(text(700, 1)).add(text(90, 2), level=1)


# ---- member kinds ------------------------------------------------------------------------------

def kind_cases():
    out = []
    empty = member(b"")
    assert len(empty) == 20
    out.append(File().add(b"").case("one_empty_member"))
    out.append(File().add(text(5000, 3)).case("one_member"))
    out.append(File().add(b"").add(b"").add(text(10, 4)).add(b"").case("empty_members_between"))
    f = File()
    f.add(noise(300, 5), level=0).add(text(3000, 6), strategy=zlib.Z_FIXED).add(text(3000, 7))
    f.add(text(70000, 8), level=0)  # two stored blocks
    f.add(text(200_000, 9), level=1).add(text(150_000, 10), level=6).add(text(60_000, 11), level=9).add(noise(40_000, 12), level=6)
    f.add(b"x").add(b"", level=0).add(b"", strategy=zlib.Z_FIXED)
    out.append(f.case("stored_fixed_dynamic_levels"))
    f = File()
    f.add(text(100, 13), extra=b"AB\x03\x00xyz").add(text(100, 14), name=b"file.txt").add(text(100, 15), comment=b"a comment")
    f.add(text(100, 16), flg=FHCRC).add(text(100, 17), flg=FHCRC | FTEXT, extra=b"", name=b"", comment=b"")
    f.add(text(100, 18), flg=FHCRC, extra=b"XY\x04\x00abcd" + b"Z" * 600, name=b"n" * 300, comment=b"c" * 300, mtime=0x12345678, xfl=2, os_=255)
    out.append(f.case("header_fields"))
    return out


# ---- positions -----------------------------------------------------------------------------------

def position_cases():
    out = []
    # member starts at every residue mod 16, in an order that is no progression
    f = File().add(text(40, 20))
    pos = len(f.data)
    for k, r in enumerate([5, 15, 14, 13, 0, 1, 12, 2, 11, 3, 10, 4, 9, 6, 8, 7]):
        end = pos + 80
        end += (r - end) % 16
        f.add_to(text(30 + k, 21 + k), end)
        pos = end
    f.add(text(10, 40))
    out.append(f.case("starts_at_every_residue_mod_16"))
    for by in (1, 2, 3):  # a header straddling a 16-byte chunk boundary, and a 16 KiB tile boundary
        f = File().add_to(text(50, 41), 96 - by).add(text(60, 42))
        out.append(f.case(f"chunk_boundary_straddled_by_{by}"))
        f = File().add_to(noise(15000, 43), TILE - by).add(text(60, 44)).add_to(noise(15000, 45), 2 * TILE - by).add(text(5, 46))
        out.append(f.case(f"tile_boundary_straddled_by_{by}"))
    for want in (1, 2, 3, 0):  # the last member ends exactly at len, whatever len is modulo 4
        f = File().add(text(500, 47))
        end = len(f.data) + 60
        end += (want - end) % 4
        f.add_to(text(33, 48), end)
        assert len(f.data) % 4 == want
        out.append(f.case(f"len_mod_4_is_{want}"))
    return out


# ---- counts ----------------------------------------------------------------------------------------

def count_cases():
    r = random.Random(50)
    f = File()
    for k in range(3000):  # more than a 1024-entry scan workgroup of candidates, 12 jump levels
        c = text(r.randrange(0, 24), 100 + k)
        if k % 500 == 250:
            f.add(c, name=b"\x1f\x8b\x08\x01")  # a few decoys among them
        else:
            f.add(c, level=r.choice((1, 6)), strategy=r.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED)))
    return [f.case("three_thousand_tiny")]


# ---- decoys ----------------------------------------------------------------------------------------

def decoy_cases():
    out = []
    inner = member(text(300, 60))
    inner2 = member(text(40, 61), name=b"in")
    f = good2().add(b"abc\x1f\x8b\x08\x00defgh" + noise(30, 62) + b"\x1f\x8b\x08\x08", level=0).add(text(50, 63))
    out.append(f.case("magic_in_stored_payload"))
    f = good2().add(b"ab" + inner + inner2 + b"tail", level=0).add(text(50, 64))  # a chain of two decoys
    out.append(f.case("members_in_stored_payload"))
    f = good2().add(text(80, 65), extra=b"ZZ" + struct.pack("<H", len(inner)) + inner).add(text(50, 66))
    out.append(f.case("member_in_fextra"))
    f = File().add(text(80, 67), mtime=0x00088B1F).add(text(80, 68), mtime=0x00088B1F, flg=FHCRC).add(text(5, 69))
    out.append(f.case("mtime_is_the_magic"))
    mid = member(b"pq" + inner + b"rs", level=0)  # a decoy whose stored payload holds a decoy
    f = good2().add(b"12345" + mid + b"678", level=0).add(text(50, 70))
    out.append(f.case("decoy_in_a_decoy"))
    # a decoy inside the header of the member at position 0
    f = File().add(text(20, 71), extra=b"ZZ" + struct.pack("<H", len(inner)) + inner).add(text(50, 72))
    out.append(f.case("decoy_in_first_header"))
    return out


# ---- stops -----------------------------------------------------------------------------------------

def stop_cases():
    out = []
    whole = member(text(4000, 80), name=b"a name", comment=b"and a comment")
    body_at = len(header(name=b"a name", comment=b"and a comment"))
    block3 = header() + b"\x07" + trailer(b"")  # BFINAL 1, BTYPE 3
    c = text(900, 81)
    stops = {
        "cut_in_header": whole[:body_at - 5],
        "cut_in_header_after_4": whole[:4],
        "cut_in_deflate": whole[:body_at + 700],
        "cut_in_trailer_1": whole[:-1],
        "cut_in_trailer_5": whole[:-5],
        "cut_before_trailer": whole[:-8],
        "trailing_1": b"\x1f",
        "trailing_2": b"\x1f\x8b",
        "trailing_3": b"\x1f\x8b\x08",
        "trailing_zeros": bytes(8),
        "trailing_zeros_4": bytes(4),
        "zlib_stream": zlib.compress(c),
        "1f_8b_07": b"\x1f\x8b\x07" + whole[3:],
        "reserved_flg_bit_5": whole[:3] + bytes([whole[3] | 0x20]) + whole[4:],
        "reserved_flg_bit_7": whole[:3] + bytes([whole[3] | 0x80]) + whole[4:],
        "block_type_3": block3,
        "wrong_isize": header() + deflate(c) + trailer(c, isize_add=1),
        "wrong_fhcrc": header(flg=FHCRC, hcrc_xor=0x0101) + deflate(c) + trailer(c),
        "distance_too_far": header() + far_match_block() + trailer(b"aaaa"),
        "stored_len_nlen": header() + b"\x01\x05\x00\xfa\xfe" + b"hello" + trailer(b"hello"),
    }
    for name, tail in stops.items():
        out.append(File().raw(tail).case("first_" + name))
        out.append(good2().raw(tail).case("third_" + name))
    # a stop in the middle leaves what follows unlisted
    out.append(good2().raw(block3).raw(member(text(30, 82))).case("block_type_3_then_a_good_member"))
    out.append(good2().raw(bytes(5)).raw(member(text(30, 83))).case("zeros_then_a_good_member"))
    # a wrong CRC-32 is not seen: the member is listed, its neighbours too
    out.append(File().add_bad_crc(text(500, 84)).case("first_wrong_crc"))
    out.append(good2().add_bad_crc(text(500, 85)).add(text(60, 86)).case("third_wrong_crc"))
    # a wrong CRC and a cut ISIZE: the size pass reads the cut (rule 2's exemption), and so does the twin
    f = good2()
    m = member(text(200, 87))
    f.data += m[:-8] + b"\0\0\0\0" + m[-4:-2]
    f.twin += m[:-2]
    out.append(f.case("third_wrong_crc_and_cut_isize"))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = kind_cases() + position_cases() + count_cases() + decoy_cases() + stop_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert len(c.data) == len(c.twin)
    return cases


def by_name(name):
    return {c.name: c for c in all_cases()}[name]


# ---- sizes at the 2^32 edge ------------------------------------------------------------------------

MIB = 1 << 20


@functools.lru_cache(maxsize=None)
def zero_chunks():
    """(C, D): the raw-deflate bytes zlib level 9 writes for 1 MiB of zeros, and for 2^20 - 2 zeros, each followed by Z_FULL_FLUSH,
    taken as the second such piece of a stream: it starts and ends at a byte, needs nothing in front of it, and repeats byte for
    byte."""
    def second(n):
        co = zlib.compressobj(9, zlib.DEFLATED, -15)
        pieces = [co.compress(bytes(k)) + co.flush(zlib.Z_FULL_FLUSH) for k in (MIB, n, n)]
        assert pieces[1] == pieces[2]
        return pieces[1]

    return second(MIB), second(MIB - 2)


def zeros_member(k, short_tail=False, crc=0):
    """header + C x k (+ D) + the empty final fixed block + any CRC + ISIZE: k MiB of zeros (+ 2^20 - 2); (member, decoded size)"""
    c, d = zero_chunks()
    size = k * MIB + (MIB - 2 if short_tail else 0)
    return header() + c * k + (d if short_tail else b"") + b"\x03\x00" + struct.pack("<II", crc, size & 0xFFFFFFFF), size


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[(name, file, rows, summary)] by arithmetic: a member of 2^32 bytes is TOO_LARGE, one of 2^32 - 2 is a member"""
    over, over_size = zeros_member(4096)
    edge, edge_size = zeros_member(4095, short_tail=True)
    assert over_size == 1 << 32 and edge_size == 0xFFFFFFFE
    small = member(text(100, 90))
    return [
        ("size_2_pow_32", small + over, [(0, len(small), 0, 100)], (1, 100, len(small), TOO_LARGE, 0)),
        ("size_2_pow_32_minus_2", edge, [(0, len(edge), 0, edge_size)], (1, edge_size, len(edge), OK, 0)),
        ("two_of_2_pow_32_minus_2", edge + edge, [(0, len(edge), 0, edge_size), (len(edge), len(edge), edge_size, edge_size)],
         (2, 2 * edge_size, 2 * len(edge), OK, 0)),
    ]


# ---- calling the library into poisoned arrays ------------------------------------------------------

POISON64, POISON32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def new_summary():
    from compu_amd.api import _GzipPlanSummary

    return _GzipPlanSummary(7, 7, 7, 7, 7)


def check_arrays(arrs, s, max_members):
    """Nothing behind min(n_members, max_members) is written; returns (rows, summary tuple)."""
    k = min(int(s.n_members), max_members)
    assert k <= len(arrs[0])
    for a, poison in zip(arrs, (POISON64, POISON32, POISON64, POISON32)):
        assert (a[k:] == poison).all(), "entries behind min(n_members, max_members) were written"
    rows = [tuple(int(a[i]) for a in arrs) for i in range(k)]
    return rows, (int(s.n_members), int(s.total_out), int(s.in_used), int(s.status), int(s.member_status))
