"""The walk that defines CHIP_F_MEMBERS (include/compu_hip.h), in Python: what a unit that is a series of gzip members or of zstd
frames must answer, given `decode1` -- what a unit without the flag answers for the rest of the input and the room that is left.

decode1 defaults to the CPU oracle read as the batch call documents its default status, one unit at a time: oracle.InflateDecoder / ZstdDecoder, the single-unit form of
oracle.inflate_units / zstd_units (the batch entry points do not report the input consumed, which the walk needs).  A GPU test passes
the unflagged chip_decode_batch as decode1 instead and thereby checks the contract to the letter.  Shared by tests/test_members_cpu.py
and tests/test_members_gpu.py."""
from collections import namedtuple

from oracle import oracle as O

NEED_INPUT, NEED_OUTPUT, FINISHED = 0, 1, 2
GZIP, AUTO, ZSTD = 31, 47, 100
ZSTD_MAGIC = 0xFD2FB528

# status, out_len, in_used, the bytes; `last_p`: where the last member started; `members`: how many were started
Answer = namedtuple("Answer", "status out_len in_used data last_p members")


def oracle_decode1(fmt):
    """(status, bytes, in_used) of the oracle for one unit of `fmt` with `room` bytes of output"""

    def decode1(data, room):
        d = O.ZstdDecoder() if fmt == ZSTD else O.InflateDecoder(fmt)
        got, in_rem, _out_rem, st, err = d.decode(data, int(room))
        if fmt != ZSTD and not err and len(data) == 0:
            # an empty deflate / zlib / gzip unit: zlib answers Z_BUF_ERROR, which compu maps to NeedOutput; the batch status names
            # the cause, CHIP_NEED_INPUT (include/compu_hip.h, pinned by tests/test_inflate_gpu.py)
            assert st == NEED_OUTPUT
            st = NEED_INPUT
        return (err if err else st), got, len(data) - in_rem

    return decode1


def starts_member(fmt, unit, p, first_two):
    """"another member starts at p": only behind a member of the same family (`first_two`: the first bytes of the member just
    finished -- under CHIP_FMT_AUTO a zlib member is never continued)"""
    rest = len(unit) - p
    if fmt == ZSTD:
        if rest < 4:
            return False
        magic = int.from_bytes(unit[p:p + 4], "little")
        return magic == ZSTD_MAGIC or 0x184D2A50 <= magic <= 0x184D2A5F
    return first_two == b"\x1f\x8b" and rest >= 2 and unit[p:p + 2] == b"\x1f\x8b"


def walk(fmt, unit, cap, decode1=None, sizes=False):
    """The flagged answer for `unit` (bytes) with out_cap `cap`.  sizes: the size pass -- no room limit (decode1 is called with `cap` for
    every member; pass a cap that is ample)."""
    decode1 = decode1 or oracle_decode1(fmt)
    unit = bytes(unit)
    p, total, out, members = 0, 0, [], 0
    while True:
        members += 1
        st, got, iu = decode1(unit[p:], cap if sizes else cap - total)
        total += len(got)
        out.append(got)
        if st != FINISHED:
            return Answer(st, total, len(unit) if st == NEED_INPUT else p + iu, b"".join(out), p, members)
        first_two = unit[p:p + 2]
        last_p = p
        p += iu
        if iu > 0 and starts_member(fmt, unit, p, first_two):
            continue
        return Answer(FINISHED, total, p, b"".join(out), last_p, members)
