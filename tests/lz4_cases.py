"""The shared LZ4 case lists: raw blocks and frames built by tests/lz4_writer.py, good and bad.  A case is (name, data, cap): cap
None means ample room (what the unit decodes to, plus a little).  What each must answer is lz4_ref's business."""
import functools
import random
import struct

import lz4_ref as R
import lz4_writer as W

GROUP = 64  # sequences the kernel parses and executes together (lz4_unit.h)

WORDS = (b"alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau upsilon phi chi psi omega "
         b"the quick brown fox jumps over the lazy dog and runs away ").split()


def text(n, seed):
    """word salad: compressible, never the same twice"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS) + (b" " if rng.random() < 0.9 else b"\n")
    return bytes(out[:n])


def noise(n, seed):
    return random.Random(seed).randbytes(n)


def chain(n_seq, seed, first=b"0123456789abcdef"):
    """n_seq sequences of short literals and short matches at mixed offsets, overlapping ones included"""
    rng = random.Random(seed)
    seqs, produced = [], 0
    for k in range(n_seq):
        lits = first if k == 0 else noise(rng.randrange(0, 4), seed * 1000 + k)
        produced += len(lits)
        off = rng.randrange(1, min(produced, 300) + 1)
        ml = rng.randrange(4, 24)
        seqs.append((lits, off, ml))
        produced += ml
    return seqs


@functools.lru_cache(maxsize=None)
def block_cases():
    c = []
    lead = [(b"abcdefgh", 3, 5)]
    for L in (0, 1, 14, 15, 16, 269, 270, 271, 15 + 2 * 255 + 3, 70000):
        c.append((f"lit{L}", W.block(lead + [(noise(L, L), 7, 6)], b"xyz"), None))
    for M in (4, 18, 19, 20, 273, 274, 70000):
        for off in (16, 1, 3):
            c.append((f"match{M}_off{off}", W.block([(b"0123456789abcdef", off, M)], b"."), None))
    for off in (1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 65535):
        for ml in (4, 19, 100, 300):
            c.append((f"off{off}_ml{ml}", W.block([(noise(off, off + 7), off, ml)], b"tail"), None))
    for off in range(1, 20):
        for ml in range(4, 41):
            c.append((f"overlap_off{off}_ml{ml}", W.block([(b"ABCDEFGHIJKLMNOPQRST", off, ml)], b"!"), None))
    for n in (1, 63, 64, 65, 128, 129):
        c.append((f"seqs{n}", W.block(chain(n, n), b"end"), None))
        c.append((f"seqs{n}_ends_empty", W.block(chain(n, n + 1000), b""), None))
    # a match whose source straddles the boundary between two groups: sequence GROUP (the second group's first) reads the last
    # bytes the first group wrote and the literals it has just placed itself
    g = chain(GROUP, 77)
    c.append(("straddle", W.block(g + [(b"STRADL", 10, 9), (b"", 3, 11)], b"fin"), None))
    c.append(("straddle_overlap", W.block(g + [(b"xy", 8, 30)], b"fin"), None))
    c.append(("straddle_long", W.block(g + [(b"xy", 70, 400)], b"fin"), None))
    # a match sourced from the match just before it
    c.append(("match_from_match", W.block([(b"abcdefgh", 8, 8), (b"", 8, 8), (b"", 4, 12), (b"", 12, 12), (b"z", 1, 9)], b""), None))
    c.append(("block_00", b"\x00", None))
    c.append(("block_00_nibble", b"\x0f", None))  # the last token's low nibble is not looked at
    c.append(("lit_only_1", W.block([], b"Q"), None))
    c.append(("lit_only_200000", W.block([], noise(200000, 5)), None))
    c.append(("empty_input", b"", None))
    c.append(("ext_not_canonical", W.sequence(b"x" * 15, 1, 19, ll_ext=[0], ml_ext=[0]) + W.sequence(b"yz"), None))
    c.append(("ends_after_match", W.block([(b"abcd", 2, 6)], end=False), None))
    # truncation of a ~150-byte block at every length
    blk = W.compress_block(text(260, 3))
    assert 120 <= len(blk) <= 200, len(blk)
    for n in range(len(blk)):
        c.append((f"cut{n}", blk[:n], None))
    # each offset error at the first, a middle and the last sequence
    base = chain(9, 31)
    for k in (0, 4, 8):
        for what, off in (("zero", 0), ("far", None)):
            s = list(base)
            produced = sum(len(l) + m for l, _, m in s[:k]) + len(s[k][0])
            s[k] = (s[k][0], produced + 1 if off is None else off, s[k][2])
            c.append((f"offset_{what}_seq{k}", W.block(s, b"end"), None))
    # out_cap at every value from 0 to the full size of a ~100-byte block
    seqs, last = W.compress(text(100, 9) + text(100, 9)[:40])
    small = W.block(seqs, last)
    full = len(W.expand(seqs, last))
    for cap in range(full + 1):
        c.append((f"cap{cap}", small, cap))
    return c


def _three(seed=1, sizes=(700, 650, 300)):
    return text(sum(sizes), seed), list(sizes)


@functools.lru_cache(maxsize=None)
def frame_cases():
    c = []
    data, sizes = _three()
    for bits in range(16):
        kw = dict(linked=not bits & 1, bchk=bool(bits & 2), csize=bool(bits & 4), cchk=bool(bits & 8))
        c.append(("flags_" + "".join(k[0] + str(int(v)) for k, v in kw.items()), W.frame_of(data, sizes, **kw), None))
    for bd in (5, 6, 7):
        c.append((f"bd{bd}", W.frame_of(text(70000, bd), 70000, bd=bd, cchk=True), None))
    c.append(("stored", W.frame_of(noise(900, 2), [300, 300, 300], stored_every=1, bchk=True, cchk=True), None))
    c.append(("stored_mixed", W.frame_of(data, sizes, stored_every=2, cchk=True, csize=True), None))
    c.append(("no_block", W.frame([], cchk=True, csize=True), None))
    c.append(("no_block_plain", W.frame([]), None))
    c.append(("short_middle", W.frame_of(text(1301, 4), [650, 1, 650], cchk=True), None))
    c.append(("stored_empty_block", W.frame([(False, W.compress_block(text(50, 1))), (True, b""), (True, b"xy")], cchk=True), None))
    c.append(("trailing", W.frame_of(data, sizes, cchk=True) + b"\x00\x01trailing bytes", None))
    # linked blocks: the second block copies 65 535 back; independent, the same bytes reach in front of their block
    far = [(True, noise(65535, 8) + b"0123456789"), (False, W.block([(b"", 65535, 20), (b"ab", 65535, 5)], b"end"))]
    c.append(("linked_65535", W.frame(far, indep=False, bd=5, cchk=True), None))
    c.append(("indep_reaches_back", W.frame(far, content=b"", indep=True, bd=5), None))
    c.append(("linked_before_frame", W.frame([(True, b"0123456789"), (False, W.block([(b"ab", 13, 5)], b"end"))], content=b"", indep=False), None))
    # every rule violated once
    good = dict(cchk=True, csize=True, bchk=True)
    c.append(("short_6", W.frame_of(data, sizes)[:6], None))
    for name, magic in (("legacy", 0x184C2102), ("skippable", 0x184D2A50), ("skippable_f", 0x184D2A5F), ("zstd", 0xFD2FB528)):
        c.append((f"magic_{name}", W.frame_of(data, sizes, magic=magic), None))
    c.append(("version_0", W.frame_of(data, sizes, version=0), None))
    c.append(("version_2", W.frame_of(data, sizes, version=2), None))
    c.append(("flg_reserved", W.frame_of(data, sizes, flg_reserved=1), None))
    c.append(("bd_bit7", W.frame_of(data, sizes, bd_extra=0x80), None))
    c.append(("bd_low_bits", W.frame_of(data, sizes, bd_extra=1), None))
    for code in (0, 3):
        c.append((f"bd_code{code}", W.frame_of(data, sizes, bd=code), None))
    c.append(("bad_hc", W.frame_of(data, sizes, hc=0x11 if W.header()[6] != 0x11 else 0x12), None))
    c.append(("dict_id", W.frame_of(data, sizes, dict_id=7), None))
    c.append(("dict_id_bad_hc", W.frame_of(data, sizes, dict_id=7, hc=(W.header(dict_id=7)[10] + 1) & 0xFF), None))
    c.append(("dict_id_cut", W.frame_of(data, sizes, dict_id=7)[:9], None))
    c.append(("size_field_above_max", W.frame([(False, W.compress_block(text(100, 1))), (False, b"\x00" * 65537)], content=b""), None))
    c.append(("stored_above_max", W.frame([(True, noise(65537, 1))], content=b""), None))
    c.append(("size_field_above_max_absent", W.frame([(False, W.compress_block(text(100, 1)))], content=b"", end_mark=False) + struct.pack("<I", 65537), None))
    c.append(("decodes_above_max", W.frame([(True, b"head"), (False, W.block([(b"0123456789abcdef", 16, 70000)], b"."))], content=b""), None))
    c.append(("decodes_above_max_literals", W.frame([(False, W.block([(b"0123456789abcdef", 16, 65500)], noise(40, 1)))], content=b""), None))
    c.append(("decodes_to_max", W.frame([(False, W.block([(b"0123456789abcdef", 16, 65500)], noise(20, 1)))], cchk=True), None))
    c.append(("block_ends_after_match", W.frame([(True, b"head"), (False, W.block([(b"abcd", 2, 6)], end=False)), (True, b"tail")], content=b""), None))
    c.append(("block_cut_inside", W.frame([(False, W.compress_block(text(300, 2))[:40])], content=b""), None))
    c.append(("block_offset_zero", W.frame([(True, b"head"), (False, W.block([(b"abcd", 0, 6)], b"x"))], content=b""), None))
    for i in range(3):
        c.append((f"bad_block_checksum{i}", W.frame_of(data, sizes, bchk_values={i: 0x12345678}, **good), None))
    c.append(("bad_block_checksum_stored", W.frame_of(data, sizes, stored_every=2, bchk_values={1: 1}, **good), None))
    c.append(("malformed_and_bad_block_checksum", W.frame([(False, W.block([(b"abcd", 2, 6)], end=False))], content=b"", bchk=True, bchk_values={0: 5}), None))
    c.append(("content_size_plus1", W.frame_of(data, sizes, csize=True, csize_value=len(data) + 1), None))
    c.append(("content_size_minus1", W.frame_of(data, sizes, csize=True, cchk=True, csize_value=len(data) - 1), None))
    c.append(("content_size_huge", W.frame_of(data, sizes, csize=True, csize_value=(1 << 63) + 5), None))
    c.append(("bad_content_checksum", W.frame_of(data, sizes, cchk=True, cchk_value=0xDEADBEEF), None))
    c.append(("bad_size_and_content_checksum", W.frame_of(data, sizes, csize=True, cchk=True, csize_value=3, cchk_value=1), None))
    c.append(("bad_size_checksum_cut", W.frame_of(data, sizes, csize=True, cchk=True, csize_value=3)[:-2], None))
    c.append(("no_end_mark", W.frame_of(data, sizes, end_mark=False), None))
    # room: tight by one, by a block, none
    full = W.frame_of(data, sizes, **good)
    for cap in (0, 1, 699, 700, 701, 1349, 1350, 1649):
        c.append((f"room{cap}", full, cap))
    c.append(("room_stored", W.frame_of(data, sizes, stored_every=2), 1000))
    # truncation of a ~200-byte frame at every length
    small = W.frame_of(text(100, 6) * 2 + text(60, 7), [120, 80, 60], **good)
    assert 150 <= len(small) <= 300, len(small)
    for n in range(len(small)):
        c.append((f"cut{n}", small[:n], None))
    return c


def ample(expected_len):
    return expected_len + 9


@functools.lru_cache(maxsize=None)
def parallel_frames():
    """BD 4 frames of 2, 3 and 65 blocks whose blocks hold between 1 and 3 000 bytes: (name, frame kwargs, data, sizes)"""
    out = []
    for n in (2, 3, 65):
        rng = random.Random(n)
        sizes = [rng.choice((1, 2, 17, 300, 1000, 3000)) if n > 3 else (3000, 1, 1700)[i] for i in range(n)]
        out.append((f"blocks{n}", text(sum(sizes), 40 + n), sizes))
    return out
