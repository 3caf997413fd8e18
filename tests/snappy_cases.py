"""The shared Snappy case lists: raw blocks and framed streams built by tests/snappy_writer.py, good and bad -- the smallest shapes
at which the kernel of snappy_unit.h can go wrong.  A case is (name, data, cap): cap None means ample room (ample_block /
ample_frame).  What each must answer is snappy_ref's business."""
import functools
import random

import snappy_ref as R
import snappy_writer as W

GROUP = 64     # elements the kernel parses and executes together (snappy_unit.h)
WINDOW = 2048  # bytes of input it stages in LDS; a tag and its bytes are fetched as 8 bytes of it

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


def ample_block(data):
    """room for what the block states (where that is sane) and for what it decodes to, and a little"""
    content, status, _ = R._block(data, 0, len(data), None, False)
    n, shift = 0, 0
    for b in data[:5]:
        n |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    return max(len(content), n if n <= 1 << 20 else 0) + 9


def ample_frame(data):
    """room for what the stream decodes to and for one more chunk"""
    return R.frame_decode(data, None, checks=False)[1] + R.CHUNK_MAX + 9


def chain(n_elems, seed):
    """n_elems elements: short literals and copies at mixed offsets and in mixed forms, overlapping ones included"""
    rng = random.Random(seed)
    elems, produced = [("lit", b"0123456789abcdef")], 16
    while len(elems) < n_elems:
        if rng.random() < 0.4:
            lit = noise(rng.randrange(1, 9), seed * 1000 + len(elems))
            elems.append(("lit", lit, rng.choice((None, None, 1, 2))))
            produced += len(lit)
        else:
            off, m = rng.randrange(1, min(produced, 300) + 1), rng.randrange(1, 30)
            forms = [2, 4] + ([1] if 4 <= m <= 11 else [])
            elems.append(("copy", off, m, rng.choice(forms)))
            produced += m
    return elems


def fill_to(t, pre=2):
    """elements whose bytes, behind a preamble of `pre` bytes, end exactly at position t of the block: literals of 19 bytes and one
    that fits"""
    elems, at, k = [], pre, 0
    while t - at > 40:
        elems.append(("lit", noise(19, 500 + k)))
        at += 20
        k += 1
    rest = t - at  # 2 .. 40 bytes: a tag and rest - 1 literal bytes
    assert 2 <= rest <= 41
    elems.append(("lit", noise(rest - 1, 900)))
    return elems


@functools.lru_cache(maxsize=None)
def block_cases():
    c = []

    def add(name, elems, **kw):
        c.append((name, W.block(elems, **kw), None))

    # literals: every length in every form that can hold it
    for L in (1, 59, 60, 61, 255, 256, 257, 65535, 65536, 65537, 70000, 200000):
        for form in range(5):
            if L <= (60 if form == 0 else 1 << (8 * form)):
                add(f"lit{L}_form{form}", [("lit", b"abcdefgh"), ("copy", 3, 5), ("lit", noise(L, L), form), ("copy", 7, 6), ("lit", b"xyz")])
    add("lit_2pow32", [W.literal(b"0123456789", form=4, stated=1 << 32)], n=10)
    add("lit_2pow32_behind", [("lit", b"ab"), W.literal(b"0123456789", form=4, stated=1 << 32)], n=12)
    # copies: each form at its offsets, every length
    for off in list(range(1, 13)) + [2047]:
        for m in range(4, 12):
            add(f"copy1_off{off}_m{m}", [("lit", noise(off, off)), ("copy", off, m, 1), ("lit", b"!")])
    for off in list(range(1, 71)) + [2048, 65535]:
        elems = [("lit", noise(off, off + 7))]
        for m in range(1, 65):
            elems += [("copy", off, m, 2), ("lit", noise(3, m))]
        add(f"copy2_off{off}", elems)
    for off in (1, 65536, 70000):
        for m in (1, 4, 33, 64):
            add(f"copy4_off{off}_m{m}", [("lit", noise(off, off + 9)), ("copy", off, m, 4), ("lit", b"tail")])
    for off in range(1, 20):
        for m in range(1, 65):
            add(f"overlap_off{off}_m{m}", [("lit", b"ABCDEFGHIJKLMNOPQRST"), ("copy", off, m, 2), ("lit", b"!")])
    # chains and group boundaries
    for n in (1, 63, 64, 65, 128, 129):
        add(f"elems{n}", chain(n, n))
    g = chain(GROUP, 77)
    add("straddle", g + [("copy", 10, 9), ("lit", b"STRADL"), ("copy", 3, 11)])
    add("straddle_overlap", g + [("copy", 2, 30)])
    add("straddle_far", g + [("copy", len(W.expand(g)), 64, 4)])
    add("copy_from_copy", [("lit", b"abcdefgh"), ("copy", 8, 8), ("copy", 8, 8), ("copy", 4, 12), ("copy", 12, 12), ("lit", b"z"), ("copy", 1, 9)])
    # the LDS window's edge: a copy-4 and a 4-byte literal length whose tag lies at every position around it, whatever the
    # unit's alignment (the window begins at the aligned dword that holds the block's first byte)
    for t in range(WINDOW - 24, WINDOW + 6):
        add(f"edge_copy4_at{t}", fill_to(t) + [("copy", 17, 9, 4), ("lit", b"after")])
        add(f"edge_lit4_at{t}", fill_to(t) + [("lit", noise(300, t), 4), ("copy", 5, 7)])
    add("edge_short_literal_crosses", fill_to(WINDOW - 20) + [("lit", noise(45, 1)), ("copy", 40, 20)])
    add("edge_long_literal_crosses", fill_to(WINDOW - 100) + [("lit", noise(3000, 2)), ("copy", 2999, 64)])
    # empty blocks
    c.append(("block_00", b"\x00", None))
    c.append(("block_00_and_a_byte", b"\x00\x41", None))
    c.append(("empty_input", b"", None))
    # preambles
    for k in range(1, 6):
        add(f"preamble_{k}_bytes", [("lit", b"hello")], preamble=W.varint(5, k))
    c.append(("preamble_80_00", b"\x80\x00", None))
    c.append(("preamble_fifth_0f", b"\xff\xff\xff\xff\x0f" + W.literal(b"0123456789"), None))  # 2^32 - 1 over ten bytes
    c.append(("preamble_fifth_10", b"\xff\xff\xff\xff\x10" + W.literal(b"0123456789"), None))
    c.append(("preamble_fifth_80", b"\x80\x80\x80\x80\x80\x00", None))
    for k in range(1, 5):
        c.append((f"preamble_cut{k}", b"\x80\x80\x80\x80\x00"[:k], None))
    # errors: each offset error at the first copy, a middle one and the last; one byte too much and too few against n
    base = [("lit", b"0123456789abcdef")] + [e for k in range(9) for e in (("copy", 5 + k, 6), ("lit", noise(2, k)))]
    copies = [i for i, e in enumerate(base) if e[0] == "copy"]
    for which, i in (("first", copies[0]), ("middle", copies[4]), ("last", copies[-1])):
        produced = len(W.expand(base[:i]))
        for what, off in (("zero", 0), ("far", produced + 1)):
            bad = list(base)
            bad[i] = ("copy", off, 6, 2)
            c.append((f"offset_{what}_{which}", W.block(bad, n=len(W.expand(base))), None))
    full = len(W.expand(base))
    add("n_one_too_few", base, n=full + 1)   # the elements end one byte short of n
    add("n_one_too_much", base, n=full - 1)  # the last literal takes the block beyond n
    add("n_copy_too_much", base[:-1], n=len(W.expand(base[:-1])) - 1)
    add("n_reached_bytes_remain", base + [("lit", b"q")], n=full)
    # every prefix of a ~150-byte block
    blk = W.compress_block(text(260, 3))
    assert 120 <= len(blk) <= 200, len(blk)
    for n in range(len(blk)):
        c.append((f"cut{n}", blk[:n], None))
    # out_cap from 0 to n
    small = W.compress_block(text(100, 9) + text(100, 9)[:40])
    for cap in range(141):
        c.append((f"cap{cap}", small, cap))
    return c


def _three(seed=1, sizes=(700, 650, 300)):
    return text(sum(sizes), seed), list(sizes)


@functools.lru_cache(maxsize=None)
def frame_cases():
    c = []

    def add(name, chunks, cap=None, ident=True):
        c.append((name, W.stream(chunks, ident), cap))

    data, sizes = _three()
    good = [W.data_chunk(data[:700]), W.data_chunk(data[700:1350], compressed=False), W.data_chunk(data[1350:])]
    add("three_chunks", good)
    add("ident_alone", [])
    add("no_ident", good, ident=False)
    c.append(("ident_wrong_length", b"\xff\x07\x00\x00sNaPpY!" + good[0], None))
    c.append(("ident_wrong_bytes", b"\xff\x06\x00\x00sNaPpy" + good[0], None))
    c.append(("ident_wrong_type", b"\xfe\x06\x00\x00sNaPpY" + good[0], None))
    add("ident_repeated", [good[0], R.IDENT, good[1], R.IDENT, R.IDENT, good[2]])
    add("ident_repeated_wrong", [good[0], b"\xff\x06\x00\x00sNaPpy", good[1]])
    add("ident_repeated_long", [good[0], W.chunk(0xFF, b"sNaPpY!"), good[1]])
    for kind in (True, False):
        for n in (1, 65536, 65537):
            add(f"{'compressed' if kind else 'uncompressed'}_{n}", [good[0], W.data_chunk(text(n, n), compressed=kind)])
    add("compressed_65537_noise", [W.data_chunk(noise(65537, 1))])
    add("empty_chunks", [W.data_chunk(b""), W.data_chunk(b"", compressed=False), good[0]])
    for s in range(4):
        for kind in (0, 1):
            add(f"type{kind}_s{s}", [good[0], W.chunk(kind, b"\x01\x02\x03"[:s]), good[1]])
    add("padding", [W.padding(0), good[0], W.padding(1), W.padding(300), good[1], W.padding(7)])
    for kind in (0x80, 0xFD):
        add(f"skippable_{kind:02x}", [W.chunk(kind, b"skip me"), good[0], W.chunk(kind, b""), good[2]])
    for kind in (0x02, 0x7F):
        add(f"reserved_{kind:02x}", [good[0], W.chunk(kind, b"no"), good[1]])
    for i in range(3):
        bad = list(good)
        bad[i] = W.data_chunk(data[sum(sizes[:i]):sum(sizes[:i + 1])], compressed=i != 1, crc=0x12345678)
        add(f"bad_crc{i}", bad)
    add("crc_unmasked", [W.data_chunk(data[:700], crc=R.crc32c(data[:700]))])
    blk = W.compress_block(data[:700])
    add("block_cut_inside", [good[1], W.data_chunk(data[:700], body=blk[:40]), good[2]])
    add("block_trailing_byte", [good[1], W.data_chunk(data[:700], body=blk + b"\x00"), good[2]])
    add("block_preamble_cut", [good[1], W.data_chunk(b"", body=b"\x80")])
    add("block_preamble_bad", [good[1], W.data_chunk(b"", body=b"\x80\x80\x80\x80\x10")])
    add("block_offset_zero", [good[1], W.data_chunk(b"", body=W.block([("lit", b"abcd"), ("copy", 0, 4, 2)], n=8))])
    add("block_length", [good[1], W.data_chunk(b"", body=W.block([("lit", b"abcd"), ("copy", 2, 6)], n=9))])
    # pairs that pin the order of the checks
    add("reserved_and_cut", [good[0], W.chunk(0x02, b"abc", s=9)])                       # the length is looked at before the type
    add("bad_ident_and_cut", [good[0], W.chunk(0xFF, b"sNaPp", s=7)])
    add("s3_and_cut", [good[0], W.chunk(0x00, b"ab", s=3)])
    add("damaged_then_cut", [good[0], W.data_chunk(b"", body=blk[:40]), good[2][:20]])  # the fourth chunk is cut, the second answers
    add("bad_crc_then_reserved", [W.data_chunk(data[:700], crc=1), W.chunk(0x03, b"")])
    add("too_large_and_bad_crc", [W.data_chunk(noise(65537, 2), compressed=False, crc=5)])
    add("stated_too_large_no_room", [W.data_chunk(b"", body=W.varint(65537) + W.literal(b"x"))], cap=10)
    add("damaged_and_bad_crc", [W.data_chunk(b"", body=blk[:40], crc=7)])
    add("header_cut_3", [good[0], b"\x00\x10\x00"])
    # tight room: by one, by a chunk, none
    for cap in (0, 1, 699, 700, 701, 1349, 1350, 1649):
        add(f"room{cap}", good, cap=cap)
    # every prefix of a ~250-byte stream
    small = W.stream([W.data_chunk(text(160, 6) * 2), W.padding(3), W.data_chunk(noise(40, 7), compressed=False), W.data_chunk(text(90, 8))])
    assert 200 <= len(small) <= 320, len(small)
    for n in range(len(small)):
        c.append((f"cut{n}", small[:n], None))
    return c


@functools.lru_cache(maxsize=None)
def parallel_streams():
    """streams of 2, 3 and 65 data chunks of 1 to 3 000 bytes, both types mixed, padding and skippable chunks between them:
    (name, stream, content, n_chunks, n_skipped)"""
    out = []
    for n in (2, 3, 65):
        rng = random.Random(n)
        sizes = [rng.choice((1, 2, 17, 300, 1000, 3000)) if n > 3 else (3000, 1, 1700)[i] for i in range(n)]
        data = text(sum(sizes), 40 + n)
        parts, p, skipped = [], 0, 0
        for k, size in enumerate(sizes):
            if k % 3 == 1:
                parts += [W.padding(k % 5), W.chunk(0x80 + k % 0x7E, b"between")]
                skipped += 2
            parts.append(W.data_chunk(data[p:p + size], compressed=k % 4 != 2))
            p += size
        out.append((f"chunks{n}", W.stream(parts), data, n, skipped))
    return out
