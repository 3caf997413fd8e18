"""Frames for the block description of one zstd frame (chip_zstd_blocks_host / chip_zstd_blocks), built with
tests/zstd_writer.py, and what each must be described as.

A case is (name, frame, rows, summary): `rows` one dict per block with what the CASE built -- type, size, last, and for a compressed
block lit_type, lit_regen, n_seq and modes -- plus `src`, the four source indices (Huffman, LL, OF, ML) written out by hand;
`summary` the fields of chip_zstd_blocks_summary the case pins.  py_blocks() is a second, independent reading of a frame's headers
in Python: the tests hold the library against both."""
import functools
import random
from collections import namedtuple

import zstd_writer as W
from zstd_writer import new_offset as N

OK, TRUNCATED, BAD_HEADER, TOO_LARGE = 0, 1, 2, 3
UNSIZED = 0xFFFFFFFFFFFFFFFF
LAST, MALFORMED = 1, 2
MAX_BLOCKS = 1 << 20
RAW, RLE, COMPRESSED = 0, 1, 2
LIT = {"raw": 0, "rle": 1, "huf": 2, "treeless": 3}

Case = namedtuple("Case", "name frame rows summary content")


def _mode(m):
    return 0 if m == "pre" else 3 if m == "rep" else 1 if m[0] == "rle" else 2


class Built:
    """A zstd_writer.Frame that writes down what it was asked to build."""

    def __init__(self, **kw):
        self.f = W.Frame(**kw)
        self.rows = []

    def raw(self, data, last=False):
        self.f.raw(data, last=last)
        self.rows.append(dict(type=RAW, size=len(data), last=last))
        return self

    def rle(self, byte, n, last=False):
        self.f.rle(byte, n, last=last)
        self.rows.append(dict(type=RLE, size=n, last=last))
        return self

    def compressed(self, lits=b"", seqs=(), lit="raw", modes=("pre", "pre", "pre"), last=False, **kw):
        before = len(self.f.blocks)
        self.f.compressed(lits, seqs, lit=lit, modes=modes, last=last, **kw)
        row = dict(type=COMPRESSED, size=len(self.f.blocks) - before - 3, last=last, lit_type=LIT[lit], lit_regen=len(lits), n_seq=len(seqs),
                   modes=tuple(_mode(m) for m in modes) if seqs else (0, 0, 0))
        if lit in ("raw", "rle"):
            row["lit_comp"] = len(lits) if lit == "raw" else 1
        self.rows.append(row)
        return self

    def case(self, name, src, **summary):
        """src: per block (huf, ll, of, ml)"""
        frame, content = self.f.finish()
        assert len(src) == len(self.rows), name
        cuts = self.f.block_cuts()
        for k, (row, s) in enumerate(zip(self.rows, src)):
            row["src"] = tuple(s)
            row["offset"] = cuts[k]
        summary.setdefault("status", OK)
        summary.setdefault("n_blocks", len(self.rows))
        summary.setdefault("in_used", len(frame))
        summary.setdefault("header_bytes", cuts[0])
        return Case(name, frame, self.rows, summary, content)


def _rb(rnd, n, lo=97, hi=123):
    return bytes(rnd.randrange(lo, hi) for _ in range(n))


def _seqs(rnd, n, avail):
    return [(rnd.choice([0, 1, 2, 5, 17]), rnd.randrange(3, 40), rnd.choice([1, 2, N(rnd.randrange(1, avail))])) for _ in range(n)]


def _lits(rnd, seqs, extra=7):
    return rnd.randbytes(sum(s[0] for s in seqs) + extra)


def _definer(kind, codes, k):
    if kind == "pre":
        return "pre"
    if kind == "rle":
        return ("rle", codes[k][0])
    al = 6 if k != 1 else 5
    return ("fse", W.fit(codes[k], al), al)


def source_cases():
    rnd = random.Random(419)
    out = []
    # treeless after a Huffman block, with a raw block and a raw-literals block between them
    b = Built(checksum=True)
    b.compressed(bytes(range(60, 90)) + _rb(rnd, 900, 60, 90), [(100, 30, N(40))], lit="huf", streams=4)
    b.raw(rnd.randbytes(77))
    b.compressed(rnd.randbytes(50), [(20, 5, 1)])
    b.compressed(_rb(rnd, 800, 60, 90), [(0, 9, 2), (300, 12, N(600))], lit="treeless", streams=4)
    b.compressed(_rb(rnd, 60, 60, 90), [], lit="treeless", streams=1)
    b.compressed(_rb(rnd, 200, 60, 90) + bytes(range(60, 90)), [], lit="huf", streams=1)
    b.compressed(_rb(rnd, 40, 60, 90), [(3, 4, 1)], lit="treeless", streams=1, last=True)
    out.append(b.case("treeless_after_huf_raw_rawlit", [(-1, -1, -1, -1), (0, 0, 0, 0), (0, 0, 0, 0), (0, 2, 2, 2), (0, 3, 3, 3), (0, 3, 3, 3),
                                                        (5, 3, 3, 3)]))
    # Repeat of each table over each kind of definer; the other two tables predefined
    for k, t in enumerate(("ll", "of", "ml")):
        for kind in ("fse", "rle", "pre"):
            b = Built()
            b.raw(rnd.randbytes(3000))
            seqs1 = [(5, 9, N(77))] * 4 if kind == "rle" else _seqs(rnd, 60, 3000)
            codes = W.seq_codes(seqs1)
            b.compressed(_lits(rnd, seqs1), seqs1, modes=tuple(_definer(kind, codes, j) if j == k else "pre" for j in range(3)))
            seqs2 = [seqs1[j] for j in rnd.sample(range(len(seqs1)), min(len(seqs1), 20))]
            rep = tuple("rep" if j == k else "pre" for j in range(3))
            b.compressed(_lits(rnd, seqs2), seqs2, modes=rep)
            b.compressed(_lits(rnd, seqs2), seqs2, modes=rep, last=True)  # a Repeat block defines nothing: the source stays block 1
            three = (-1,) + tuple(2 if j != k else 1 for j in range(3))
            out.append(b.case(f"rep_{t}_over_{kind}", [(-1, -1, -1, -1), (-1, -1, -1, -1), (-1, 1, 1, 1), three]))
    # a block with no sequences in between is stepped over
    b = Built()
    b.raw(rnd.randbytes(2000))
    seqs = _seqs(rnd, 40, 2000)
    c = W.seq_codes(seqs)
    b.compressed(_lits(rnd, seqs), seqs, modes=(("fse", W.fit(c[0], 7), 7), ("fse", W.fit(c[1], 5), 5), ("fse", W.fit(c[2], 8), 8)))
    b.compressed(rnd.randbytes(33), [])
    b.rle(0x41, 10)
    b.compressed(_lits(rnd, seqs), seqs[::-1], modes=("rep", "rep", "rep"), last=True)
    out.append(b.case("rep_over_noseq_block", [(-1, -1, -1, -1), (-1, -1, -1, -1), (-1, 1, 1, 1), (-1, 1, 1, 1), (-1, 1, 1, 1)]))
    # a reuse with no source
    for k, t in enumerate(("ll", "of", "ml")):
        b = Built()
        b.raw(rnd.randbytes(100))
        b.compressed(rnd.randbytes(9), [])
        b.compressed(b"xyz", [(1, 5, N(50))], modes=tuple("rep" if j == k else "pre" for j in range(3)), invalid=1)
        b.compressed(b"xyz", [(1, 5, N(50))], last=True)
        four = (-1,) + tuple(2 if j != k else -1 for j in range(3))
        out.append(b.case(f"rep_{t}_without_source", [(-1, -1, -1, -1), (-1, -1, -1, -1), (-1, -1, -1, -1), four]))
    b = Built()
    b.raw(b"no table yet")
    b.compressed(_rb(rnd, 100, 60, 90), [], lit="treeless", weights=W.huf_weights(bytes(range(60, 90))), last=True)
    out.append(b.case("treeless_without_source", [(-1, -1, -1, -1), (-1, -1, -1, -1)]))
    return out


def form_cases():
    """frame header forms, block types mixed, every size format of the two section headers"""
    rnd = random.Random(420)
    out = []
    b = Built(fcs=None, window=(3, 5), checksum=True)
    b.raw(rnd.randbytes(9000)).rle(0x5A, 70000).compressed(_rb(rnd, 10), [(2, 50, N(9000))]).raw(b"", last=True)
    out.append(b.case("mixed_empty_last_window", [(-1, -1, -1, -1)] * 3 + [(-1, 2, 2, 2)], content_size=UNSIZED, window_size=W.window_size(3, 5),
                      descriptor=0x04))
    b = Built(checksum=False)
    b.raw(b"one block of a single-segment frame", last=True)
    out.append(b.case("single_segment_fcs1", [(-1, -1, -1, -1)], content_size=35, window_size=35, descriptor=0x20))
    b = Built(fcs=2, window=(0, 0))
    b.raw(rnd.randbytes(300)).raw(rnd.randbytes(300), last=True)
    out.append(b.case("window_fcs2", [(-1, -1, -1, -1)] * 2, content_size=600, window_size=1024, descriptor=0x40))
    b = Built(fcs=8, dict_id=(0, 4), checksum=True)
    b.rle(9, 5000, last=True)
    out.append(b.case("fcs8_did4", [(-1, -1, -1, -1)], content_size=5000, window_size=5000, descriptor=0xE7, header_bytes=17))
    # literals headers: raw and RLE in 1, 2 and 3 bytes; Huffman in 3, 4 and 5; sequence counts in 1, 2 and 3 bytes
    b = Built(fcs=None, window=(10, 0))
    for n in (0, 31, 32, 4095, 4096, 70000):
        b.compressed(rnd.randbytes(n), [])
        b.compressed(bytes([7]) * n, [], lit="rle")
    b.compressed(rnd.randbytes(5), [], sf=2)
    b.compressed(_rb(rnd, 100), [], lit="huf", streams=1)
    b.compressed(_rb(rnd, 1000), [], lit="huf", streams=4)
    b.compressed(_rb(rnd, 5000), [], lit="treeless", streams=4)
    b.compressed(_rb(rnd, 20000), [], lit="huf", streams=4)
    b.compressed(_rb(rnd, 300), [(1, 3, 1)] * 127, lit="treeless", streams=1)
    b.compressed(b"", [(0, 3, 1)] * 128, modes=(("rle", 0), ("rle", 0), ("rle", 0)))
    b.compressed(b"", [(0, 3, 1)] * 5, nseq_form=2, modes=("rep", "pre", "rep"))
    b.compressed(b"", [(0, 3, 1)] * 0x7F00, modes=("rep", ("rle", 0), "rep"), last=True)
    h = [(-1, -1, -1, -1)] * 14 + [(13, -1, -1, -1), (14, -1, -1, -1), (14, -1, -1, -1), (16, -1, -1, -1), (16, 17, 17, 17), (16, 18, 18, 18),
                                   (16, 18, 19, 18)]
    out.append(b.case("every_header_form", h, content_size=UNSIZED, window_size=1 << 20))
    return out


def _frame(blocks, fhd=0x20, tail=b""):
    """a single-segment frame of the given (header word, body) blocks with a 1-byte content size of 0"""
    out = bytearray(W.MAGIC) + bytes([fhd, 0])
    for h, body in blocks:
        out += h.to_bytes(3, "little") + body
    return bytes(out) + tail


def malformed_cases():
    """compressed blocks whose section headers do not fit into their body: (name, frame, per block (flags, lit_type, lit_regen,
    lit_comp, n_seq, modes))"""
    def c(size, last=1):
        return (size << 3) | (2 << 1) | last

    zero = (0, 0, 0)
    return [
        ("empty_compressed_block", _frame([(c(0), b"")]), [(LAST | MALFORMED, 0, 0, 0, 0, zero)]),
        ("huf_header_cut", _frame([(c(2), b"\x02\xff")]), [(LAST | MALFORMED, 0, 0, 0, 0, zero)]),
        ("raw_header_cut", _frame([(c(1), b"\x04")]), [(LAST | MALFORMED, 0, 0, 0, 0, zero)]),
        ("no_sequences_header", _frame([(c(4), b"\x18abc")]), [(LAST | MALFORMED, 0, 3, 3, 0, zero)]),
        ("literals_over_the_block", _frame([(c(4), b"\x20abc")]), [(LAST | MALFORMED, 0, 4, 4, 0, zero)]),
        ("count_cut", _frame([(c(2), b"\x00\x80")]), [(LAST | MALFORMED, 0, 0, 0, 0, zero)]),
        ("count3_cut", _frame([(c(3), b"\x00\xff\x01")]), [(LAST | MALFORMED, 0, 0, 0, 0, zero)]),
        ("modes_cut", _frame([(c(2), b"\x00\x05")]), [(LAST | MALFORMED, 0, 0, 0, 0, zero)]),
        # a malformed block defines nothing, a well-formed one behind it does
        ("malformed_defines_nothing", _frame([(c(2, 0), b"\x00\x05"), (c(3, 0), b"\x00\x05\x00"), (c(2), b"\x00\x00")]),
         [(MALFORMED, 0, 0, 0, 0, zero), (0, 0, 0, 0, 5, zero), (LAST, 0, 0, 0, 0, zero)]),
    ]


def three_block_frame():
    rnd = random.Random(421)
    b = Built(fcs=None, window=(0, 0), checksum=True)
    b.raw(rnd.randbytes(40)).compressed(_rb(rnd, 30), [(5, 20, N(30))]).rle(1, 9, last=True)
    return b.case("three_blocks", [(-1, -1, -1, -1)] * 2 + [(-1, 1, 1, 1)], content_size=UNSIZED, window_size=1024)


def verdict_files():
    """(name, buffer, status, n_blocks)"""
    three = three_block_frame().frame
    out = [("empty", b"", TRUNCATED, 0), ("three_bytes", W.MAGIC[:3], TRUNCATED, 0), ("no_magic", b"abcdefgh", BAD_HEADER, 0),
           ("skippable_in_front", W.skippable(b"abc") + three, BAD_HEADER, 0),
           ("reserved_block_type", _frame([(5 << 3, b"12345"), ((3 << 3) | (3 << 1) | 1, b"xyz")]), BAD_HEADER, 1),
           ("frames_behind", three + three, OK, 3)]
    return out


def block_cap_files():
    """2^20 empty raw blocks are followed to the end, one more is TOO_LARGE"""
    head = bytes(W.MAGIC) + bytes([0x20, 0])
    return [("cap", head + bytes(3) * (MAX_BLOCKS - 1) + b"\x01\0\0", OK, MAX_BLOCKS),
            ("cap_plus_1", head + bytes(3) * MAX_BLOCKS + b"\x01\0\0", TOO_LARGE, MAX_BLOCKS)]


@functools.lru_cache(maxsize=None)
def all_cases():
    return source_cases() + form_cases() + [three_block_frame()]


# ---- the second reading: the headers of a frame in plain Python (RFC 8878 3.1.1) ----
def py_blocks(data):
    """(rows, summary) as chip_zstd_blocks_host defines them; a row is (offset, size, lit_regen, lit_comp, n_seq, type, flags,
    lit_type, modes, src), the summary (n_blocks, in_used, content_size, window_size, status, descriptor, header_bytes)"""
    n = len(data)
    if n < 4:
        return [], (0, 0, UNSIZED, 0, TRUNCATED, 0, 0)
    if data[:4] != W.MAGIC:
        return [], (0, 0, UNSIZED, 0, BAD_HEADER, 0, 0)
    if n < 5:
        return [], (0, 0, UNSIZED, 0, TRUNCATED, 0, 0)
    fhd = data[4]
    single, fcs_bytes = (fhd >> 5) & 1, (0, 2, 4, 8)[fhd >> 6]
    if fhd >> 6 == 0:
        fcs_bytes = single
    at = 5 + (1 - single) + (0, 1, 2, 4)[fhd & 3]
    hs = at + fcs_bytes
    if n < hs:
        return [], (0, 0, UNSIZED, 0, TRUNCATED, fhd, 0)
    fcs = UNSIZED
    if fcs_bytes:
        fcs = int.from_bytes(data[at:at + fcs_bytes], "little") + (256 if fcs_bytes == 2 else 0)
    window = fcs if single else W.window_size(data[5] >> 3, data[5] & 7)
    rows, q, last_def = [], hs, [-1, -1, -1, -1]

    def stop(status):
        return rows, (len(rows), 0, fcs, window, status, fhd, hs)

    while True:
        if n - q < 3:
            return stop(TRUNCATED)
        h = int.from_bytes(data[q:q + 3], "little")
        btype, size = (h >> 1) & 3, h >> 3
        if btype == 3:
            return stop(BAD_HEADER)
        if len(rows) + 1 > MAX_BLOCKS:
            return stop(TOO_LARGE)
        body = 1 if btype == 1 else size
        if body > n - q - 3:
            return stop(TRUNCATED)
        flags, lit_type, regen, comp, nseq, modes = h & 1, 0, 0, 0, 0, (0, 0, 0)
        if btype == 2:
            flags, lit_type, regen, comp, nseq, modes = _py_sections(data[q + 3:q + 3 + size], flags)
        defines = [False] * 4
        if btype == 2 and not flags & MALFORMED:
            defines = [lit_type == 2] + [nseq > 0 and m != 3 for m in modes]
        rows.append((q, size, regen, comp, nseq, btype, flags, lit_type, modes, tuple(last_def)))
        for k in range(4):
            if defines[k]:
                last_def[k] = len(rows) - 1
        q += 3 + body
        if h & 1:
            break
    if fhd & 4:
        if n - q < 4:
            return stop(TRUNCATED)
        q += 4
    return rows, (len(rows), q, fcs, window, OK, fhd, hs)


def _py_sections(body, flags):
    bad = flags | MALFORMED
    if not body:
        return bad, 0, 0, 0, 0, (0, 0, 0)
    lt, sf = body[0] & 3, (body[0] >> 2) & 3
    if lt < 2:
        lh = {0: 1, 2: 1, 1: 2, 3: 3}[sf]
        if len(body) < lh:
            return bad, 0, 0, 0, 0, (0, 0, 0)
        regen = int.from_bytes(body[:lh], "little") >> (3 if lh == 1 else 4)
        comp = regen if lt == 0 else 1
    else:
        lh, bits = {0: (3, 10), 1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
        if len(body) < lh:
            return bad, 0, 0, 0, 0, (0, 0, 0)
        v = int.from_bytes(body[:lh], "little") >> 4
        regen, comp = v & ((1 << bits) - 1), (v >> bits) & ((1 << bits) - 1)
    seq = body[lh + comp:]
    if not seq:
        return bad, lt, regen, comp, 0, (0, 0, 0)
    if seq[0] < 128:
        nseq, sh = seq[0], 1
    elif seq[0] < 255:
        nseq, sh = ((seq[0] - 128) << 8) + (seq[1] if len(seq) > 1 else 0), 2
    else:
        nseq, sh = int.from_bytes(seq[1:3], "little") + 0x7F00, 3
    if len(seq) < sh or (nseq and len(seq) < sh + 1):
        return bad, lt, regen, comp, 0, (0, 0, 0)
    m = seq[sh] if nseq else 0
    return flags, lt, regen, comp, nseq, (m >> 6, (m >> 4) & 3, (m >> 2) & 3)
