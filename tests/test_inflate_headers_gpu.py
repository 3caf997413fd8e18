"""The block-header phase of the inflate kernels (compu_amd/csrc/inflate_unit.h): the code-length rounds of inflate_unit(), the
counting sort of canon_prep() and the sub-table fills of build_litlen() / build_dist().  Streams are built with
tests/deflate_writer.py; each aims at one shape of that code:

  * literal/length sub-tables of every size 2 .. 64 in one block (one of two sizes holds a prefix that straddles two lengths),
    tokens through the first and the last entry of each; 80 root prefixes with long codes (the second batch of 64 prefixes, a
    fill of 160 entries); a block with no long code at all;
  * distance sub-tables of the sizes 2, 4, 8 and 128 in one block whose code has all 30 symbols, and of 16, 32 and 64 in three
    more blocks of the same unit.  (Seven different sizes cannot stand in one distance code: canonical codes are handed out by
    rising length, so a root prefix whose longest code has L bits is followed by one that begins with at least L bits; prefixes
    that end with 9, 10, .., 15 bits then need at least 2 + 3 + 5 + 9 + 17 + 33 + 65 symbols.)  The block with no distance
    code and the block with one;
  * the sort: batches of 64 symbols that hold one length each; a batch with all 15 lengths (in both alphabets); symbol 285 with
    the longest length, once beside its twin in the first batch and once alone (a complete code has an even number of longest
    codes, so "alone" is an incomplete set: the oracle's verdict is an error); HLIT 257 and 286, HDIST 1 and 30;
  * the code-length sequence: a round of 64 one-bit symbols; a 14-bit symbol (18: 7 + 7 extra bits) over the end of each of the
    first three rounds; an 18 of 138 zeros from the literal/length lengths into the distance lengths (138 zeros across the seam
    take the end-of-block code with them: the oracle's verdict is "missing end-of-block"; the longest valid run over the seam,
    57 zeros, stands beside it); a 16 as the first symbol of a round; a sequence whose last symbol sits on the 64th position of
    its round; each of zlib's header errors with the offending symbol behind the first round where the error allows it ("repeat
    with no previous length" can only be the first symbol; a bad code-length code is found before any round); one header cut
    at every byte.

Bytes, out_len and status are oracle.inflate_units' at the same offsets and capacities, status and in_used the oracle decoder's, and
Python's zlib decodes every valid stream to the writer's content; the size pass names the oracle's length.  One unit of three
gzip members goes through CHIP_F_MEMBERS (tests/members_ref.py's walk over the oracle).  The first test needs no GPU: it pins,
from the writer's records, that each stream has the shape it was built for."""
import random
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_writer as W
import members_ref as R
from oracle import oracle as O

LIT_ROOT, DIST_ROOT = 9, 8  # root table bits (compu_amd/csrc/inflate_unit.h)
ROUND = 64                  # bit positions a code-length round covers
POISON = 0xA5
BAD = -3  # Z_DATA_ERROR
F_MEMBERS = 2
VALID, INVALID = "valid", "invalid"
Case = namedtuple("Case", "name body content kind blocks layout")


def _lens(n, **by_len):
    """code lengths of n symbols from l<bits>=[symbols]"""
    out = [0] * n
    for k, syms in by_len.items():
        for s in syms:
            assert out[s] == 0
            out[s] = int(k[1:])
    return out


def subtables(lens, root):
    """the root prefixes that hold codes of more than `root` bits, in code order: [(entries, lengths in it, its symbols in code order)]"""
    by = {}
    for s, (code, l) in W.canonical(lens).items():
        if l > root:
            by.setdefault(code >> (l - root), []).append((code << (15 - l), l, s))
    return [(1 << (max(l for _, l, _ in v) - root), sorted({l for _, l, _ in v}), [s for _, _, s in sorted(v)]) for _, v in sorted(by.items())]


def cl_rounds(info):
    """the rounds of the code-length loop over a dynamic block's sequence: a round takes every symbol that starts inside its 64 bit
    positions, the next one begins behind the last of them.  -> [[(offset in the round, bits, symbol, index in the sequence)]]"""
    cc = W.canonical(info["cl"])
    rounds, pos, r0 = [], 0, None
    for i, (s, _) in enumerate(info["cl_seq"]):
        n = cc[s][1] + W.CL_EXTRA.get(s, 0)
        if r0 is None or pos >= r0 + ROUND:
            r0 = pos
            rounds.append([])
        rounds[-1].append((pos - r0, n, s, i))
        pos += n
    return rounds


def _info(c, b=0):
    return [blk[3] for blk in c.blocks if len(blk) > 3][b]


def _explicit(lens):
    return [(l, 0) for l in lens]


def _cl(**by_sym):
    out = [0] * 19
    for k, l in by_sym.items():
        out[int(k[1:])] = l
    return out


# ---- literal/length sub-tables
# literals 65..70 of 1..6 bits, the end of the block 9 bits; 10 bits: 100, 101 (one prefix) and 102, which shares the next prefix
# with the 11-bit 103, 104; then whole prefixes of 4 / 8 / 16 / 32 / 64 codes of 11 / 12 / 13 / 14 / 15 bits
DEEP = {10: [100, 101, 102], 11: list(range(103, 109)), 12: list(range(110, 118)), 13: list(range(120, 136)), 14: list(range(140, 172)),
        15: list(range(180, 244))}
DEEP_LIT = _lens(257, l1=[65], l2=[66], l3=[67], l4=[68], l5=[69], l6=[70], l9=[256], **{f"l{b}": s for b, s in DEEP.items()})
# 160 literals of 10 bits: 80 root prefixes of two codes each; 26 literals and the end of the block 5 bits
WIDE_LIT = _lens(257, l10=list(range(160)), l5=list(range(160, 186)) + [256])
# nothing above the root: 253 literals of 8 bits, six symbols of 9
FLAT_LIT = _lens(259, l8=list(range(253)), l9=list(range(253, 259)))
# ---- distance sub-tables.  30 symbols: 22..29 short (1, 2, 3, 4, 6, 6, 7, 7 bits), 0..21 long: prefixes {9, 9}, {9, 10, 10},
# {10, 10, 10, 11, 11} and {11 x 7, 12, 13, 14, 15, 15}: sub-tables of 2, 4, 8 and 128 entries
DIST_A = [9, 9, 9, 10, 10, 10, 10, 10, 11, 11] + [11] * 7 + [12, 13, 14, 15, 15] + [1, 2, 3, 4, 6, 6, 7, 7]
# symbols 0..4+k long in one prefix that ends with two codes of 12 + k bits (16 << k entries), eight short ones of 1..8 bits behind
DIST_BCD = [list(range(9, 12 + k)) + [12 + k, 12 + k] + list(range(1, 9)) for k in range(3)]
# a few literals and length symbols 257 (3 bytes) .. 264 (10 bytes) for the blocks that are about distances
PLAIN_LIT = W.lengths_for({97: 9, 98: 9, 99: 9, 100: 9, 256: 2, **{s: 4 for s in range(257, 265)}}, 15, 265)
# ---- the sort
UNIFORM_LIT = [8] * 192 + [9] * 64 + [7] * 16          # batches of 64 symbols: 8, 8, 8, 9 bits, then sixteen of 7
UNIFORM_DIST = [4] * 16
L15 = list(range(1, 16)) + [15]                         # all 15 lengths in 16 neighbouring symbols
SPREAD_LIT = [0] * 256 + L15                            # the end of the block 1 bit, length symbols 257..271 2..15 bits
TWIN_LIT = _lens(286, l1=[97], l2=[256], l15=[0, 285], **{f"l{b}": [b - 2] for b in range(3, 15)})
ALONE_LIT = _lens(286, l1=[97], l2=[256], l15=[285])    # incomplete
# ---- the code-length sequence
CL_ONE_BIT = _cl(s8=1, s9=2, s0=3, s18=3)
LIT_8_9 = [8] * 255 + [9, 9]
CL_18_7BIT = _cl(s8=1, s0=2, s7=3, s9=4, s6=5, s10=6, s18=7, s17=7)
STRADDLE_LIT = ([8] * 52 + [0] * 11) * 3 + [7] * 10 + [8] * 80
SEAM_LIT, SEAM_DIST = [7] * 86 + [8] * 84 + [0] * 116, [0] * 22 + [3] * 8  # 116 + 22 = 138 zeros, no end-of-block code
SEAM_OK_LIT, SEAM_OK_DIST = LIT_8_9 + [0] * 29, [0] * 28 + [1, 1]          # 29 + 28 = 57 zeros
CL_ERR = _cl(s8=1, s9=3, s1=3, s16=3, s0=3)
for _l in (DEEP_LIT, WIDE_LIT, FLAT_LIT, DIST_A, *DIST_BCD, PLAIN_LIT, UNIFORM_LIT, UNIFORM_DIST, L15, SPREAD_LIT, TWIN_LIT, CL_ONE_BIT, LIT_8_9,
           CL_18_7BIT, STRADDLE_LIT, SEAM_DIST, SEAM_OK_LIT, SEAM_OK_DIST, CL_ERR):
    assert W.kraft(_l) == 32768, _l


def _zero_runs(lens, sym18_of):
    """explicit code-length symbols, every run of zeros in `sym18_of` {run length: extra} written as one 18"""
    seq, i = [], 0
    while i < len(lens):
        r = 0
        while i + r < len(lens) and lens[i + r] == 0:
            r += 1
        if r in sym18_of:
            seq.append((18, sym18_of[r]))
            i += r
        else:
            seq.append((lens[i], 0))
            i += 1
    return seq


def _last_position_lens():
    """literal/length lengths [8] * a + [9] + [8] * (255 - a) + [9] + [0] * z whose sequence (code-length code: 1 -> 1 bit, 8 -> 2,
    9, 0, 17 and 18 -> 4; distance lengths 1, 1) ends with a one-bit symbol on the 64th position of its round"""
    cl = _cl(s1=1, s8=2, s9=4, s0=4, s17=4, s18=4)
    for z in range(30):
        for a in range(256):
            lit = [8] * a + [9] + [8] * (255 - a) + [9] + [0] * z
            rounds = cl_rounds(dict(cl=cl, cl_seq=_explicit(lit + [1, 1])))
            if rounds[-1][-1][:2] == (ROUND - 1, 1):
                return cl, lit
    raise AssertionError("no such sequence")


def _dist_tokens(rnd, dist_lens):
    """a match through every long distance code (root prefixes in code order, first and last code of each first), between literals"""
    toks = []
    for _, _, syms in subtables(dist_lens, DIST_ROOT):
        for s in [syms[0], syms[-1]] + syms:
            toks += [("m", rnd.randrange(3, 11), W.DBASE[s] + rnd.randrange(0, 1 << W.DEXT[s])), rnd.randrange(97, 101)]
    return toks


def build_cases():
    rnd = random.Random(20261019)
    cases = []

    def add(name, d, kind=VALID):
        s = W.wrap(d)
        cases.append(Case(name, s.data, s.content, kind, s.blocks, s.layout))

    def lits(n, pool):
        return [rnd.choice(pool) for _ in range(n)]

    # -- literal/length sub-tables
    long_ = [s for b in DEEP for s in DEEP[b]]
    toks = []
    for _, _, syms in subtables(DEEP_LIT, LIT_ROOT):
        toks += [syms[0], syms[-1]] + lits(3, range(65, 71))
    toks += rnd.sample(long_, len(long_)) + lits(40, range(65, 71))
    add("sub_all_sizes", W.Deflate().dynamic(toks, DEEP_LIT, [0], final=True))
    toks = list(range(160)) + lits(60, range(160, 186))
    rnd.shuffle(toks)
    add("sub_80_prefixes", W.Deflate().dynamic(toks, WIDE_LIT, [0], final=True))
    add("sub_none", W.Deflate().dynamic(lits(200, range(256)), FLAT_LIT, [0], final=True))
    # -- distance sub-tables: 2100 stored bytes to reach back into, then the four blocks
    d = W.Deflate().stored(bytes(rnd.randrange(256) for _ in range(2100)))
    for k, dl in enumerate([DIST_A] + DIST_BCD):
        d.dynamic(_dist_tokens(rnd, dl), PLAIN_LIT, dl, final=k == 3)
    add("dist_sub_sizes", d)
    add("dist_none", W.Deflate().dynamic(lits(90, (97, 98, 99)), PLAIN_LIT, [0], final=True))
    add("dist_one_code", W.Deflate().dynamic([97, 98, ("m", 3, 1), 99, ("m", 10, 1), 98], PLAIN_LIT, [1], final=True))
    # -- the sort
    toks = lits(150, range(256)) + [("m", 3 + k % 8, 1 + k) for k in range(16)] + lits(20, range(256))
    add("sort_uniform_batches", W.Deflate().dynamic(toks, UNIFORM_LIT, UNIFORM_DIST, final=True))
    d = W.Deflate().stored(bytes(rnd.randrange(256) for _ in range(300)))
    toks = [("m", W.LBASE[s - 257], W.DBASE[ds] + (ds % 2 if W.DEXT[ds] else 0), s, ds) for s, ds in zip(range(257, 272), range(15))] * 2
    toks.append(("m", 5, 257, None, 15))  # distance symbol 15: 193 .. 256
    toks[-1] = ("m", 5, 200, None, 15)
    add("sort_15_lengths", d.dynamic(toks, SPREAD_LIT, L15, final=True))
    toks = [97] * 9 + [0, ("m", 258, 3, 285), 0, 97, ("m", 258, 1, 285)]
    add("sort_285_twin", W.Deflate().dynamic(toks, TWIN_LIT, W.lengths_for({0: 1, 2: 1}, 15, 30), final=True))
    add("sort_285_alone", W.Deflate().dynamic(None, ALONE_LIT, [1, 1], final=True).raw_bits(0, 32), kind=INVALID)
    # -- the code-length sequence
    add("cl_one_bit_round", W.Deflate().dynamic(lits(150, range(255)), LIT_8_9, [0], cl_lens=CL_ONE_BIT, cl_seq=_explicit(LIT_8_9 + [0]), final=True))
    used = [s for s, l in enumerate(STRADDLE_LIT) if l and s < 256]
    straddle = W.Deflate().dynamic(lits(150, used), STRADDLE_LIT, [0], cl_lens=CL_18_7BIT, cl_seq=_zero_runs(STRADDLE_LIT + [0], {11: 0}), final=True)
    add("cl_18_straddles", straddle)
    d = W.Deflate().dynamic(None, SEAM_LIT, SEAM_DIST, cl_seq=_zero_runs(SEAM_LIT + SEAM_DIST, {138: 127}), final=True)
    add("cl_18_of_138_over_seam", d.raw_bits(0, 32), kind=INVALID)
    add("cl_18_of_57_over_seam", W.Deflate().dynamic(lits(100, range(255)), SEAM_OK_LIT, SEAM_OK_DIST, cl_seq=_zero_runs(SEAM_OK_LIT + SEAM_OK_DIST, {57: 46}), final=True))
    seq = [(8, 0)] * 64 + [(16, 3)] + [(8, 0)] * (255 - 70) + [(9, 0), (9, 0), (0, 0)]
    assert W.expand_cl_seq(seq) == LIT_8_9 + [0]
    add("cl_16_first_of_round", W.Deflate().dynamic(lits(100, range(255)), LIT_8_9, [0], cl_lens=_cl(s8=1, s9=2, s16=3, s0=3), cl_seq=seq, final=True))
    cl, lit = _last_position_lens()
    add("cl_ends_on_last_position", W.Deflate().dynamic(lits(60, range(200)), lit, [1, 1], cl_lens=cl, cl_seq=_explicit(lit + [1, 1]), final=True))

    # -- zlib's header errors; the good header these are made from decodes (first case)
    def err(name, lit=LIT_8_9, dist=(1, 1), cl=CL_ERR, seq=None, kind=INVALID, toks=None):
        d = W.Deflate().dynamic(toks, lit, list(dist), cl_lens=cl, cl_seq=_explicit(list(lit) + list(dist)) if seq is None else seq, final=True)
        add(name, d if kind == VALID else d.raw_bits(0, 32), kind=kind)

    good = _explicit(LIT_8_9 + [1, 1])
    err("err_none", kind=VALID, toks=lits(50, range(255)))
    err("err_rep_first", seq=[(16, 0)] + good)
    err("err_rep16_past_end", seq=good[:-1] + [(16, 3)])
    # 64 lengths in the first round; the second: a 16 (6 more), an 18 of 138 zeros, and an 18 that runs past the 259
    err("err_rep18_past_end_round2", lit=[8] * 70 + [0] * 187, cl=_cl(s8=1, s16=2, s18=3, s0=3), seq=[(8, 0)] * 64 + [(16, 3), (18, 127), (18, 127)])
    over, inc = list(LIT_8_9), list(LIT_8_9)
    over[100], inc[100] = 1, 9
    err("err_lit_over", lit=over)
    err("err_lit_incomplete", lit=inc)
    err("err_dist_over", dist=(1, 1, 1))
    err("err_dist_incomplete", dist=(9, 9))
    err("err_cl_over", cl=_cl(s8=1, s9=1, s1=1, s16=3, s0=3))
    err("err_cl_incomplete", cl=_cl(s8=2, s9=3, s1=3, s16=3, s0=3))
    err("err_no_eob", lit=[8] * 256 + [0])
    return cases, W.wrap(straddle)


@pytest.fixture(scope="module")
def built():
    return build_cases()


@pytest.fixture(scope="module")
def cases(built):
    return built[0]


def _hdr_bytes(s):
    blk = [r for r in s.layout if r.kind == "block"][0]
    return (blk.bit + blk.nbits + 7) // 8


def _units(built):
    """(name, data, capacity, kind): every case as a raw unit, then one header cut at every byte of its length"""
    cases, s = built
    units = [(c.name, c.body, len(c.content) + 19, c.kind) for c in cases]
    units += [(f"cut_{k}", s.data[:k], len(s.content) + 19, "cut") for k in range(1, _hdr_bytes(s) + 1)]
    return units


def _pack(units):
    lens = np.array([len(u[1]) for u in units], dtype=np.int64)
    offs = np.zeros(len(units), dtype=np.int64)
    offs[1:] = np.cumsum((lens[:-1] + 7) & ~7)
    buf = np.zeros(int(offs[-1] + lens[-1]) + 8, dtype=np.uint8)
    for i, u in enumerate(units):
        buf[offs[i] : offs[i] + lens[i]] = np.frombuffer(u[1], dtype=np.uint8)
    caps = np.array([u[2] for u in units], dtype=np.int64)
    ooff = np.zeros(len(units), dtype=np.int64)
    ooff[1:] = np.cumsum((caps[:-1] + 15 + 16) & ~15)
    ooff += 16
    return (buf, offs, lens), (ooff, caps, int(ooff[-1] + caps[-1]) + 32)


_ORACLE = {}


def _oracle(built):
    """units, packed input, output layout, the oracle's output, lengths and statuses, the oracle decoder's verdicts; computed
    once, shared, read-only"""
    if "raw" not in _ORACLE:
        units = _units(built)
        packed, layout = _pack(units)
        ooff, caps, total = layout
        out = np.full(total, POISON, dtype=np.uint8)
        out, out_len, status, _ = O.inflate_units(O.MODE_DEFLATE, *packed, total, ooff, caps, out=out)
        verdicts = []
        for _, data, cap, _ in units:
            got, ir, _, st, e = O.InflateDecoder(O.MODE_DEFLATE).decode(data, int(cap))
            verdicts.append((got, len(data) - ir, e if e else st))
        for a in (out, out_len, status):
            a.setflags(write=False)
        _ORACLE["raw"] = (units, packed, layout, out, out_len, status, verdicts)
    return _ORACLE["raw"]


def _members_unit(cases):
    by = {c.name: c for c in cases}
    pick = [by[n] for n in ("sub_all_sizes", "dist_sub_sizes", "cl_18_straddles")]
    return b"".join(W.gzip_header() + c.body + W.gzip_trailer(c.content) for c in pick), b"".join(c.content for c in pick)


def test_streams_have_the_shape_they_were_built_for(built, cases):
    """no GPU: one assertion per shape, from the writer's records; zlib and the oracle agree on every case"""
    by = {c.name: c for c in cases}
    assert len(by) == len(cases)
    units, _, (ooff, caps, _), out, out_len, status, verdicts = _oracle(built)
    assert len(units) <= 128
    for i, (name, data, cap, kind) in enumerate(units):
        got, used, st = verdicts[i]
        where = (name, st, used, len(data))
        assert len(data) <= 4096 and cap <= 8192, where
        assert bytes(out[ooff[i] : ooff[i] + out_len[i]]) == got and int(status[i]) == st, where
        if kind == VALID:
            z = zlib.decompressobj(-15)
            assert z.decompress(data) == by[name].content == got and z.eof and st == O.FINISHED and used == len(data), where
        elif kind == INVALID:
            assert st == BAD, where
            with pytest.raises(zlib.error):
                zlib.decompressobj(-15).decompress(data)
        else:
            assert st == O.NEED_INPUT and used == len(data) and got == b"", where

    def syms_used(c, b=0):
        return {r.sym for r in c.layout if r.kind in ("lit", "match") and r.block == b}

    # literal/length sub-tables: sizes 2 .. 64, one prefix with two lengths, the first and last code of every prefix decoded
    c = by["sub_all_sizes"]
    tabs = subtables(_info(c)["lit"], LIT_ROOT)
    assert [t[0] for t in tabs] == [2, 4, 4, 8, 16, 32, 64] and [t[1] for t in tabs][1] == [10, 11] and all(len(t[1]) == 1 for t in tabs[2:])
    assert all({t[2][0], t[2][-1]} <= syms_used(c) for t in tabs) and tabs[1][2][0] == 102
    tabs = subtables(_info(by["sub_80_prefixes"])["lit"], LIT_ROOT)
    assert len(tabs) == 80 > 64 and sum(t[0] for t in tabs) == 160 > 128 and set(range(160)) <= syms_used(by["sub_80_prefixes"])
    assert subtables(_info(by["sub_none"])["lit"], LIT_ROOT) == [] and max(_info(by["sub_none"])["lit"]) == LIT_ROOT
    # distance sub-tables: 2, 4, 8, 128 beside 30 symbols; 16, 32, 64; every long code in a match
    c = by["dist_sub_sizes"]
    sizes = [[t[0] for t in subtables(_info(c, b)["dist"], DIST_ROOT)] for b in range(4)]
    assert sizes == [[2, 4, 8, 128], [16], [32], [64]] and len(_info(c, 0)["dist"]) == 30 and all(_info(c, 0)["dist"])
    for b in range(4):
        long_ = {s for t in subtables(_info(c, b)["dist"], DIST_ROOT) for s in t[2]}
        assert long_ <= {r.dsym for r in c.layout if r.kind == "match" and r.block == b + 1}
    assert _info(by["dist_none"])["dist"] == [0] and _info(by["dist_one_code"])["dist"] == [1]
    assert any(r.kind == "match" for r in by["dist_one_code"].layout)
    # the sort
    lit = _info(by["sort_uniform_batches"])["lit"]
    assert [sorted(set(lit[k : k + 64])) for k in range(0, len(lit), 64)] == [[8], [8], [8], [9], [7]]
    assert len(set(_info(by["sort_uniform_batches"])["dist"])) == 1
    i15 = _info(by["sort_15_lengths"])
    assert set(i15["lit"][256:320]) == set(range(1, 16)) and set(i15["dist"]) == set(range(1, 16))
    assert syms_used(by["sort_15_lengths"], 1) == set(range(257, 272))
    for name, n in (("sort_285_twin", 2), ("sort_285_alone", 1)):
        lit = _info(by[name])["lit"]
        assert lit[285] == max(lit) == 15 and lit.count(15) == n and len(lit) == 286
    assert 285 in syms_used(by["sort_285_twin"]) and W.kraft(_info(by["sort_285_alone"])["lit"]) < 32768
    hlits = {len(_info(c, b)["lit"]) for c in cases for b in range(sum(1 for x in c.blocks if len(x) > 3))}
    hdists = {len(_info(c, b)["dist"]) for c in cases for b in range(sum(1 for x in c.blocks if len(x) > 3))}
    assert {257, 286} <= hlits and {1, 30} <= hdists
    # the code-length sequence
    rounds = cl_rounds(_info(by["cl_one_bit_round"]))
    assert [x[:2] for x in rounds[0]] == [(k, 1) for k in range(64)] and len(rounds[1]) == 64
    rounds = cl_rounds(_info(by["cl_18_straddles"]))
    for r in rounds[:3]:
        off, n, s, _ = r[-1]
        assert s == 18 and n == 14 and off < ROUND < off + n, r[-1]
    for name, zeros, nlit in (("cl_18_of_138_over_seam", 138, 286), ("cl_18_of_57_over_seam", 57, 286)):
        info = _info(by[name])
        (i, (s, x)), = [(i, e) for i, e in enumerate(info["cl_seq"]) if e[0] == 18]
        first = len(W.expand_cl_seq(info["cl_seq"][:i]))
        assert 11 + x == zeros and first < nlit < first + zeros and len(info["lit"]) == nlit
    assert _info(by["cl_18_of_138_over_seam"])["lit"][256] == 0
    rounds = cl_rounds(_info(by["cl_16_first_of_round"]))
    assert rounds[1][0][2] == 16 and rounds[1][0][0] == 0 and rounds[0][-1][2] == 8
    rounds = cl_rounds(_info(by["cl_ends_on_last_position"]))
    assert rounds[-1][-1][:2] == (ROUND - 1, 1) and rounds[-1][-1][3] == len(_info(by["cl_ends_on_last_position"])["cl_seq"]) - 1

    def round_of(name, i):
        return [k for k, r in enumerate(cl_rounds(_info(by[name]))) if any(x[3] == i for x in r)][0]

    assert _info(by["err_rep_first"])["cl_seq"][0][0] == 16
    for name in ("err_rep16_past_end", "err_rep18_past_end_round2"):
        seq = _info(by[name])["cl_seq"]
        total = len(_info(by[name])["lit"]) + len(_info(by[name])["dist"])
        bad = [i for i in range(len(seq)) if seq[i][0] >= 16 and len(W.expand_cl_seq(seq[: i + 1])) > total][0]
        assert round_of(name, bad) >= 1 and len(W.expand_cl_seq(seq[:bad])) < total, name
    assert round_of("err_rep18_past_end_round2", 66) == 1
    for name, k in (("err_lit_over", 32768 + 16384 - 128), ("err_lit_incomplete", 32768 - 64)):
        assert W.kraft(_info(by[name])["lit"]) == k and round_of(name, 100) == 1, name
    assert W.kraft(_info(by["err_dist_over"])["dist"]) > 32768 > W.kraft(_info(by["err_dist_incomplete"])["dist"])
    assert W.kraft(_info(by["err_cl_over"])["cl"]) > 32768 > W.kraft(_info(by["err_cl_incomplete"])["cl"])
    assert _info(by["err_no_eob"])["lit"][256] == 0 and W.kraft(_info(by["err_no_eob"])["lit"]) == 32768
    # the cut header: every byte of it, and the whole header is not a cut
    s = built[1]
    cuts = [u for u in units if u[3] == "cut"]
    assert len(cuts) == _hdr_bytes(s) >= 40 and len(cuts[-1][1]) == _hdr_bytes(s) < len(s.data)
    # the members unit: three members, the walk over the oracle finishes with all their content
    unit, content = _members_unit(cases)
    a = R.walk(R.GZIP, unit, len(content) + 19)
    assert a.status == R.FINISHED and a.members == 3 and a.data == content and a.in_used == len(unit)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "compu_status"])
def test_units_match_the_oracle(gpu, built, flagged):
    import compu_amd

    units, (buf, offs, lens), (ooff, caps, total), r_out, r_len, r_st, verdicts = _oracle(built)
    d_out = gpu.full((total,), POISON, dtype=gpu.uint8, device="cuda:0")
    out_len, in_used, status = compu_amd.decode_batch(O.MODE_DEFLATE, _dev(gpu, buf), _dev(gpu, offs), _dev(gpu, lens.astype(np.int32)), d_out, _dev(gpu, ooff),
                                                      _dev(gpu, caps.astype(np.int32)), flags=compu_amd.F_COMPU_STATUS if flagged else 0)
    gpu.cuda.synchronize()
    g_out, g_len, g_used, g_st = d_out.cpu().numpy(), out_len.cpu().numpy(), in_used.cpu().numpy(), status.cpu().numpy()
    keep = np.ones(len(g_out), dtype=bool)
    for i, (name, data, cap, kind) in enumerate(units):
        _, used, st = verdicts[i]
        where = (name, flagged, int(g_st[i]), st, int(g_used[i]), used, int(g_len[i]), int(r_len[i]))
        assert int(g_st[i]) == st == int(r_st[i]), where
        assert int(g_len[i]) == int(r_len[i]), where
        lo, hi = int(ooff[i]), int(ooff[i]) + int(r_len[i])
        assert np.array_equal(g_out[lo:hi], r_out[lo:hi]), where
        keep[lo:hi] = False
        if st in (O.FINISHED, O.NEED_INPUT):
            assert int(g_used[i]) == used, where
    assert (g_out[keep] == POISON).all(), np.flatnonzero(g_out[keep] != POISON)[:8]


@pytest.mark.gpu
def test_size_pass_names_the_oracle_length(gpu, built):
    import compu_amd

    units, (buf, offs, lens), _, _, r_len, r_st, verdicts = _oracle(built)
    size, used, st = compu_amd.decode_batch_sizes(O.MODE_DEFLATE, _dev(gpu, buf), _dev(gpu, offs), _dev(gpu, lens.astype(np.int32)))
    gpu.cuda.synchronize()
    size, used, st = size.cpu().numpy(), used.cpu().numpy(), st.cpu().numpy()
    for i, (name, _, _, _) in enumerate(units):
        assert int(st[i]) == int(r_st[i]) and int(size[i]) == int(r_len[i]), (name, int(size[i]), int(r_len[i]), int(st[i]), int(r_st[i]))
        if int(r_st[i]) in (O.FINISHED, O.NEED_INPUT):
            assert int(used[i]) == verdicts[i][1], (name, int(used[i]), verdicts[i][1])


@pytest.mark.gpu
def test_members_unit(gpu, cases):
    """three gzip members as one unit under CHIP_F_MEMBERS, decode and size pass"""
    import compu_amd

    unit, content = _members_unit(cases)
    cap = len(content) + 19
    a = R.walk(R.GZIP, unit, cap)
    (buf, offs, lens), (ooff, caps, total) = _pack([("members", unit, cap, VALID)])
    d_out = gpu.full((total,), POISON, dtype=gpu.uint8, device="cuda:0")
    out_len, in_used, status = compu_amd.decode_batch(R.GZIP, _dev(gpu, buf), _dev(gpu, offs), _dev(gpu, lens.astype(np.int32)), d_out, _dev(gpu, ooff),
                                                      _dev(gpu, caps.astype(np.int32)), flags=F_MEMBERS)
    size, used, st = compu_amd.decode_batch_sizes(R.GZIP, _dev(gpu, buf), _dev(gpu, offs), _dev(gpu, lens.astype(np.int32)), flags=F_MEMBERS)
    gpu.cuda.synchronize()
    g = d_out.cpu().numpy()
    assert (int(status[0]), int(out_len[0]), int(in_used[0])) == (a.status, a.out_len, a.in_used) == (R.FINISHED, len(content), len(unit))
    assert bytes(g[int(ooff[0]) : int(ooff[0]) + len(content)]) == a.data == content
    assert (g[: int(ooff[0])] == POISON).all() and (g[int(ooff[0]) + len(content) :] == POISON).all()
    assert (int(st[0]), int(size[0]), int(used[0])) == (R.FINISHED, len(content), len(unit))
