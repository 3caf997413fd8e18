"""The inflate walk's step (compu_amd/csrc/inflate_unit.h, walk_round's `token`) forms the two table indices of a token's first
code from bits the step before left in a register (the low 16 bits of the 64 it held, shifted by that token's length), and issues
the reads for a pair's second literal beside the distance root's, in front of the branch that skips the long-distance-code
region.  Neither changes a decision, so every unit below must come out as the CPU oracle decodes it.  Streams are built with
tests/deflate_writer.py; each aims at one edge of the two:

  * tokens of exactly 48 bits (length code 15 + 5 extra bits, distance code 15 + 13 extra bits) in runs: the carried bits are the
    top 16 of the 64, again and again; an invalid code met as a first code from carried bits, behind the longest token of the one
    block type that can hold such a code (fixed Huffman: 31 bits);
  * pairs of two 15-bit literals;
  * first codes of 10 to 15 bits whose sub-tables have 1 to 6 index bits (all 15 carried index bits used);
  * a block of 1-bit and 2-bit literal codes;
  * first literals of every length 3 to 9, each behind a match (so that it is a step's first code) and in front of a literal, a
    length code and the end-of-block code;
  * pairs whose second literal starts exactly on a segment boundary, which the next segment's owner marked;
  * a stream whose last code ends 1, 8, 15 and 16 bits before the input's end, and one cut inside its last code;
  * long distance codes (9 bits and more) and literal pairs side by side: other lanes pair in the step that takes the region.

Bytes, out_len and status are oracle.inflate_units' at the same offsets and capacities; status and in_used the oracle decoder's;
the size pass names the oracle's length.  One launch of fewer than 64 units of at most 64 KiB per format.  The first test needs
no GPU: it pins, from the writer's layout records, that each stream has the shape it was built for."""
import random
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_writer as W
from oracle import oracle as O

S_BITS = 320  # the walk's segment (CHIP_S_BITS)
POISON = 0xA5
BAD = -3  # Z_DATA_ERROR
VALID, INVALID, CUT, PADDED = "valid", "invalid", "cut", "padded"
Case = namedtuple("Case", "name body content kind layout")


def _lens(n, **by_len):
    """code lengths of n symbols from l<bits>=[symbols]"""
    out = [0] * n
    for k, syms in by_len.items():
        for s in syms:
            assert out[s] == 0
            out[s] = int(k[1:])
    return out


# 48-bit tokens: literal 97 1 bit, length 258 (symbol 285) 2 bits, end of block 3 bits, one unused literal of each length
# 4..14, length symbols 281 and 284 (5 extra bits) 15 bits
T48_LIT = _lens(286, l1=[97], l2=[285], l3=[256], l15=[281, 284], **{f"l{b}": [b - 4] for b in range(4, 15)})
# distance 1 one bit, one unused symbol of each length 2..14, symbols 28 and 29 (13 extra bits) 15 bits
T48_DIST = _lens(30, l1=[0], l15=[28, 29], **{f"l{b}": [b - 1] for b in range(2, 15)})
# two 15-bit literals, the end of the block 1 bit, one unused literal of each length 2..14
L15_LITS = [200, 201]
L15_LIT = _lens(257, l1=[256], l15=L15_LITS, **{f"l{b}": [b - 2] for b in range(2, 15)})
# literals of 1..6 bits (65..70), the end of the block 8 bits, then 2 / 4 / 8 / 16 / 32 / 64 literals of 10 / 11 / ... / 15 bits:
# each group fills one 9-bit prefix, whose sub-table has 1 / 2 / ... / 6 index bits
DEEP = {10: list(range(100, 102)), 11: list(range(102, 106)), 12: list(range(106, 114)), 13: list(range(114, 130)),
        14: list(range(130, 162)), 15: list(range(162, 226))}
DEEP_LIT = _lens(257, l1=[65], l2=[66], l3=[67], l4=[68], l5=[69], l6=[70], l8=[256], **{f"l{b}": s for b, s in DEEP.items()})
# one literal of each length 3..9 (99..105 = 'c'..'i'), length symbol 257 2 bits, end of block 4 bits, literals 65..68 of 2, 3, 4, 9 bits
G_FIRST = {b: 96 + b for b in range(3, 10)}
G_LIT = _lens(258, l2=[257, 65], l3=[66, G_FIRST[3]], l4=[256, 67, G_FIRST[4]], l9=[68, G_FIRST[9]], **{f"l{b}": [G_FIRST[b]] for b in range(5, 9)})
# (tests/test_inflate_walk_skips_gpu.py's tables) distance symbols 0..7 1..8 bits, 8..15 (distances 17..256) 9..15, 15 bits;
# literals 97..112 5 bits, 113..119 and the end of the block 6, 120 3 bits, length symbols 257 3 bits, 258 and 260 4 bits
DIST_LENS = list(range(1, 9)) + [9, 10, 11, 12, 13, 14, 15, 15]
MIX_LIT = _lens(261, l5=list(range(97, 113)), l6=list(range(113, 120)) + [256], l3=[120, 257], l4=[258, 260])
assert all(W.kraft(l) == 32768 for l in (T48_LIT, T48_DIST, L15_LIT, DEEP_LIT, G_LIT, DIST_LENS, MIX_LIT))


def _tok48(rnd, n):
    """a literal and 64 matches of 258 bytes at distance 1 (16 513 bytes to reach back into), then n matches of 48 bits"""
    toks, have = [97] + [("m", 258, 1)] * 64, 1 + 64 * 258
    for _ in range(n):
        length = rnd.randrange(227, 258) if rnd.random() < 0.1 else rnd.randrange(131, 163)  # symbols 284, 281
        dist = rnd.randrange(16385, min(have, 32768) + 1)
        toks.append(("m", length, dist))
        have += length
    return toks


def _boundary_pairs(rnd, nseg):
    """MIX_LIT tokens in which, for k = 1 .. nseg - 1, a match (3 + 2 bits) ends 5 bits in front of bit k * S_BITS behind the
    block's first token and two 5-bit literals follow: the second starts exactly on the boundary.  -> tokens, those starts"""
    toks, pos, starts = [], 0, []

    def lits(n_bits):  # literals of 5 and 6 bits that take exactly n_bits
        nonlocal pos
        b = n_bits % 5
        a = (n_bits - 6 * b) // 5
        assert a >= 0 and 5 * a + 6 * b == n_bits, n_bits
        ls = [5] * a + [6] * b
        rnd.shuffle(ls)
        toks.extend(rnd.randrange(97, 113) if l == 5 else rnd.randrange(113, 120) for l in ls)
        pos += n_bits

    lits(40)
    for k in range(1, nseg):
        lits(k * S_BITS - 5 - 5 - pos)
        toks.append(("m", 3, 2))
        toks += [rnd.randrange(97, 113) for _ in range(4)]
        pos += 5 + 20
        starts.append(pos - 15)
    return toks, starts


def _stored_then(shift):
    """a stored block, then `shift` empty non-final fixed blocks of 10 bits: the next block starts at bit 2 * shift of a byte"""
    d = W.Deflate().stored(b"in front")
    for _ in range(shift):
        d.fixed([])
    return d


def build_cases():
    rnd = random.Random(20261019)
    cases = []

    def add(name, d, kind=VALID, body=None):
        cases.append(Case(name, d.body() if body is None else body, bytes(d.content), kind, list(d.layout)))

    # -- 48-bit tokens in a run; the same with a few literals between (the run's phase against the dwords moves), and ending in
    #    an invalid code instead of the end of the block
    add("tok48_run", W.Deflate().dynamic(_tok48(rnd, 280), lit_lens=T48_LIT, dist_lens=T48_DIST, final=True))
    toks = _tok48(rnd, 200)
    for k in range(70, len(toks), 9):
        toks.insert(k, 97)
    add("tok48_lits", W.Deflate().dynamic(toks, lit_lens=T48_LIT, dist_lens=T48_DIST, final=True))
    # (no dynamic block can hold an invalid literal/length code: zlib refuses a header that names symbol 286 or leaves the code
    # incomplete before it reads a token.  The invalid code therefore stands in a fixed block, behind that block's longest token:
    # 8 + 5 + 5 + 13 = 31 bits.)
    add("tok31_invalid", W.Deflate().fixed(_tok48(rnd, 150) + [("s", 286)], final=True, eob=False).raw_bits(0, 16), kind=INVALID)
    # -- pairs of 15 + 15 bits
    add("pair_15_15", W.Deflate().dynamic([rnd.choice(L15_LITS) for _ in range(700)], lit_lens=L15_LIT, dist_lens=[0], final=True))
    # -- first codes of 10..15 bits, sub-tables of 1..6 index bits, between literals of 1..6 bits
    toks = []
    for _ in range(150):
        b = rnd.randrange(10, 16)
        toks += [rnd.choice(DEEP[b])] + [rnd.randrange(65, 71) for _ in range(rnd.randrange(0, 3))]
    toks += [s for b in DEEP for s in DEEP[b]]  # every long code once
    add("first_10_15", W.Deflate().dynamic(toks, lit_lens=DEEP_LIT, dist_lens=[0], final=True))
    # -- 1-bit and 2-bit literal codes
    add("lits_1_2", W.Deflate().dynamic([rnd.choice((65, 65, 66)) for _ in range(4000)], lit_lens=DEEP_LIT, dist_lens=[0], final=True))
    # -- first literals of 3..9 bits behind a match, in front of a literal / a length code / the end of the block: one block per length
    d = W.Deflate()
    for b in range(3, 10):
        f = G_FIRST[b]
        toks = [65, 66, 67, 68] * (50 if b == 3 else 1)  # (the first block's matches reach back up to 199 bytes)
        for _ in range(12):
            toks += [("m", 3, rnd.randrange(1, 5)), f, rnd.choice((65, 66, 67, 68, f))]        # ... a literal
            toks += [("m", 3, rnd.randrange(1, 5)), f, ("m", 3, rnd.randrange(1, 200))]         # ... a length code
            toks += [rnd.choice((65, 66, 67)) for _ in range(rnd.randrange(0, 4))]
        toks += [("m", 3, 1), f]                                                                   # ... the end of the block
        d.dynamic(toks, lit_lens=G_LIT, dist_lens=DIST_LENS, final=b == 9)
    add("first_3_9", d)
    # -- a pair's second literal on a boundary the next segment's owner marked; the block's first bit at even positions of a byte
    for shift in (0, 1, 3):
        toks, _ = _boundary_pairs(rnd, 64 + 9)
        add(f"pair_on_boundary_{shift}", _stored_then(shift).dynamic(toks, lit_lens=MIX_LIT, dist_lens=DIST_LENS, final=True))
    # -- the last code (the end of the block, 6 bits) ends k bits before the input's end; a cut inside the last code (15 bits)
    for k in (1, 8, 15, 16):
        toks = [rnd.randrange(97, 120) for _ in range(300)]
        while True:
            d = W.Deflate().dynamic(toks, lit_lens=MIX_LIT, dist_lens=DIST_LENS, final=True)
            if (d.w.n + k) % 8 == 0:
                break
            toks.append(rnd.randrange(97, 113))
        add(f"end_pad_{k}", d.raw_bits(0, k), kind=PADDED)
    d = W.Deflate().dynamic([rnd.choice(L15_LITS) for _ in range(301)], lit_lens=L15_LIT, dist_lens=[0], final=True, eob=False)
    body = d.body()
    add("end_cut_inside", d, kind=CUT, body=body[:-1])
    # -- long distance codes and literal pairs side by side
    toks = [rnd.randrange(97, 121) for _ in range(300)]
    for _ in range(500):
        if rnd.random() < 0.5:
            toks.append(("m", rnd.choice((3, 4, 6)), rnd.randrange(17, 257)))
        else:
            toks += [rnd.randrange(97, 121) for _ in range(rnd.randrange(2, 7))]
    add("dist_long_beside_pairs", W.Deflate().dynamic(toks, lit_lens=MIX_LIT, dist_lens=DIST_LENS, final=True))
    return cases


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def _units(cases, fmt):
    units = []
    for c in cases:
        data = c.body if fmt == O.MODE_DEFLATE else W.gzip_header() + c.body + (W.gzip_trailer(c.content) if c.kind == VALID else b"")
        units.append((c, data, len(c.content) + 19))
    return units


def _layout(units, mis):
    caps = np.array([u[2] for u in units], dtype=np.int64)
    ooff = np.zeros(len(units), dtype=np.int64)
    ooff[1:] = np.cumsum((caps[:-1] + 15 + 16) & ~15)
    ooff += 16 + mis
    return ooff, caps, int(ooff[-1] + caps[-1]) + 32


def _pack(units):
    lens = np.array([len(u[1]) for u in units], dtype=np.int64)
    offs = np.zeros(len(units), dtype=np.int64)
    offs[1:] = np.cumsum((lens[:-1] + 7) & ~7)
    buf = np.zeros(int(offs[-1] + lens[-1]) + 8, dtype=np.uint8)
    for i, u in enumerate(units):
        buf[offs[i] : offs[i] + lens[i]] = np.frombuffer(u[1], dtype=np.uint8)
    return buf, offs, lens


_ORACLE = {}


def _oracle(fmt, mis, cases):
    """per (format, misalignment): units, packed input, output layout, oracle output, lengths, statuses, decoder verdicts;
    computed once, shared, read-only"""
    if (fmt, mis) not in _ORACLE:
        units = _units(cases, fmt)
        assert len(units) <= 64
        buf, offs, lens = _pack(units)
        ooff, caps, total = _layout(units, mis)
        out = np.full(total, POISON, dtype=np.uint8)
        out, out_len, status, _ = O.inflate_units(fmt, buf, offs, lens, total, ooff, caps, out=out)
        verdicts = []
        for _, data, cap in units:
            got, ir, _, st, err = O.InflateDecoder(fmt).decode(data, int(cap))
            verdicts.append((got, len(data) - ir, err if err else st))
        for a in (out, out_len, status):
            a.setflags(write=False)
        _ORACLE[(fmt, mis)] = (units, (buf, offs, lens), (ooff, caps, total), out, out_len, status, verdicts)
    return _ORACLE[(fmt, mis)]


def _toks(c, block=None):
    return [r for r in c.layout if r.kind in ("lit", "match", "sym", "eob") and (block is None or r.block == block)]


def test_streams_have_the_shape_they_were_built_for(cases):
    """no GPU: token bit lengths and code lengths of each case, read from the writer's layout records; the oracle's verdicts"""
    by = {c.name: c for c in cases}
    assert len(by) == len(cases)
    for c in cases:
        assert len(c.content) + 19 <= 65536 and len(c.body) <= 8192, (c.name, len(c.content), len(c.body))
        assert len(_toks(c)) >= 150, (c.name, len(_toks(c)))
        assert 8 * len(c.body) >= 4 * S_BITS  # several segments: chains cross boundaries and join
        if c.kind in (VALID, PADDED):
            z = zlib.decompressobj(-15)
            assert z.decompress(c.body) == c.content and z.eof, c.name
            assert len(z.unused_data) == (int(c.name[8:]) // 8 if c.kind == PADDED else 0), c.name
    units, _, (ooff, caps, _), out, out_len, status, verdicts = _oracle(O.MODE_DEFLATE, 0, cases)
    for i, (c, data, cap) in enumerate(units):
        got, used, st = verdicts[i]
        where = (c.name, st, used, len(data))
        assert bytes(out[ooff[i] : ooff[i] + out_len[i]]) == got and int(status[i]) == st, where
        if c.kind in (VALID, PADDED):
            assert st == O.FINISHED and got == c.content, where
        elif c.kind == INVALID:
            assert st == BAD and got == c.content, where
        else:
            assert st == O.NEED_INPUT and used == len(data) and c.content.startswith(got), where
    # 48-bit tokens: at least 150 in a row, both 15-bit length codes and both 15-bit distance codes; the invalid code behind one
    lc, dc = W.canonical(T48_LIT), W.canonical(T48_DIST)
    assert lc[281][1] == lc[284][1] == dc[28][1] == dc[29][1] == 15 and W.LEXT[281 - 257] == W.LEXT[284 - 257] == 5 and W.DEXT[28] == W.DEXT[29] == 13
    for name in ("tok48_run", "tok48_lits"):
        recs = _toks(by[name])
        long_ = [r for r in recs if r.kind == "match" and r.nbits == 48]
        assert len(long_) >= 150 and {r.sym for r in long_} == {281, 284} and {r.dsym for r in long_} == {28, 29}, name
        assert max(r.nbits for r in recs) == 48
    recs = _toks(by["tok48_run"])
    assert all(r.nbits == 48 for r in recs[65:-1]) and recs[-1].kind == "eob"
    recs = _toks(by["tok31_invalid"])
    assert recs[-1].kind == "sym" and recs[-1].sym == 286 and recs[-1].nbits == 8 and all(r.nbits == 31 for r in recs[65:-1]) and len(recs) == 216
    assert sum(1 for a, b in zip(_toks(by["tok48_lits"]), _toks(by["tok48_lits"])[1:]) if a.nbits == 48 and b.kind == "lit") >= 15
    # 15 + 15
    assert all(r.nbits == 15 for r in _toks(by["pair_15_15"])[:-1]) and len(_toks(by["pair_15_15"])) == 701
    # first codes of 10..15 bits: every length, every symbol of every group; the groups fill whole 9-bit prefixes
    cc = W.canonical(DEEP_LIT)
    for b, syms in DEEP.items():
        assert len(syms) == 1 << (b - 9) and len({cc[s][0] >> (b - 9) for s in syms}) == 1 and all(cc[s][1] == b for s in syms)
    recs = _toks(by["first_10_15"])
    assert {r.sym for r in recs if r.kind == "lit" and r.nbits >= 10} == {s for b in DEEP for s in DEEP[b]}
    assert {r.nbits for r in recs if r.kind == "lit"} == set(range(1, 7)) | set(range(10, 16))
    assert {r.nbits for r in _toks(by["lits_1_2"])[:-1]} == {1, 2}
    # first literals of 3..9 bits: behind a match, in front of a literal, a length code and the end of the block
    c = by["first_3_9"]
    for b in range(3, 10):
        recs = _toks(c, block=b - 3)
        seen = set()
        for x, y, z_ in zip(recs, recs[1:], recs[2:]):
            if x.kind == "match" and y.kind == "lit" and y.sym == G_FIRST[b]:
                assert y.nbits == b
                seen.add(z_.kind)
        assert seen == {"lit", "match", "eob"}, (b, seen)
    # the pairs on a boundary: behind a match, two 5-bit literals, the second k * 320 bits behind the block's first token
    for shift in (0, 1, 3):
        c = by[f"pair_on_boundary_{shift}"]
        recs = _toks(c, block=1 + shift)
        first = recs[0].bit
        hits = [z_.bit - first for x, y, z_ in zip(recs, recs[1:], recs[2:]) if x.kind == "match" and y.kind == z_.kind == "lit" and y.nbits == z_.nbits == 5]
        assert hits == [k * S_BITS for k in range(1, 64 + 9)], shift
    assert len({_toks(by[f"pair_on_boundary_{s}"], block=1 + s)[0].bit % 8 for s in (0, 1, 3)}) == 3
    # the padded ends: the end-of-block code ends k bits before the input's end; the cut falls inside the last code
    for k in (1, 8, 15, 16):
        c = by[f"end_pad_{k}"]
        last = _toks(c)[-1]
        assert last.kind == "eob" and 8 * len(c.body) - (last.bit + last.nbits) == k
    c = by["end_cut_inside"]
    last = _toks(c)[-1]
    assert last.kind == "lit" and last.nbits == 15 and last.bit < 8 * len(c.body) < last.bit + last.nbits
    # long distance codes beside pairs: matches with 9..15-bit distance codes, and runs of literals between them
    dc = W.canonical(DIST_LENS)
    recs = _toks(by["dist_long_beside_pairs"])
    assert sum(1 for r in recs if r.kind == "match" and dc[r.dsym][1] >= 9) >= 200
    assert sum(1 for a, b in zip(recs, recs[1:]) if a.kind == b.kind == "lit") >= 500


def _run_gpu(torch, fmt, packed, layout, flags):
    import compu_amd

    buf, offs, lens = packed
    ooff, caps, total = layout
    dev = "cuda:0"
    d_out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    out_len, in_used, status = compu_amd.decode_batch(
        fmt, torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), d_out,
        torch.from_numpy(ooff).to(dev), torch.from_numpy(caps.astype(np.int32)).to(dev), flags=flags)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_len.cpu().numpy(), in_used.cpu().numpy(), status.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [O.MODE_DEFLATE, O.MODE_GZIP], ids=["raw", "gzip"])
@pytest.mark.parametrize("mis", [0, 3])
def test_units_match_the_oracle(gpu, cases, fmt, mis):
    import compu_amd

    units, packed, layout, r_out, r_len, r_st, verdicts = _oracle(fmt, mis, cases)
    ooff = layout[0]
    for flags in (compu_amd.F_COMPU_STATUS, 0):
        g_out, g_len, g_used, g_st = _run_gpu(gpu, fmt, packed, layout, flags)
        keep = np.ones(len(g_out), dtype=bool)
        for i, (c, data, cap) in enumerate(units):
            _, used, st = verdicts[i]
            where = (c.name, mis, flags, int(g_st[i]), st, int(g_used[i]), used, int(g_len[i]), int(r_len[i]))
            assert int(g_len[i]) == int(r_len[i]), where
            lo, hi = int(ooff[i]), int(ooff[i]) + int(r_len[i])
            assert np.array_equal(g_out[lo:hi], r_out[lo:hi]), where
            keep[lo:hi] = False
            assert int(g_st[i]) == st == int(r_st[i]), where
            # in_used is zlib's count for these verdicts (without the flag: for a finished unit and one that wants input)
            if st in (O.FINISHED, O.NEED_INPUT):
                assert int(g_used[i]) == used, where
        assert (g_out[keep] == POISON).all(), (mis, flags, np.flatnonzero(g_out[keep] != POISON)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [O.MODE_DEFLATE, O.MODE_GZIP], ids=["raw", "gzip"])
def test_size_pass_names_the_oracle_length(gpu, cases, fmt):
    """the size pass shares the walk: its length and status are the oracle's at ample capacity"""
    import compu_amd

    dev = "cuda:0"
    units, (buf, offs, lens), _, _, r_len, r_st, _ = _oracle(fmt, 0, cases)
    size, _, st = compu_amd.decode_batch_sizes(fmt, gpu.from_numpy(buf).to(dev), gpu.from_numpy(offs).to(dev), gpu.from_numpy(lens.astype(np.int32)).to(dev))
    gpu.cuda.synchronize()
    size, st = size.cpu().numpy(), st.cpu().numpy()
    for i, (c, _, _) in enumerate(units):
        assert int(size[i]) == int(r_len[i]) and int(st[i]) == int(r_st[i]), (c.name, int(size[i]), int(r_len[i]), int(st[i]), int(r_st[i]))
