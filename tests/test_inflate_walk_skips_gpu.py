"""Wave-uniform skips in the inflate walk's step (compu_amd/csrc/inflate_unit.h, walk_round's `token`).  The sub-table read of a
distance code of more than 8 bits runs only in a step in which some lane has one; the pair's mark bit, which is always 0 for a
second code that starts inside the lane's own segment, is still read in every step (a skip of that read was built and measured
slower, profiles/walk_skips_ab.md), and the cases that would break such a skip stay here for whoever tries it again.  No skip
changes a decision, so every unit below must come out as the CPU oracle decodes it.  Streams are built with
tests/deflate_writer.py; each is the smallest shape that breaks one skip:

  * distance codes: a block whose used distances all have codes of 9-15 bits (a long code in every step), one with codes of at
    most 8 bits only (in none), and one with a single long code per 320 bits of input (the region runs with one live lane); each
    spans more than three super-rounds (64 segments of 320 bits);
  * all-literal blocks of more than two super-rounds: 3 000 literals of 15 bits, 9 000 of 4-6 bits;
  * literal runs behind matches placed so that a pair starts exactly at, one code before and one code after every segment
    boundary of the first super-round, dynamic and fixed Huffman (the two have different chain limits), with the block's first
    bit at every position of a byte behind a stored block;
  * a literal whose would-be partner is the end-of-block code, an invalid code, or a code cut by the input's end;
  * a length code whose distance code is invalid, or cut by the input's end (short and long distance codes).

Bytes, out_len and status are oracle.inflate_units' at the same offsets and capacities; status and in_used the oracle decoder's;
the size pass names the oracle's length.  Every launch has at most 64 units of at most 64 KiB.  The first test needs no GPU: it
pins, from the writer's layout records, that each stream has the shape it was built for, and what the oracle and zlib say."""
import random
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_writer as W
from oracle import oracle as O

S_BITS = 320  # the walk's segment (CHIP_S_BITS); a super-round is 64 of them
ROUND_BITS = 64 * S_BITS
POISON = 0xA5
BAD = -3  # Z_DATA_ERROR
VALID, INVALID, CUT = "valid", "invalid", "cut"
Case = namedtuple("Case", "name body content kind")

# distance code lengths: symbols 0..7 have 1..8 bits, symbols 8..15 (distances 17..256) 9, 10, ... 14, 15, 15 bits: complete
DIST_LENS = list(range(1, 9)) + [9, 10, 11, 12, 13, 14, 15, 15]
# literals 97..112 5 bits, 113..119 and the end of the block 6 bits, length symbols 257 (3 bytes) 3 bits, 258 and 260 4 bits,
# literal 120 3 bits: complete
LIT_LENS = [0] * 261
for _s in range(97, 113):
    LIT_LENS[_s] = 5
for _s in range(113, 120):
    LIT_LENS[_s] = 6
LIT_LENS[120], LIT_LENS[256], LIT_LENS[257], LIT_LENS[258], LIT_LENS[260] = 3, 6, 3, 4, 4
# end of block 1 bit, thirteen unused literals of 2..14 bits, two literals of 15 bits (as tests/test_inflate_pairs_gpu.py)
LONG_LITS = [200, 201]
LONG_LENS = [0] * 257
LONG_LENS[256] = 1
for _i in range(13):
    LONG_LENS[_i] = 2 + _i
LONG_LENS[200] = LONG_LENS[201] = 15
SHORT_LITS = list(range(97, 97 + 27))
SHORT_LENS = [0] * 257
for _i, _s in enumerate(SHORT_LITS):
    SHORT_LENS[_s] = 4 if _i < 8 else 5 if _i < 20 else 6
SHORT_LENS[256] = 6
assert all(W.kraft(l) == 32768 for l in (DIST_LENS, LIT_LENS, LONG_LENS, SHORT_LENS))


def _shifted(shift):
    """a stored block (the next block starts on a byte), then non-final fixed blocks: empty ones take 10 bits, one with a 9-bit
    literal 19 -- (2 a + 3 b) mod 8 reaches every bit position"""
    d = W.Deflate().stored(b"stored in front")
    a, b = {0: (0, 0), 1: (0, 3), 2: (1, 0), 3: (0, 1), 4: (2, 0), 5: (1, 1), 6: (3, 0), 7: (2, 1)}[shift]
    for _ in range(a):
        d.fixed([])
    for _ in range(b):
        d.fixed([200])
    return d


def _boundary_tokens(rnd, by_len, match, match_bits, nseg):
    """Tokens of one block in which, for k = 1 .. nseg - 1, a run of six literals behind a match starts at k * S_BITS + delta
    bits behind the block's first token, delta = 0, -c, +c in turn (c = the run's code length): the run's first literal starts a
    pair.  by_len = {code length: literals} with two neighbouring lengths c, c + 1; everything between two runs is literals."""
    c = min(by_len)
    toks, pos, starts = [], 0, []

    def lits(n_bits):  # literals of c and c + 1 bits that take exactly n_bits
        nonlocal pos
        b = n_bits % c
        a = (n_bits - (c + 1) * b) // c
        assert a >= 0 and a * c + b * (c + 1) == n_bits, n_bits
        lens = [c] * a + [c + 1] * b
        rnd.shuffle(lens)
        toks.extend(rnd.choice(by_len[l]) for l in lens)
        pos += n_bits

    lits(8 * c)  # something to copy from
    for k in range(1, nseg):
        target = k * S_BITS + (0, -c, c)[k % 3]
        lits(target - match_bits - pos)
        toks.append(match)
        pos += match_bits
        starts.append(pos)
        lits(6 * c)
    return toks, starts


def build_cases():
    rnd = random.Random(20260214)
    cases = []

    def add(name, d, kind=VALID, content=None, body=None):
        cases.append(Case(name, d.body() if body is None else body, bytes(d.content) if content is None else content, kind))

    # -- distance codes of more than 8 bits: in every step, in none, one per 320 bits (each more than three super-rounds)
    head = [rnd.randrange(97, 121) for _ in range(300)]
    toks = list(head)
    for _ in range(3600):  # length code 3-4 bits, distance code 9-15 bits, 3-6 extra bits
        toks.append(("m", rnd.choice((3, 4, 6)), rnd.randrange(17, 257)))
    add("dist_long_all", W.Deflate().dynamic(toks, lit_lens=LIT_LENS, dist_lens=DIST_LENS, final=True))
    toks = list(head)
    for _ in range(5000):  # distance codes of 1-8 bits (distances 1..16)
        toks += [rnd.randrange(97, 121), ("m", rnd.choice((3, 4, 6)), rnd.randrange(1, 17))]
    add("dist_short_only", W.Deflate().dynamic(toks, lit_lens=LIT_LENS, dist_lens=DIST_LENS, final=True))
    toks = list(head)
    for _ in range(220):  # 30 pairs of a 5-bit literal and a 3 + 1-bit match, then one match with a 13-bit code: about 320 bits
        for _ in range(30):
            toks += [rnd.randrange(97, 113), ("m", 3, 1)]
        toks.append(("m", 4, rnd.randrange(65, 97)))
    add("dist_long_sparse", W.Deflate().dynamic(toks, lit_lens=LIT_LENS, dist_lens=DIST_LENS, final=True))
    # -- all-literal blocks of more than two super-rounds
    add("lits_long_3000", W.Deflate().dynamic([rnd.choice(LONG_LITS) for _ in range(3000)], lit_lens=LONG_LENS, dist_lens=[0], final=True))
    add("lits_short_9000", W.Deflate().dynamic([rnd.choice(SHORT_LITS) for _ in range(9000)], lit_lens=SHORT_LENS, dist_lens=[0], final=True))
    # -- pairs that start at, one code before and one code after every segment boundary; the block's first bit at every position
    dyn = {5: list(range(97, 113)), 6: list(range(113, 120))}
    fix = {8: list(range(97, 144)), 9: list(range(144, 200))}
    for shift in range(8):
        toks, _ = _boundary_tokens(rnd, dyn, ("m", 3, 2), 3 + 2, 2 * 64 + 9)
        add(f"bound_dynamic_{shift}", _shifted(shift).dynamic(toks, lit_lens=LIT_LENS, dist_lens=DIST_LENS, final=True))
        toks, _ = _boundary_tokens(rnd, fix, ("m", 3, 2), 7 + 5, 2 * 64 + 9)
        add(f"bound_fixed_{shift}", _shifted(shift).fixed(toks, final=True))
    # -- a literal's would-be partner: the end of the block, an invalid code, a code cut by the input's end
    for n in (1, 2, 3, 4):
        add(f"second_eob_{n}", W.Deflate().dynamic([97 + k for k in range(n)], lit_lens=LIT_LENS, dist_lens=DIST_LENS, final=True))
        add(f"second_eob_fixed_{n}", W.Deflate().fixed([97 + k for k in range(n)], final=True))
        for bad in (286, 287):
            add(f"second_invalid_{n}_{bad}", W.Deflate().fixed([97 + k for k in range(n)] + [("s", bad)], final=True, eob=False).raw_bits(0, 16), kind=INVALID)
    for shift in (0, 3, 5):
        d = _shifted(shift).dynamic([rnd.choice(LONG_LITS) for _ in range(3)], lit_lens=LONG_LENS, dist_lens=[0], final=True)
        body = d.body()
        for n in range(len(body) - 6, len(body)):  # the cut falls inside the second and the third literal's 15 bits
            add(f"second_cut_{shift}_{n}", d, kind=CUT, body=body[:n])
    # -- a length code whose distance code is invalid (the fixed code's 30 and 31) or cut by the input's end
    for n in (0, 1, 2):
        for bad in (30, 31):
            d = W.Deflate().fixed([97] * 4 + [98 + k for k in range(n)] + [("s", 257), ("d", bad)], final=True, eob=False).raw_bits(0, 16)
            add(f"dist_invalid_{n}_{bad}", d, kind=INVALID)
    for name, dist in (("short", 3), ("long", 200)):
        d = W.Deflate().dynamic(head + [("m", 4, dist)], lit_lens=LIT_LENS, dist_lens=DIST_LENS, final=True)
        body = d.body()
        for n in range(len(body) - 3, len(body)):
            add(f"dist_cut_{name}_{n}", d, kind=CUT, body=body[:n])
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


def _batches(units):
    return [units[i : i + 64] for i in range(0, len(units), 64)]


_ORACLE = {}


def _oracle(fmt, mis, cases):
    """per (format, misalignment): [(units, packed input, output layout, oracle output, lengths, statuses, decoder verdicts)] of
    the batches of at most 64 units; computed once, shared, read-only"""
    if (fmt, mis) not in _ORACLE:
        res = []
        for units in _batches(_units(cases, fmt)):
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
            res.append((units, (buf, offs, lens), (ooff, caps, total), out, out_len, status, verdicts))
        _ORACLE[(fmt, mis)] = res
    return _ORACLE[(fmt, mis)]


def test_streams_have_the_shape_they_were_built_for(cases):
    """no GPU: the geometry each case aims at, read from the writer's layout records, and the oracle's and zlib's verdicts"""
    by = {c.name: c for c in cases}
    assert len(by) == len(cases)
    for c in cases:
        assert len(c.content) + 19 <= 65536 and len(c.body) <= 65536, c.name
        if c.kind == VALID:
            z = zlib.decompressobj(-15)
            assert z.decompress(c.body) == c.content and z.eof and z.unused_data == b"", c.name
    for batch in _oracle(O.MODE_DEFLATE, 0, cases):
        units, _, (ooff, caps, _), out, out_len, status, verdicts = batch
        assert len(units) <= 64
        for i, (c, data, cap) in enumerate(units):
            got, used, st = verdicts[i]
            where = (c.name, st, used, len(data))
            assert bytes(out[ooff[i] : ooff[i] + out_len[i]]) == got and int(status[i]) == st, where
            if c.kind == VALID:
                assert st == O.FINISHED and got == c.content and used == len(data), where
            elif c.kind == INVALID:
                assert st == BAD and got == c.content, where
            else:
                assert st == O.NEED_INPUT and used == len(data) and c.content.startswith(got), where
    # the distance cases: more than three super-rounds of input, long codes where they were meant to be
    rnd = random.Random(20260214)
    dc = W.canonical(DIST_LENS)
    for name in ("dist_long_all", "dist_short_only", "dist_long_sparse"):
        assert 8 * len(by[name].body) >= 3 * ROUND_BITS, name
    assert all(dc[W.dist_sym(d)][1] >= 9 for d in range(17, 257)) and all(dc[W.dist_sym(d)][1] <= 8 for d in range(1, 17))
    assert dc[W.dist_sym(65)][1] == dc[W.dist_sym(96)][1] == 13
    # (one period of the sparse case: 30 * (5 + 3 + 1) bits, then 4 + 13 + 5)
    assert abs(30 * 9 + 22 - S_BITS) <= 32
    assert 8 * len(by["lits_long_3000"].body) >= 2 * ROUND_BITS and 8 * len(by["lits_short_9000"].body) >= 2 * ROUND_BITS
    # the boundary cases: behind a match, a literal starts at k * 320 + (0, -c, +c) bits behind the block's first token
    for codes, lens, c, fixed in (({5: [97], 6: [113]}, LIT_LENS, 5, False), ({8: [97], 9: [144]}, W.FIXED_LIT, 8, True)):
        toks, starts = _boundary_tokens(rnd, codes, ("m", 3, 2), 12 if fixed else 5, 2 * 64 + 9)
        d = _shifted(5)
        d.fixed(toks, final=True) if fixed else d.dynamic(toks, lit_lens=LIT_LENS, dist_lens=DIST_LENS, final=True)
        recs = [r for r in d.layout if r.block == len(d.blocks) - 1 and r.kind in ("lit", "match")]
        first = recs[0].bit
        behind = [b.bit - first for a, b in zip(recs, recs[1:]) if a.kind == "match"]
        assert behind == starts and len(starts) == 2 * 64 + 8
        assert [s - k * S_BITS for k, s in enumerate(starts, 1)] == [(0, -c, c)[k % 3] for k in range(1, len(starts) + 1)]
        assert all(b.kind == "lit" and b.nbits == c for a, b in zip(recs, recs[1:]) if a.kind == "match")
        assert d.blocks[-1][0] % 8 == 5  # (the block's first bit is at position 5 of a byte)


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

    for units, packed, layout, r_out, r_len, r_st, verdicts in _oracle(fmt, mis, cases):
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
    for units, (buf, offs, lens), _, _, r_len, r_st, _ in _oracle(fmt, 0, cases):
        size, _, st = compu_amd.decode_batch_sizes(fmt, gpu.from_numpy(buf).to(dev), gpu.from_numpy(offs).to(dev), gpu.from_numpy(lens.astype(np.int32)).to(dev))
        gpu.cuda.synchronize()
        size, st = size.cpu().numpy(), st.cpu().numpy()
        for i, (c, _, _) in enumerate(units):
            assert int(size[i]) == int(r_len[i]) and int(st[i]) == int(r_st[i]), (c.name, int(size[i]), int(r_len[i]), int(st[i]), int(r_st[i]))
