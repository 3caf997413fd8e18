"""The steady loop of the inflate executor (flush_tokens in compu_amd/csrc/inflate_unit.h) where it hands a group over to the
general code and takes the stream back: raw DEFLATE units built by hand (tests/deflate_writer.py), decoded with
compu_amd.decode_batch and compared with zlib.decompressobj(-15) for the bytes, out_len, in_used and status, with the unit's
first output byte at each of the four alignments modulo 4.

How the cases reach the places they aim at.  A token of the executor is a match, a literal, or two literals that the walk has
paired; a literal in front of a match is never paired, so a stream of matches behind one literal (or of literals and matches in
turn) has as many tokens as it has codes.  A unit of one small dynamic block is one super-round, that is one batch of
flush_tokens, and the batch's groups are its tokens 64 by 64; every batch begins an empty chunk, at image offset (address of the
unit's next byte) % 4.  Where literals follow each other the pairing is the walk's own business: such cases come at both parities
of the place they aim at.

  * batch end: 64 k - 1, 64 k, 64 k + 1 tokens for k = 1 and 4 (the last group left short, exact, or one token over);
  * chunk fill: the second group ends one byte short of CHUNK_BYTES, exactly there, and one byte over (the whole group goes to the
    next chunk); a run of literals across the edge, at both parities (a pair whose second byte does not fit), behind a group and
    inside the first group of an empty chunk;
  * a group of 64 matches of length 258 into an empty chunk (a block of its own: its batch begins the chunk), small groups behind;
  * ten groups of 64 short matches each (a round at every trip, the queue wraps), ten and more groups of literals and then a match;
  * 40 KiB of mixed tokens with a distance of exactly 32 768 just behind 32 768 bytes of output and again a chunk later;
  * a distance one byte too far in the middle of the second group: Z_DATA_ERROR behind the bytes in front of it, and
    CHIP_NEED_OUTPUT when the output is exactly full there;
  * capacity that ends at a literal, at either byte of a literal pair and inside a match of a full group.

The first test needs no GPU: it pins what zlib alone says about every case."""
import random
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_writer as W

CHUNK_BYTES = 2560  # output of one executor chunk (CHIP_CHUNK_BYTES)
POISON = 0xA5
NEED_INPUT, NEED_OUTPUT, FINISHED, DATA_ERROR = 0, 1, 2, -3  # CHIP_NEED_INPUT, CHIP_NEED_OUTPUT, CHIP_FINISHED, Z_DATA_ERROR
RAW = -15

# far_at: the output position of a match whose distance reaches one byte in front of the output (None: the stream is valid)
# caps: capacities to run the unit at (None = room for everything and a little more)
Case = namedtuple("Case", "name body content far_at caps")


def _lits(rnd, n):
    return [rnd.randrange(97, 123) for _ in range(n)]


def _matches(rnd, pos, lengths, near=False):
    """one match per length, each from anywhere in the `pos` bytes in front of it (near: from the last 40, so that sources overlap
    the matches of the same round); -> tokens, new position"""
    toks = []
    for ln in lengths:
        toks.append(("m", ln, rnd.randrange(1, min(pos, 40 if near else 32768) + 1)))
        pos += ln
    return toks, pos


def _lengths(rnd, n, total):
    """n match lengths (3..258) that sum to `total`"""
    assert 3 * n <= total <= 258 * n
    out = [3] * n
    left = total - 3 * n
    while left:
        i = rnd.randrange(n)
        add = min(left, 258 - out[i], rnd.randrange(1, 60))
        out[i] += add
        left -= add
    return out


def _dyn(tokens):
    d = W.Deflate().dynamic(tokens, final=True, ndist=2)  # (a lone distance symbol gets its twin at symbol + 1)
    return d.body(), bytes(d.content)


def _mixed(rnd, n_out, force=()):
    """literals and matches giving exactly n_out bytes; `force`: (position, distance) of matches of length 7 to place at the first
    token boundary at or behind the position; -> tokens, where those matches begin"""
    toks, pos, force, at = [], 0, list(force), []
    while pos < n_out:
        room = n_out - pos
        if force and pos >= force[0][0] and room >= 7:
            toks.append(("m", 7, force.pop(0)[1]))
            at.append(pos)
            pos += 7
        elif pos >= 1 and room >= 3 and rnd.random() < 0.35:
            ln = min(room, rnd.choice([3, 3, 4, 5, 6, 8, 11, 16, 17, 31, 32, 33, 64, 100, 258]))
            dist = rnd.randrange(1, min(pos, 32768) + 1) if rnd.random() < 0.7 else rnd.randrange(1, min(pos, 40) + 1)
            toks.append(("m", ln, dist))
            pos += ln
        else:
            toks.append(rnd.randrange(97, 123))
            pos += 1
    assert not force
    return toks, at


def build_cases(mis):
    """the cases for units whose first output byte lies at an address = mis (mod 4): the chunk's first byte is at image offset mis"""
    rnd = random.Random(20250917 + mis)
    cases = []
    room = CHUNK_BYTES - mis  # bytes the unit's first chunk takes

    def add(name, body, content, far_at=None, caps=(None,)):
        cases.append(Case(name, body, content, far_at, tuple(caps)))

    # -- the batch ends at a group boundary, one token short of it, one token behind it
    for k in (1, 4):
        for n in (64 * k - 1, 64 * k, 64 * k + 1):
            toks, _ = _matches(rnd, 1, [rnd.choice((3, 4, 9, 20)) for _ in range(n - 1)])
            add(f"end_matches_{n}", *_dyn([97] + toks))
            toks, pos = [], 0
            for i in range(n):  # a literal and a match in turn: no two literals meet
                if i % 2 == 0:
                    toks.append(rnd.randrange(97, 123))
                    pos += 1
                else:
                    t, pos = _matches(rnd, pos, [rnd.choice((3, 5, 17))])
                    toks += t
            add(f"end_turns_{n}", *_dyn(toks))
    # -- the chunk fills at the edge: group 0 gives 190 bytes, group 1 ends at the chunk's last byte + delta, two more groups follow
    for delta in (-1, 0, 1):
        g0, pos = _matches(rnd, 1, [3] * 63)
        g1, pos = _matches(rnd, pos, _lengths(rnd, 64, room + delta - pos))
        assert pos == room + delta
        rest, pos = _matches(rnd, pos, [rnd.choice((3, 4, 30)) for _ in range(130)])
        add(f"edge_group_{delta:+d}", *_dyn([97] + g0 + g1 + rest))
    #    a run of 120 literals across the edge, behind a group of matches (p, p + 1: whichever way the walk pairs them, in one of the
    #    two a pair lies across the chunk's last byte)
    for par in (0, 1):
        g0, pos = _matches(rnd, 1, [3] * 63)
        g1, pos = _matches(rnd, pos, _lengths(rnd, 40, room - 61 + par - pos))
        rest, _ = _matches(rnd, pos + 120, [3] * 80)
        add(f"edge_pair_{par}", *_dyn([97] + g0 + g1 + _lits(rnd, 120) + rest))
        # the same inside the first group of the batch: the chunk is empty, the group is taken up to the token that does not fit
        g0, pos = _matches(rnd, 1, _lengths(rnd, 10, room - 41 + par - 1))
        rest, _ = _matches(rnd, pos + 104, [3] * 80)
        add(f"edge_pair_first_{par}", *_dyn([97] + g0 + _lits(rnd, 104) + rest))
    # -- 64 matches of length 258 into an empty chunk: a block of its own, so that its batch begins with them; small groups behind
    d = W.Deflate().dynamic(_lits(rnd, 300), ndist=2)
    g, pos = _matches(rnd, 300, [258] * 64)
    rest, _ = _matches(rnd, pos, [rnd.choice((3, 4, 5)) for _ in range(64 * 5 + 7)])
    d.dynamic(g + rest, final=True, ndist=2)
    add("group_258", d.body(), bytes(d.content))
    g, pos = _matches(rnd, 1, [258] * 63)
    rest, _ = _matches(rnd, pos, [3] * 200)
    add("group_258_first", *_dyn([97] + g + rest))
    # -- groups of matches only: a round is due at every trip, the queue wraps
    toks, _ = _matches(rnd, 40, [rnd.choice((3, 4, 5, 8)) for _ in range(64 * 10 + 5)])
    add("all_matches", *_dyn(_lits(rnd, 40) + toks))
    toks, _ = _matches(rnd, 40, [rnd.choice((3, 4, 5, 8, 17, 33)) for _ in range(64 * 10 + 5)], near=True)
    add("all_matches_near", *_dyn(_lits(rnd, 40) + toks))
    # -- groups of literals only (at two to a token 1 500 literals are at least eleven groups), then one match
    add("all_literals", *_dyn(_lits(rnd, 1500) + [("m", 10, 700)] + _lits(rnd, 3)))
    # -- the distance test is dropped once 32 KiB of output exist: distances of exactly 32 768 just behind that and a chunk later
    toks, at = _mixed(rnd, 40960, force=((32768, 32768), (32768 + CHUNK_BYTES, 32768), (36000, 32768)))
    assert all(p <= a < p + 258 for p, a in zip((32768, 32768 + CHUNK_BYTES, 36000), at))
    add("switch_32k", *_dyn(toks))
    # -- a distance one byte too far in the middle of the second group; capacity: room to spare, and exactly full at that token
    head, pos = _matches(rnd, 1, [3] * (64 + 31))
    tail, _ = _matches(rnd, pos + 3, [3] * 100)
    body, content = _dyn([97] + head + [("m", 3, pos + 1)] + tail)
    add("too_far", body, content, far_at=pos, caps=(None, pos + 1, pos))
    # -- the capacity ends inside a full group: at a literal between matches, at either byte of a literal pair, inside a match
    head, pos = _matches(rnd, 1, [rnd.choice((3, 6, 40)) for _ in range(64 + 20)])
    caps = [pos, pos + 1]  # (in front of / behind the single literal)
    mid, pos2 = _matches(rnd, pos + 1, [5] * 3)
    caps += [pos2 + 10, pos2 + 11, pos2 + 12]  # (in a run of 30 literals)
    tail, pos3 = _matches(rnd, pos2 + 30, [100, 3, 258])
    caps += [pos2 + 30 + 1, pos2 + 30 + 50, pos2 + 30 + 99, pos2 + 30 + 100, pos3 - 1]
    rest, _ = _matches(rnd, pos3, [3] * 60)
    add("capacity", *_dyn([97] + head + [98] + mid + _lits(rnd, 30) + tail + rest), caps=[None] + caps)
    return cases


@pytest.fixture(scope="module")
def cases():
    return {mis: build_cases(mis) for mis in range(4)}


def _units(cases):
    """-> [(case, capacity)]"""
    return [(c, len(c.content) + 19 if cap is None else cap) for c in cases for cap in c.caps]


def zlib_verdict(c, cap):
    """what zlib makes of the unit in `cap` bytes of room: (bytes, in_used or None where zlib gives none, status)"""
    d = zlib.decompressobj(RAW)
    if c.far_at is not None and cap > c.far_at:
        got = d.decompress(c.body, c.far_at) if c.far_at else b""  # the bytes in front of the match ...
        with pytest.raises(zlib.error, match="invalid distance too far back"):
            d.decompress(d.unconsumed_tail, cap - c.far_at)  # ... and what inflate() says once there is room for its first byte
        return got, None, DATA_ERROR
    got = d.decompress(c.body, cap)
    if d.eof:
        return got, len(c.body) - len(d.unused_data), FINISHED
    assert len(got) == cap
    return got, len(c.body) - len(d.unconsumed_tail), NEED_OUTPUT


def test_zlib_verdicts(cases):
    """no GPU: zlib says about every case what the case was built for"""
    for mis in range(4):
        names = [c.name for c in cases[mis]]
        assert len(set(names)) == len(names) and len(names) == 27
        for c, cap in _units(cases[mis]):
            got, used, st = zlib_verdict(c, cap)
            where = (c.name, mis, cap, st, used)
            assert len(c.content) <= 65536 and len(c.body) <= 65536, where
            if c.far_at is not None:
                assert (st, got) == ((DATA_ERROR, c.content[: c.far_at]) if cap > c.far_at else (NEED_OUTPUT, c.content[:cap])), where
            elif cap > len(c.content):
                assert st == FINISHED and got == c.content and used == len(c.body), where
            else:
                assert st == NEED_OUTPUT and got == c.content[:cap] and 0 < used <= len(c.body), where
        by = {c.name: c for c in cases[mis]}
        assert 300 + 64 * 258 < len(by["group_258"].content) < 300 + 64 * 258 + 5 * 327
        assert len(by["switch_32k"].content) == 40960
        assert len(by["too_far"].caps) == 3 and len(by["capacity"].caps) == 11


def _layout(units, mis):
    caps = np.array([u[1] for u in units], dtype=np.int64)
    ooff = np.zeros(len(units), dtype=np.int64)
    ooff[1:] = np.cumsum((caps[:-1] + 15 + 16) & ~15)
    ooff += 16 + mis  # every unit's first byte at an address = mis (mod 4); poison in front of the first as well
    return ooff, caps, int(ooff[-1] + caps[-1]) + 32


def _pack(units):
    lens = np.array([len(u[0].body) for u in units], dtype=np.int64)
    offs = np.zeros(len(units), dtype=np.int64)
    offs[1:] = np.cumsum((lens[:-1] + 7) & ~7)
    buf = np.zeros(int(offs[-1] + lens[-1]) + 8, dtype=np.uint8)
    for i, u in enumerate(units):
        buf[offs[i] : offs[i] + lens[i]] = np.frombuffer(u[0].body, dtype=np.uint8)
    return buf, offs, lens


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_steady_loop_matches_zlib(gpu, cases, mis):
    import compu_amd

    torch = gpu
    units = _units(cases[mis])
    verdicts = [zlib_verdict(c, cap) for c, cap in units]
    buf, offs, lens = _pack(units)
    ooff, caps, total = _layout(units, mis)
    dev = "cuda:0"
    for flags in (compu_amd.F_COMPU_STATUS, 0):
        d_out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
        out_len, in_used, status = compu_amd.decode_batch(
            RAW, torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), d_out,
            torch.from_numpy(ooff).to(dev), torch.from_numpy(caps.astype(np.int32)).to(dev), flags=flags)
        torch.cuda.synchronize()
        g_out, g_len, g_used, g_st = d_out.cpu().numpy(), out_len.cpu().numpy(), in_used.cpu().numpy(), status.cpu().numpy()
        keep = np.ones(len(g_out), dtype=bool)
        for i, (c, cap) in enumerate(units):
            got, used, st = verdicts[i]
            where = (c.name, mis, flags, cap, int(g_st[i]), st, int(g_used[i]), used, int(g_len[i]), len(got))
            assert int(g_len[i]) == len(got), where
            lo, hi = int(ooff[i]), int(ooff[i]) + len(got)
            assert bytes(g_out[lo:hi]) == got, where
            keep[lo:hi] = False
            assert int(g_st[i]) == st, where  # (no unit here has its output exactly full with all its input read)
            if st == NEED_OUTPUT:
                assert int(g_len[i]) == cap, where
            # in_used is zlib's count for a finished unit, and with CHIP_F_COMPU_STATUS for one that ran out of room as well
            if st == FINISHED or (st == NEED_OUTPUT and flags & compu_amd.F_COMPU_STATUS):
                assert int(g_used[i]) == used, where
        # every byte outside the produced ranges keeps its poison: behind out_len, between the units, in front of the first
        assert (g_out[keep] == POISON).all(), (mis, flags, np.flatnonzero(g_out[keep] != POISON)[:8])
