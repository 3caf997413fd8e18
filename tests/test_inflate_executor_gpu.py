"""The LZ77 executor of the inflate kernel (flush_tokens / round_issue / round_finish / lds_put in compu_amd/csrc/inflate_unit.h)
against the oracle, on streams built here from zlib and from hand-made bit streams (tests/deflate_writer.py), as raw deflate and
as gzip, at all four byte misalignments of the output:

  * units whose token count per super-round is no multiple of 64 (the last group of a batch has lanes behind its end);
  * a group of 64 matches of length 258 (16 KB: it does not fit a chunk, whether the chunk is empty or not);
  * chunks that end exactly at CHUNK_BYTES, by literals and by a match, and a match that would run one byte over;
  * distances that reach the output's first byte and one byte in front of it, below and exactly at 32 768 bytes of output;
  * capacity that ends inside a match, at its first byte, and exactly at a token boundary;
  * self-overlapping matches of distance 1, 2, 3 and 17 whose source or destination straddles a chunk's end.

Every case compares bytes and out_len with oracle.inflate_units (same offsets, same capacities), status and in_used with the
oracle's decoder, and the bytes behind out_len must keep their poison.  The first test needs no GPU: it pins what the oracle alone
says about each case, so that the GPU comparison stands on verdicts that were looked at."""
import random
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_writer as W
from oracle import oracle as O

CHUNK_BYTES = 2560  # output of one executor chunk (CHIP_CHUNK_BYTES)
POISON = 0xA5
FAR = -3            # Z_DATA_ERROR: "invalid distance too far back"

# want: FINISHED, or FAR; caps: capacities to run the unit at (None = room for everything and a little more)
Case = namedtuple("Case", "name body content want caps")


def _lits(rnd, n):
    return [rnd.randrange(97, 123) for _ in range(n)]


def _mixed(rnd, n_out, max_len=258):
    """literals and matches (any length, any distance within the output so far) giving exactly n_out bytes; -> tokens, match starts"""
    toks, pos, starts = [], 0, []
    while pos < n_out:
        room = n_out - pos
        if pos >= 1 and room >= 3 and rnd.random() < 0.35:
            ln = min(room, rnd.choice([3, 3, 4, 5, 6, 8, 11, 16, 17, 31, 32, 33, 64, 100, max_len]))
            dist = rnd.randrange(1, min(pos, 32768) + 1) if rnd.random() < 0.7 else rnd.randrange(1, min(pos, 40) + 1)
            starts.append((pos, ln))
            toks.append(("m", ln, dist))
            pos += ln
        else:
            toks.append(rnd.randrange(97, 123))
            pos += 1
    return toks, starts


def _dyn(tokens):
    d = W.Deflate().dynamic(tokens, final=True, ndist=2)  # (a lone distance symbol gets its twin at symbol + 1)
    return d.body(), bytes(d.content)


def _fix(tokens):
    d = W.Deflate().fixed(tokens, final=True)
    return d.body(), bytes(d.content)


def _prefix(rnd, n):
    """tokens that give exactly n bytes quickly: a few literals, then long matches"""
    toks, pos = [], 0
    while pos < min(n, 40):
        toks.append(rnd.randrange(97, 123))
        pos += 1
    while pos < n:
        ln = min(258, n - pos)
        if ln < 3:
            toks += _lits(rnd, ln)
        else:
            toks.append(("m", ln, rnd.randrange(1, min(pos, 32768) + 1)))
        pos += ln
    return toks


def build_cases():
    rnd = random.Random(20240611)
    cases = []

    def add(name, body, content, want=O.FINISHED, caps=(None,)):
        cases.append(Case(name, body, content, want, tuple(caps)))

    # -- token counts that are no multiple of 64 (or 128): exact small counts by hand, arbitrary ones from zlib
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 1000, 2561):
        toks, _ = _mixed(rnd, 4 * n)
        toks = toks[:n] if len(toks) >= n else toks + _lits(rnd, n - len(toks))
        add(f"tokens_{n}", *_dyn(toks))
    text = bytes(rnd.choice(b"abcdefgh \n") for _ in range(70000))
    words = b" ".join(rnd.choice([b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta"]) for _ in range(12000))
    for nm, data in (("text", text), ("words", words)):
        for size, level in ((777, 1), (5001, 6), (20001, 9), (65536, 6), (65536, 1)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            add(f"zlib_{nm}_{size}_{level}", co.compress(data[:size]) + co.flush(), data[:size])
    # -- a group of 64 matches of length 258: into an empty chunk (after one literal) and into a chunk that already holds bytes
    add("group_258_empty", *_dyn([97] + [("m", 258, 1)] * 70))
    add("group_258_after", *_dyn(_lits(rnd, 100) + [("m", 258, 100)] * 64 + _lits(rnd, 5)))
    add("group_258_fixed", *_fix(_lits(rnd, 63) + [("m", 258, 7)] * 130))
    # -- a chunk that ends exactly at CHUNK_BYTES (for out_off % 4 == m the chunk's first byte sits at image offset m)
    for m in range(4):
        n = CHUNK_BYTES - m
        add(f"chunk_exact_lits_{m}", *_dyn(_lits(rnd, 2 * n + 10)))
        add(f"chunk_exact_match_{m}", *_dyn(_lits(rnd, n - 3) + [("m", 3, 50)] + _lits(rnd, 70) + [("m", 30, 60)]))
        add(f"chunk_over_by_one_{m}", *_dyn(_lits(rnd, n - 2) + [("m", 3, 50)] + _lits(rnd, 70)))
        add(f"chunk_exact_long_{m}", *_dyn(_lits(rnd, n - 258) + [("m", 258, 300)] + [("m", 258, 258)] * 12))
    # -- a distance that reaches the first byte of the output (valid) / one byte in front of it (invalid), at positions below and
    #    exactly at 32 768 (there no distance can reach in front any more: the longest one reaches the first byte)
    for p in (1, 2, 63, 64, 300, CHUNK_BYTES - 1, CHUNK_BYTES, CHUNK_BYTES + 1, 20000, 32767):
        pre = _prefix(rnd, p)
        add(f"reach_first_{p}", *_dyn(pre + [("m", 5, p)] + _lits(rnd, 3)))
        body, content = _dyn(pre + [("m", 5, p + 1)] + _lits(rnd, 3))
        add(f"reach_front_{p}", body, content[:p], want=FAR)
    for p in (32768, 32769, 40000):
        add(f"reach_max_{p}", *_dyn(_prefix(rnd, p) + [("m", 7, 32768)] + _lits(rnd, 3)))
    #    the same inside a full group of matches (the test is made in the match lanes of a common group)
    pre = _lits(rnd, 40)
    add("reach_front_in_group", *(lambda b, c: (b, c[: 40 + 3 * 30]))(*_dyn(pre + [("m", 3, 2)] * 30 + [("m", 3, 40 + 90 + 1)] + [("m", 3, 2)] * 60)), want=FAR)
    # -- capacity that ends inside a match, at its first byte, and exactly at a token boundary
    toks, starts = _mixed(rnd, 9000)
    body, content = _dyn(toks)
    caps = {None, 0, 1}
    for pos, ln in starts[3:400:37] + [s for s in starts if s[1] >= 100][:3]:
        caps |= {pos, pos + 1, pos + ln // 2, pos + ln - 1, pos + ln}
    caps |= {CHUNK_BYTES, CHUNK_BYTES - 1, CHUNK_BYTES + 1, 2 * CHUNK_BYTES, len(content) - 1, len(content)}
    add("capacity_mixed", body, content, caps=sorted(caps, key=lambda c: -1 if c is None else c))
    body, content = _dyn([97] + [("m", 258, 1)] * 40)
    add("capacity_long_runs", body, content, caps=(None, 1, 2, 130, 259, 260, CHUNK_BYTES, 1 + 258 * 9, 1 + 258 * 9 + 1, 1 + 258 * 20 - 1))
    # -- self-overlapping matches that straddle a chunk's end: the source ends in one chunk and the copy goes on in the next
    for dist in (1, 2, 3, 17):
        for m in range(4):
            n = CHUNK_BYTES - m
            add(f"overlap_{dist}_{m}", *_dyn(_lits(rnd, n - 5) + [("m", 40, dist)] + _lits(rnd, 9) + [("m", 258, dist)] * 11 + _lits(rnd, 3)))
        add(f"overlap_{dist}_short", *_dyn(_lits(rnd, 20) + [("m", 4, dist), ("m", 9, dist), 101, ("m", 33, dist)] * 150))
    return cases


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def _gzip(body, content):
    return W.gzip_header() + body + W.gzip_trailer(content)


def _units(cases, fmt):
    """-> [(case, stream, capacity)]; for a unit that ends in an error the trailer is that of the whole intended content"""
    units = []
    for c in cases:
        data = c.body if fmt == O.MODE_DEFLATE else _gzip(c.body, c.content)
        for cap in c.caps:
            units.append((c, data, len(c.content) + 19 if cap is None else cap))
    return units


def _decoder_verdict(fmt, data, cap):
    got, ir, orr, st, err = O.InflateDecoder(fmt).decode(data, int(cap))
    return got, len(data) - ir, (err if err else st)


def _layout(units, mis):
    caps = np.array([u[2] for u in units], dtype=np.int64)
    ooff = np.zeros(len(units), dtype=np.int64)
    ooff[1:] = np.cumsum((caps[:-1] + 15 + 16) & ~15)
    ooff += 16 + mis  # every unit's first byte at an address = mis (mod 4); poison in front of the first as well
    total = int(ooff[-1] + caps[-1]) + 32
    return ooff, caps, total


def _pack(units):
    lens = np.array([len(u[1]) for u in units], dtype=np.int64)
    offs = np.zeros(len(units), dtype=np.int64)
    offs[1:] = np.cumsum((lens[:-1] + 7) & ~7)
    buf = np.zeros(int(offs[-1] + lens[-1]) + 8, dtype=np.uint8)
    for i, u in enumerate(units):
        buf[offs[i] : offs[i] + lens[i]] = np.frombuffer(u[1], dtype=np.uint8)
    return buf, offs, lens


def _oracle_units(fmt, units, mis):
    buf, offs, lens = _pack(units)
    ooff, caps, total = _layout(units, mis)
    out = np.full(total, POISON, dtype=np.uint8)
    out, out_len, status, bad = O.inflate_units(fmt, buf, offs, lens, total, ooff, caps, out=out)
    return out, out_len, status


def test_oracle_verdicts(cases):
    """no GPU: what the oracle says about every case is what the case was built for"""
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for fmt in (O.MODE_DEFLATE, O.MODE_GZIP):
        units = _units(cases, fmt)
        for mis in (0, 3):
            out, out_len, status = _oracle_units(fmt, units, mis)
            ooff, caps, _ = _layout(units, mis)
            written = np.zeros(len(out), dtype=bool)
            for i, (c, data, cap) in enumerate(units):
                got, used, st = _decoder_verdict(fmt, data, cap)
                where = (c.name, fmt, cap, st, used)
                # the batch form and the decoder agree
                assert bytes(out[ooff[i] : ooff[i] + out_len[i]]) == got and int(status[i]) == st, where
                written[ooff[i] : ooff[i] + out_len[i]] = True
                if c.want == FAR:
                    assert st == (FAR if cap >= len(c.content) + 1 else O.NEED_OUTPUT) and got == c.content[:cap], where
                elif cap > len(c.content) or (fmt == O.MODE_DEFLATE and cap == len(c.content)):
                    assert st == O.FINISHED and got == c.content and used == len(data), where
                elif cap == len(c.content):  # (gzip: the trailer is read only once the decoder is called again with room)
                    assert st in (O.NEED_OUTPUT, O.FINISHED) and got == c.content, where
                else:
                    assert st == O.NEED_OUTPUT and got == c.content[:cap] and used <= len(data), where
            assert (out[~written] == POISON).all()
    # the geometry the cases aim at
    by = {c.name: c for c in cases}
    assert len(by["group_258_empty"].content) == 1 + 70 * 258 and len(by["chunk_exact_lits_1"].content) == 2 * (CHUNK_BYTES - 1) + 10
    assert sum(1 for c in cases if c.want == FAR) >= 11 and len(by["capacity_mixed"].caps) > 40


def _run_gpu(torch, fmt, units, mis, flags):
    import compu_amd

    buf, offs, lens = _pack(units)
    ooff, caps, total = _layout(units, mis)
    dev = "cuda:0"
    d_out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    out_len, in_used, status = compu_amd.decode_batch(
        fmt, torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), d_out,
        torch.from_numpy(ooff).to(dev), torch.from_numpy(caps.astype(np.int32)).to(dev), flags=flags)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_len.cpu().numpy(), in_used.cpu().numpy(), status.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [O.MODE_DEFLATE, O.MODE_GZIP], ids=["raw", "gzip"])
@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_executor_paths_match_the_oracle(gpu, cases, fmt, mis):
    import compu_amd

    units = _units(cases, fmt)
    ooff, caps, _ = _layout(units, mis)
    r_out, r_len, r_st = _oracle_units(fmt, units, mis)
    verdicts = [_decoder_verdict(fmt, data, cap) for _, data, cap in units]
    for flags in (compu_amd.F_COMPU_STATUS, 0):
        g_out, g_len, g_used, g_st = _run_gpu(gpu, fmt, units, mis, flags)
        keep = np.ones(len(g_out), dtype=bool)
        for i, (c, data, cap) in enumerate(units):
            _, used, st = verdicts[i]
            where = (c.name, mis, flags, cap, int(g_st[i]), st, int(g_used[i]), used, int(g_len[i]), int(r_len[i]))
            assert int(g_len[i]) == int(r_len[i]), where
            lo, hi = int(ooff[i]), int(ooff[i]) + int(r_len[i])
            assert np.array_equal(g_out[lo:hi], r_out[lo:hi]), where
            keep[lo:hi] = False
            if flags & compu_amd.F_COMPU_STATUS:
                assert int(g_st[i]) == st == int(r_st[i]), where
                if st in (O.NEED_OUTPUT, O.FINISHED):
                    assert int(g_used[i]) == used, where
                continue
            # without the flag, the batch call's two documented deviations (include/compu_hip.h): a unit whose output is exactly
            # full and whose input is all read reports CHIP_NEED_OUTPUT; in_used is only zlib's count for a finished unit
            if st == O.NEED_INPUT and int(r_len[i]) == cap and used == len(data) and g_st[i] != O.NEED_INPUT:
                assert g_st[i] == O.NEED_OUTPUT, where
                continue
            assert int(g_st[i]) == st, where
            if st == O.FINISHED:
                assert int(g_used[i]) == used, where
        # every byte outside the produced ranges keeps its poison: behind out_len, between the units, in front of the first
        assert (g_out[keep] == POISON).all(), (mis, flags, np.flatnonzero(g_out[keep] != POISON)[:8])
