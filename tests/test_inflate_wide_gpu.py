"""The 16-byte accesses of the inflate kernel and its walk step's table layout (compu_amd/csrc/inflate_unit.h: the chunk store at the
end of flush_tokens, the window staging at the top of walk_round, the `token` step and the tables it reads).

  * chunk store: decoded lengths around 16, 1 024 (one wide trip) and 2 560 (CHUNK_BYTES), every unit at every output offset
    modulo 16, slots back to back in a buffer of 0xA5 with a guard between them: zlib's bytes, and nothing else written;
  * a capacity that cuts a chunk (5 000-byte payload with matches): NeedOutput, the first `cap` bytes, nothing behind them;
  * window staging: the compressed units at every input offset modulo 16, the last one ending with the input tensor's last
    byte, units of fewer than 16 and fewer than 4 compressed bytes: bit-exact, in_used = the unit's length;
  * walk step, hand-built with tests/deflate_writer.py, raw and gzip: a 15-bit literal code, a 15-bit length code with 5 extra
    bits, distance codes of 9..14 bits and of 15 bits with 13 extra bits (sub-tables), a literal pair whose second literal
    starts at bit 31 / 32 / 63 of the mark words, a pair that ends exactly on the chain's limit (the super-round's end, and the
    input's end), invalid literal/length and distance codes as a token's first code and behind a literal.

Expected bytes come from Python's zlib; statuses, and what a stopped unit has written, from the oracle (same offsets and
capacities).  The first test needs no GPU: it pins that the cases are what they are built for."""
import random
import zlib

import numpy as np
import pytest

import deflate_writer as W
from oracle import oracle as O

POISON = 0xA5
GUARD = 32
BAD = -3  # Z_DATA_ERROR
CHUNK_BYTES = 2560
S_BITS, LANES = 320, 64  # the walk's segment and the segments of a super-round
EDGE_LENGTHS = (1, 3, 4, 15, 16, 17, 1023, 1024, 1025, 2559, 2560, 2561, 5121, 65536)
CUT_CAPS = (1, 15, 16, 17, 1030, 2560, 2561, 4999)
CUT_OFFSETS = (0, 1, 7, 15)

_WORDS = [w.encode() for w in "the of and a to in is that it was for on are as with his they at be this from have or by one had not but what "
          "all were when we there can an your which their said if do will each about how up out them then she many some so these would "
          "other into has more her two like him see time could no make than first been its who now people my made over did down only "
          "way find use may water long little very after words called just where most know".split()]


def text(n, seed):
    """n text-like bytes (words from a short list, seeded): compressible, so level 6 finds matches"""
    rnd = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(_WORDS) + (b". " if rnd.random() < 0.1 else b" ")
    return bytes(out[:n])


def raw6(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


_PAYLOADS = {}


def payload(n):
    """(bytes, raw deflate at level 6), made once"""
    if n not in _PAYLOADS:
        p = text(n, 1000 + n)
        _PAYLOADS[n] = (p, raw6(p))
    return _PAYLOADS[n]


def out_layout(caps, mods):
    """slots back to back, GUARD..GUARD+15 bytes between them, slot i at an offset that is mods[i] modulo 16"""
    ooff, pos = [], GUARD
    for cap, m in zip(caps, mods):
        pos += (m - pos) % 16
        ooff.append(pos)
        pos += cap + GUARD
    return np.array(ooff, dtype=np.int64), np.array(caps, dtype=np.int64), pos + 16


def in_layout(streams, mods=None):
    """units one behind the other (unit i at an offset that is mods[i] modulo 16, or 8-byte aligned); the buffer ends with the last unit"""
    offs, pos = [], 0
    for i, s in enumerate(streams):
        pos += (mods[i] - pos) % 16 if mods is not None else -pos % 8
        offs.append(pos)
        pos += len(s)
    buf = np.zeros(pos, dtype=np.uint8)
    for o, s in zip(offs, streams):
        buf[o : o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return buf, np.array(offs, dtype=np.int64), np.array([len(s) for s in streams], dtype=np.int64)


def run_gpu(torch, fmt, buf, offs, lens, ooff, caps, total, flags=0):
    import compu_amd

    dev = "cuda:0"
    d_out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    out_len, in_used, status = compu_amd.decode_batch(
        fmt, torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), d_out,
        torch.from_numpy(ooff).to(dev), torch.from_numpy(caps.astype(np.int32)).to(dev), flags=flags)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_len.cpu().numpy(), in_used.cpu().numpy(), status.cpu().numpy()


def check_written(g_out, ooff, g_len, expect):
    """every unit's bytes are `expect`'s, and every other byte of the buffer (guards, slot bytes behind out_len) is untouched"""
    keep = np.ones(len(g_out), dtype=bool)
    for i, want in enumerate(expect):
        lo = int(ooff[i])
        assert int(g_len[i]) == len(want), (i, int(g_len[i]), len(want))
        got = g_out[lo : lo + len(want)]
        if not np.array_equal(got, np.frombuffer(want, dtype=np.uint8)):
            bad = np.flatnonzero(got != np.frombuffer(want, dtype=np.uint8))
            raise AssertionError((i, lo % 16, len(want), bad[:8].tolist(), len(bad)))
        keep[lo : lo + len(want)] = False
    stray = np.flatnonzero(g_out[keep] != POISON)
    assert len(stray) == 0, np.flatnonzero(keep)[stray][:16].tolist()


# ---- hand-built streams for the walk step ------------------------------------------------------------------------------------
# end-of-block 1 bit, thirteen literals 0..12 of 2..14 bits, two codes of 15 bits: a complete set
def _long_lit_lens(n, a, b):
    lens = [0] * n
    lens[256] = 1
    for i in range(13):
        lens[i] = 2 + i
    lens[a] = lens[b] = 15
    assert W.kraft(lens) == 32768
    return lens


# distance symbols 0..13 of 1..14 bits, 28 and 29 (13 extra bits) of 15 bits: a complete set; symbols 8..13 and 28, 29 are longer
# than the 8-bit root and go through sub-tables of every size
DIST_LENS = [k + 1 for k in range(14)] + [0] * 14 + [15, 15]
assert W.kraft(DIST_LENS) == 32768
# 31 literals and the end-of-block code, all of 5 bits: S_BITS = 64 codes, so every lane's segment starts on a code
FIVE_LITS = list(range(97, 97 + 31))
FIVE_LENS = [0] * 257
for _s in FIVE_LITS + [256]:
    FIVE_LENS[_s] = 5
# 8 codes of 4 bits, 12 of 5, 8 of 6 (the end-of-block code among them)
SHORT_LITS = list(range(97, 97 + 27))
SHORT_LENS = [0] * 257
for _i, _s in enumerate(SHORT_LITS):
    SHORT_LENS[_s] = 4 if _i < 8 else 5 if _i < 20 else 6
SHORT_LENS[256] = 6
assert W.kraft(FIVE_LENS) == 32768 and W.kraft(SHORT_LENS) == 32768


def _second_literal_at(target, hdr_bits):
    """a block of SHORT_LENS literals in which an odd-numbered literal (the second of a pair of the true chain, which starts with
    the block's first token) starts at stream bit `target` modulo 64, the stream's first bit being `hdr_bits` into the unit"""
    by_len = {4: SHORT_LITS[0], 5: SHORT_LITS[8], 6: SHORT_LITS[20]}
    probe = W.Deflate().dynamic([], lit_lens=SHORT_LENS, dist_lens=[0], final=True)
    first = hdr_bits + probe.layout[-1].bit  # where the first token starts (the end-of-block code of the empty block)
    for n in range(1, 40, 2):  # literals in front of it: an odd number
        need = (target - first) % 64
        while need < 4 * n:
            need += 64
        if need > 6 * n:
            continue
        lens = [4] * n
        k = 0
        while sum(lens) < need:
            lens[k % n] += 1
            k += 1
        toks = [by_len[l] for l in lens] + [SHORT_LITS[3], SHORT_LITS[9]] * 20
        d = W.Deflate().dynamic(toks, lit_lens=SHORT_LENS, dist_lens=[0], final=True)
        lits = [r for r in d.layout if r.kind == "lit"]
        assert (hdr_bits + lits[n].bit) % 64 == target and n % 2 == 1
        return d
    raise AssertionError(target)


def build_walk_cases(fmt):
    """-> [(name, stream, content, valid)]; `content` is what comes out (in front of the bad code of an invalid stream)"""
    rnd = random.Random(77)
    hdr = W.gzip_header() if fmt == O.MODE_GZIP else b""
    cases = []

    def add(name, d, valid=True, cut=None):
        body = d.body() if cut is None else d.body()[:cut]
        whole = valid and cut is None
        cases.append((name, hdr + body + (W.gzip_trailer(bytes(d.content)) if whole and hdr else b""), bytes(d.content), whole))

    # a literal code of 15 bits (pairs of them, and next to short ones)
    ll = _long_lit_lens(257, 200, 201)
    add("lit15", W.Deflate().dynamic([rnd.choice((200, 201, 0, 1, 12)) for _ in range(700)], lit_lens=ll, dist_lens=[0], final=True))
    # a length code of 15 bits with 5 extra bits (symbols 281 and 282: lengths 131..194)
    ll = _long_lit_lens(283, 281, 282)
    toks = [0, 1, 2, 12]
    for ln in (131, 140, 162, 163, 194, 150):
        toks += [("m", ln, rnd.randrange(1, 5)), rnd.randrange(0, 13), rnd.randrange(0, 13)]
    add("len15_eb5", W.Deflate().dynamic(toks, lit_lens=ll, dist_lens=[2, 2, 2, 2], final=True))
    # distance codes of 9..14 bits and of 15 bits with 13 extra bits; 16 KiB of output first (1-bit distance code, length 258)
    toks = [97, 98, 99, 100, 101, 102, 103] + [("m", 258, 7)] * 70
    for dist in (17, 24, 25, 32, 33, 48, 49, 64, 65, 96, 97, 128, 16385, 16390, 18000, 1, 2, 3):
        toks += [("m", rnd.choice((3, 9, 40)), dist), rnd.choice((97, 98, 99))]
    d = W.Deflate().dynamic(toks, dist_lens=DIST_LENS, final=True)
    assert {r.dsym for r in d.layout if r.kind == "match"} >= {8, 9, 10, 11, 12, 13, 28}
    add("dist_long", d)
    # a pair whose second literal starts at bit 31, 32 and 63 of the mark words (units are 8-byte aligned in the input)
    for target in (31, 32, 63):
        add(f"pair_second_at_{target}", _second_literal_at(target, 8 * len(hdr)))
    # a pair that ends exactly on the chain's limit: lane 63's last pair ends with the super-round (5-bit codes only: literal
    # 64 k starts lane k's segment), and a stream cut behind a pair's last bit (the input's end is every chain's limit)
    d = W.Deflate().dynamic([rnd.choice(FIVE_LITS) for _ in range(LANES * S_BITS // 5 + 2000)], lit_lens=FIVE_LENS, dist_lens=[0], final=True)
    assert all(r.nbits == 5 for r in d.layout if r.kind == "lit")
    add("pair_ends_super_round", d)
    for nlit in (2, 4, 64, 200):
        d = W.Deflate().dynamic([rnd.choice(FIVE_LITS) for _ in range(1000)], lit_lens=FIVE_LENS, dist_lens=[0], final=True)
        lits = [r for r in d.layout if r.kind == "lit"]
        k = next(k for k in range(nlit, 1000, 2) if (lits[k - 1].bit + 5) % 8 == 0)  # an even count of literals ends on a byte
        d.content = d.content[:k]
        add(f"pair_ends_input_{nlit}", d, cut=(lits[k - 1].bit + 5) // 8)
    # invalid codes (the fixed code's literal/length symbols 286, 287 and distance symbols 30, 31): as a token's first code
    # (at the block's start, behind a match) and as the code behind a literal (the pair's second look-up meets it)
    fronts = {"start": [], "match": [97, 98, ("m", 3, 1)], "lit": [97, 98, ("m", 3, 1), 99], "lits": [97, 98, 99]}
    for where, front in fronts.items():
        for bad in (286, 287):
            add(f"bad_lit_{where}_{bad}", W.Deflate().fixed(front + [("s", bad)], final=True, eob=False).raw_bits(0, 16), valid=False)
        for bad in (30, 31):
            add(f"bad_dist_{where}_{bad}", W.Deflate().fixed(front + [("s", 257), ("d", bad)], final=True, eob=False).raw_bits(0, 16), valid=False)
    return cases


_WALK = {}


def walk_cases(fmt):
    if fmt not in _WALK:
        _WALK[fmt] = build_walk_cases(fmt)
    return _WALK[fmt]


def _walk_oracle(fmt, mis):
    cases = walk_cases(fmt)
    buf, offs, lens = in_layout([c[1] for c in cases])
    ooff, caps, total = out_layout([len(c[2]) + 19 for c in cases], [mis] * len(cases))
    out = np.full(total, POISON, dtype=np.uint8)
    out, out_len, status, _ = O.inflate_units(fmt, buf, offs, lens, total, ooff, caps, out=out)
    return (buf, offs, lens, ooff, caps, total), out, out_len, status


def test_cases_are_what_they_are_built_for():
    """no GPU: zlib decodes every valid stream to its content; the oracle calls the invalid ones data errors behind their content,
    and the cut ones NeedInput with every literal out; the payloads contain matches and the short units are short"""
    for fmt in (O.MODE_DEFLATE, O.MODE_GZIP):
        cases = walk_cases(fmt)
        assert len({c[0] for c in cases}) == len(cases)
        _, out, out_len, status = _walk_oracle(fmt, 0)
        ooff, _, _ = out_layout([len(c[2]) + 19 for c in cases], [0] * len(cases))
        for i, (name, data, content, whole) in enumerate(cases):
            if whole:
                z = zlib.decompressobj(fmt)
                assert z.decompress(data) == content and z.eof and z.unused_data == b"", name
                assert int(status[i]) == O.FINISHED, name
            elif name.startswith("bad_"):
                assert int(status[i]) == BAD, (name, int(status[i]))
            else:
                z = zlib.decompressobj(fmt)
                assert z.decompress(data) == content and not z.eof, name
                assert int(status[i]) == O.NEED_INPUT, (name, int(status[i]))
            assert bytes(out[ooff[i] : ooff[i] + out_len[i]]) == content, name
    assert sum(1 for c in walk_cases(O.MODE_DEFLATE) if c[0].startswith("bad_")) == 16
    for n in EDGE_LENGTHS + (5000,):
        p, c = payload(n)
        assert zlib.decompress(c, -15) == p
        assert n < 1000 or len(c) < 0.6 * n  # matches
    assert len(payload(1)[1]) < 4 and 4 <= len(payload(4)[1]) < 16


@pytest.mark.gpu
def test_chunk_store_edges(gpu):
    units = [(n, m) for n in EDGE_LENGTHS for m in range(16)]
    buf, offs, lens = in_layout([payload(n)[1] for n, _ in units])
    ooff, caps, total = out_layout([n + 5 for n, _ in units], [m for _, m in units])
    g_out, g_len, g_used, g_st = run_gpu(gpu, O.MODE_DEFLATE, buf, offs, lens, ooff, caps, total)
    assert (g_st == O.FINISHED).all(), np.flatnonzero(g_st != O.FINISHED)[:8]
    assert np.array_equal(g_used, lens.astype(np.int32))
    check_written(g_out, ooff, g_len, [payload(n)[0] for n, _ in units])


@pytest.mark.gpu
def test_capacity_cuts_a_chunk(gpu):
    import compu_amd

    pay, comp = payload(5000)
    units = [(cap, m) for cap in CUT_CAPS for m in CUT_OFFSETS]
    buf, offs, lens = in_layout([comp] * len(units))
    ooff, caps, total = out_layout([cap for cap, _ in units], [m for _, m in units])
    ref = np.full(total, POISON, dtype=np.uint8)
    ref, r_len, r_st, _ = O.inflate_units(O.MODE_DEFLATE, buf, offs, lens, total, ooff, caps, out=ref)
    assert (r_st == O.NEED_OUTPUT).all() and np.array_equal(r_len, caps)
    for flags in (0, compu_amd.F_COMPU_STATUS):
        g_out, g_len, g_used, g_st = run_gpu(gpu, O.MODE_DEFLATE, buf, offs, lens, ooff, caps, total, flags)
        assert (g_st == O.NEED_OUTPUT).all(), (flags, g_st.tolist())
        assert np.array_equal(g_len, caps.astype(np.int32)), (flags, g_len.tolist())
        check_written(g_out, ooff, g_len, [pay[:cap] for cap, _ in units])  # the byte at `cap` and the guard are untouched
        assert np.array_equal(g_out, ref)


@pytest.mark.gpu
def test_window_staging_input_offsets(gpu):
    units = [(n, m) for n in EDGE_LENGTHS[:-1] + (5000,) for m in range(16)]
    units.append((65536, 5))
    units.append((3, 11))  # the batch's last unit: a few bytes that end with the tensor
    streams = [payload(n)[1] for n, _ in units]
    buf, offs, lens = in_layout(streams, [m for _, m in units])
    assert {int(o) % 16 for o in offs} == set(range(16)) and int(offs[-1] + lens[-1]) == len(buf)
    assert min(len(s) for s in streams) < 4 and any(4 <= len(s) < 16 for s in streams)
    ooff, caps, total = out_layout([n for n, _ in units], [0] * len(units))
    g_out, g_len, g_used, g_st = run_gpu(gpu, O.MODE_DEFLATE, buf, offs, lens, ooff, caps, total)
    assert (g_st == O.FINISHED).all(), np.flatnonzero(g_st != O.FINISHED)[:8]
    assert np.array_equal(g_used, lens.astype(np.int32))
    check_written(g_out, ooff, g_len, [payload(n)[0] for n, _ in units])
    # the size pass stages the same window
    import compu_amd

    dev = "cuda:0"
    size, s_used, s_st = compu_amd.decode_batch_sizes(O.MODE_DEFLATE, gpu.from_numpy(buf).to(dev), gpu.from_numpy(offs).to(dev), gpu.from_numpy(lens.astype(np.int32)).to(dev))
    gpu.cuda.synchronize()
    assert size.cpu().numpy().tolist() == [n for n, _ in units] and (s_st.cpu().numpy() == O.FINISHED).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [O.MODE_DEFLATE, O.MODE_GZIP], ids=["raw", "gzip"])
def test_walk_step_hand_built(gpu, fmt):
    import compu_amd

    cases = walk_cases(fmt)
    for mis in (0, 5):
        (buf, offs, lens, ooff, caps, total), r_out, r_len, r_st = _walk_oracle(fmt, mis)
        for flags in (compu_amd.F_COMPU_STATUS, 0):
            g_out, g_len, g_used, g_st = run_gpu(gpu, fmt, buf, offs, lens, ooff, caps, total, flags)
            for i, (name, data, content, whole) in enumerate(cases):
                where = (name, mis, flags, int(g_st[i]), int(r_st[i]), int(g_len[i]), int(r_len[i]), int(g_used[i]))
                assert int(g_st[i]) == int(r_st[i]), where
                if whole or int(r_st[i]) == O.NEED_INPUT:
                    assert int(g_used[i]) == len(data), where
            check_written(g_out, ooff, g_len, [c[2] for c in cases])  # zlib's bytes (the no-GPU test ties `content` to zlib)
            assert np.array_equal(g_out, r_out)
