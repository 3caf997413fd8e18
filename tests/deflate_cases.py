"""Hand-built DEFLATE, zlib and gzip streams (tests/deflate_writer.py), each aimed at forms zlib's encoder never emits, or at the bits
and bytes where the inflate kernel changes path.

A case is (name, data, fmt, want, tags, cuts, layout, blocks, tail): `fmt` is raw, zlib, gzip or auto (the decoder's format); `want`
the content, Err(code, zlib's message) or Cut(content) for a stream that ends early; `tags` the features of FEATURES it reaches, each
checked by a predicate over the layout records (PREDICATES); `cuts` the byte offsets at which its blocks begin; `tail` the bytes
behind the stream's end.  The geometry below is the kernel's (a CPU test holds these numbers to the HIP sources)."""
import random
from collections import namedtuple

import deflate_writer as W

# compu_amd/csrc/inflate_unit.h
S_BITS = 320            # a lane's walk segment
XT_BITS = 1536          # how far a lane walks past its segment (dynamic blocks)
XT_BITS_FIXED = 3072    # (fixed blocks)
ROW_TOKENS = 256        # tokens a lane records per super-round
CHUNK_BYTES = 2560      # output of one executor chunk
MQ_CAP = 128            # queued matches
LIT_ROOT, DIST_ROOT = 9, 8
GROUP = 64              # tokens per executor step (one per lane)
# compu_amd/csrc/api.hip
DEC_DROP_OUT = 1 << 20  # a streaming decoder drops delivered output in front of the window once this much can go
WINDOW = 32768

Case = namedtuple("Case", "name data fmt want tags cuts layout blocks tail content")
Err = namedtuple("Err", "code msg")
Cut = namedtuple("Cut", "content")
MODES = {"raw": -15, "zlib": 15, "gzip": 31, "auto": 47}

BAD_LIT = Err(-3, "invalid literal/length code")
BAD_DIST = Err(-3, "invalid distance code")
FAR = Err(-3, "invalid distance too far back")


def _case(name, s, tags, fmt="raw", want=None, tail=0, cut=None):
    data = s.data if cut is None else s.data[:cut]
    if cut is not None:
        want = Cut(s.content)
    return Case(name, data, fmt, s.content if want is None else want, frozenset(tags.split()), [c for c in s.cuts if c < len(data)],
                s.layout, s.blocks, tail, s.content)


def _rb(rnd, n, lo=0, hi=256):
    return [rnd.randrange(lo, hi) for _ in range(n)]


def _lits_of_bits(rnd, t):
    """fixed-Huffman literals that take exactly `t` bits (8- and 9-bit codes)"""
    a = t % 8
    b = (t - 9 * a) // 8
    assert b >= 0
    out = [rnd.randrange(144, 256) for _ in range(a)] + [rnd.randrange(0, 144) for _ in range(b)]
    rnd.shuffle(out)
    return out


def _complete(lens_by_sym, n):
    out = [0] * n
    for s, l in lens_by_sym.items():
        out[s] = l
    assert W.kraft(out) == 32768, W.kraft(out)
    return out


# ---- tables
def table_cases():
    rnd = random.Random(1)
    out = []
    # every code length 1..15, in both alphabets, each used
    syms = list(range(65, 78)) + [257, 258, 256]
    lit = _complete({s: min(i + 1, 15) for i, s in enumerate(syms)}, 259)
    dsyms = list(range(16))
    dist = _complete({s: min(i + 1, 15) for i, s in enumerate(dsyms)}, 16)
    toks = [rnd.choice(syms[:13]) for _ in range(260)] + syms[:13]
    toks += [("m", 3 + ds % 2, W.DBASE[ds]) for ds in dsyms]
    d = W.Deflate().dynamic(toks, lit, dist, final=True)
    out.append(_case("lengths_1_to_15", W.wrap(d), "len_all_lit len_all_dist"))
    # a lit/len set of the end-of-block code alone, one bit; the other bit pattern is no code
    d = W.Deflate().dynamic([], _complete_single(256), [0])
    d.fixed([66, 67], final=True)
    out.append(_case("eob_only", W.wrap(d), "lit_only_eob dist_none"))
    d = W.Deflate().dynamic([], _complete_single(256), [0], eob=False).raw_bits(1, 1).raw_bits(0, 7)
    out.append(_case("eob_only_twin", W.wrap(d), "lit_only_eob lit_twin_hit", want=BAD_LIT))
    # a single 1-bit distance code: used, then its missing twin
    lit = W.lengths_for({97: 4, 98: 2, 257: 3, 258: 1, 256: 1}, 15, 259)
    d = W.Deflate().dynamic([97, 98, ("m", 3, 1), 97, ("m", 4, 1), 98], lit, [1], final=True)
    out.append(_case("dist_one_code", W.wrap(d), "dist_one_code"))
    d = W.Deflate().dynamic([97, 98, ("m", 3, 1), ("s", 257)], lit, [1], eob=False).raw_bits(1, 1).raw_bits(0, 12)
    out.append(_case("dist_one_code_twin", W.wrap(d), "dist_one_code dist_twin_hit", want=BAD_DIST))
    # no distance codes: literals only (accepted); a length code then has no distance to read
    d = W.Deflate().dynamic([97, 98, 98] * 30, lit, [0, 0], final=True)
    out.append(_case("dist_none_literals", W.wrap(d), "dist_none"))
    d = W.Deflate().dynamic([97, 98, ("s", 258)], lit, [0], eob=False).raw_bits(0, 16)
    out.append(_case("dist_none_match", W.wrap(d), "dist_none dist_none_match", want=BAD_DIST))
    # HLIT = 286 with code 285 in use, HDIST = 30 with code 29 at all 13 extra bits set (distance 32768)
    d = W.Deflate().stored(bytes(_rb(rnd, 40000)))
    toks = [("m", 258, 32768), ("m", 258, 1), 5, ("m", 100, 32768 - 7), ("m", 258, 24577)]
    d.dynamic(toks, final=True, nlit=286, ndist=30)
    out.append(_case("hlit286_hdist30", W.wrap(d), "hlit_286 hdist_30 dist_32768 use_285"))
    # the largest tables: every length above the root has a root prefix that straddles it and the next length (see _largest())
    lit, dist = _largest(rnd)
    d = W.Deflate().stored(bytes(_rb(rnd, 33000)))
    toks = list(range(256)) + [("m", W.LBASE[s - 257] + (1 << W.LEXT[s - 257]) - 1, W.DBASE[ds] + (1 << W.DEXT[ds]) - 1, s, ds)
                               for s, ds in zip(range(257, 286), list(range(30)))]
    toks += [("m", 3 + k, W.DBASE[k] , None, k) for k in range(29, -1, -1)]
    rnd.shuffle(toks)
    d.dynamic(toks, lit, dist, final=True)
    out.append(_case("largest_tables", W.wrap(d), "lit_straddle_all dist_straddle_all root_edge_lit root_edge_dist hlit_286 hdist_30"))
    # length 258 as 284 + 31 and as 285 in one block
    d = W.Deflate().dynamic([1, 2, ("m", 258, 2, 284), ("m", 258, 2, 285), ("m", 227, 1, 284), ("m", 257, 2, 284)], final=True)
    out.append(_case("len258_two_ways", W.wrap(d), "len258_284 use_285", fmt="raw"))
    return out


def _complete_single(sym, n=257):
    lens = [0] * max(n, sym + 1)
    lens[sym] = 1
    return lens


def _largest(rnd):
    """lit/len: 286 codes, 1 x 1 bit, 1 x 2, 26 x 8, 23 x 9, 101 x 10, 1 each of 11..14, 130 x 15 (in 15-bit code space the ends of
    lengths 10..14 lie at 32, 48, 56, 60, 62 mod 64: inside a 9-bit prefix each); distance: 30 codes, 1, 2, 3 bits, 12 x 7, 7 x 8,
    one each of 9..14, 2 x 15 (ends of 9..14 at 64, 96, ..., 126 mod 128)"""
    ll = [1, 2] + [8] * 26 + [9] * 23 + [10] * 101 + [11, 12, 13, 14] + [15] * 130
    syms = list(range(286))
    rnd.shuffle(syms)
    lit = [0] * 286
    for s, l in zip(syms, ll):
        lit[s] = l
    dl = [1, 2, 3] + [7] * 12 + [8] * 7 + [9, 10, 11, 12, 13, 14, 15, 15]
    ds = list(range(30))
    rnd.shuffle(ds)
    dist = [0] * 30
    for s, l in zip(ds, dl):
        dist[s] = l
    assert W.kraft(lit) == W.kraft(dist) == 32768
    return lit, dist


# ---- dynamic block headers
def header_cases():
    rnd = random.Random(2)
    out = []
    # the longest header: 286 + 30 lengths, each its own 7-bit code-length code, all 19 code-length lengths written
    lit = [8] * 226 + [9] * 60
    rnd.shuffle(lit)
    dist = [4] * 2 + [5] * 28
    cl = [0] * 19
    for s, l in zip([0, 16, 17], [1, 2, 3]):
        cl[s] = l
    for s in range(19):
        if not cl[s]:
            cl[s] = 7
    toks = _rb(rnd, 300) + [("m", 10 + k, 1 + k) for k in range(40)]
    d = W.Deflate().dynamic(toks, lit, dist, cl_lens=cl, cl_seq=[(l, 0) for l in lit + dist], final=True)
    out.append(_case("longest_header", W.wrap(d), "cl_7bit hdr_longest hlit_286 hdist_30"))
    hdr_case = W.wrap(d)
    # the code-length code all zeros: zlib reads every symbol as length 0 (its empty table answers symbol 0, 1 bit)
    d = W.Deflate().dynamic(None, [0] * 257, [0], cl_lens=[0] * 19, cl_seq=[])
    d.raw_bits(0, 258 + 16)
    out.append(_case("cl_all_zero", W.wrap(d), "cl_all_zero", want=Err(-3, "invalid code -- missing end-of-block")))
    # 16 right behind 17 / 18 repeats a zero; repeats across the lit/len - distance seam
    toks = [rnd.randrange(0, 20) for _ in range(200)] + [27, 250, ("m", 3, 3), ("m", 8, 129)]
    lit = W.lengths_for({**{s: 5 for s in range(20)}, 27: 1, 250: 1, 256: 1, 257: 1, 262: 1}, 15, 263)
    dist = W.lengths_for({2: 1, 14: 1}, 15, 15)
    seq = []
    for s, x in W.rle_lengths(lit + dist):
        if s == 18 and x + 11 >= 20:  # split: 18 for all but 3..6 zeros, then 16 repeats the last zero
            seq += [(18, x - 4), (16, 1)]
        elif s == 17 and x + 3 >= 6:
            seq += [(17, x - 3), (16, 0)]
        else:
            seq.append((s, x))
    assert W.expand_cl_seq(seq) == lit + dist
    d = W.Deflate().dynamic(toks, lit, dist, cl_seq=seq, final=True)
    out.append(_case("rep16_after_zero_runs", W.wrap(d), "rep16_after_17 rep16_after_18"))
    # lit/len ends with five 6-bit codes and distance starts with seven more: the 16 behind the first of them runs over the seam
    lit = [5] * 16 + [6] * 16 + [7] * 14 + [8] * 10 + [0] * 200 + [7, 7, 7] + [6] * 5
    dist = [6] * 7 + [0] * 3 + [1, 2, 3, 6] + [0] * 16
    assert W.kraft(lit) == W.kraft(dist) == 32768
    toks = [rnd.randrange(0, 56) for _ in range(300)] + [("m", 3 + k % 7, W.DBASE[ds]) for k, ds in enumerate([0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13])]
    d = W.Deflate().dynamic(toks, lit, dist, final=True)
    out.append(_case("repeat16_across_seam", W.wrap(d), "rep16_seam"))
    # lit/len ends with zeros (HLIT = 286) and distance starts with them: a 17 / 18 runs over the seam
    toks = [rnd.randrange(0, 56) for _ in range(300)] + [("m", 3 + k, W.DBASE[ds]) for k, ds in enumerate([6, 8, 10, 11, 12, 13])]
    d = W.Deflate().dynamic(toks, final=True, nlit=286, ndist=14)
    assert d.blocks[-1][3]["lit"][-1] == 0 and d.blocks[-1][3]["dist"][0] == 0
    out.append(_case("zeros_across_seam", W.wrap(d), "zeros_seam hlit_286"))
    # each code-length verdict, in zlib's order
    good_lit = W.lengths_for({97: 3, 98: 2, 256: 1, 257: 1}, 15, 258)
    good_dist = [1, 1]

    def dyn(want, tags, name, final=True, tail_bits=32, **kw):
        d = W.Deflate().dynamic(None, kw.pop("lit", good_lit), kw.pop("dist", good_dist), final=final, **kw)
        d.raw_bits(0, tail_bits)
        out.append(_case(name, W.wrap(d), tags, want=want))

    dyn(Err(-3, "too many length or distance symbols"), "bad_hlit", "hlit_287", hlit=30)
    dyn(Err(-3, "too many length or distance symbols"), "bad_hlit", "hlit_288", hlit=31)
    dyn(Err(-3, "too many length or distance symbols"), "bad_hdist", "hdist_31", hdist=30)
    dyn(Err(-3, "too many length or distance symbols"), "bad_hdist", "hdist_32", hdist=31)
    dyn(Err(-3, "too many length or distance symbols"), "bad_hlit bad_cl_over", "hlit_first", hlit=30, cl_lens=[1] * 19)
    dyn(Err(-3, "invalid code lengths set"), "bad_cl_over", "cl_over", cl_lens=[2] * 5 + [0] * 3 + [2] * 3 + [0] * 5 + [1, 2, 2])
    seq = W.rle_lengths(good_lit + good_dist)
    cf = sorted({s for s, _ in seq})
    cl = [0] * 19
    for s in cf:
        cl[s] = 4
    dyn(Err(-3, "invalid code lengths set"), "bad_cl_incomplete", "cl_incomplete", cl_lens=cl)
    cl = [0] * 19
    cl[5] = 1
    dyn(Err(-3, "invalid code lengths set"), "bad_cl_incomplete cl_one_code", "cl_one_code", cl_lens=cl, cl_seq=[(5, 0)] * 259)
    dyn(Err(-3, "invalid bit length repeat"), "bad_rep_first", "rep16_first", cl_seq=[(16, 0)] + seq)
    dyn(Err(-3, "invalid bit length repeat"), "bad_rep_past_end", "rep18_past_end", cl_seq=seq[:-1] + [(18, 0)])
    dyn(Err(-3, "invalid bit length repeat"), "bad_rep_past_end", "rep16_past_end", cl_seq=seq[:-1] + [(16, 3)])
    dyn(Err(-3, "invalid code -- missing end-of-block"), "bad_no_eob", "no_eob", lit=W.lengths_for({97: 1, 98: 1, 99: 1}, 15, 257))
    over = list(good_lit)
    over[99] = 1
    dyn(Err(-3, "invalid literal/lengths set"), "bad_lit_over", "lit_over", lit=over)
    inc = list(good_lit)
    inc[257] = 0
    inc[256] = 15
    dyn(Err(-3, "invalid literal/lengths set"), "bad_lit_incomplete", "lit_incomplete", lit=inc)
    dyn(Err(-3, "invalid distances set"), "bad_dist_over", "dist_over", dist=[1, 1, 1])
    dyn(Err(-3, "invalid distances set"), "bad_dist_incomplete", "dist_incomplete", dist=[2, 2])
    # the longest header cut at every byte
    blk = [r for r in hdr_case.layout if r.kind == "block"][0]
    for c in range(1, (blk.bit + blk.nbits) // 8 + 1):
        out.append(_case(f"header_cut_{c}", hdr_case, "hdr_cut", cut=c))
    return out


# ---- fixed blocks, chains, empty blocks
def fixed_cases():
    rnd = random.Random(3)
    out = []
    for s in (286, 287):
        d = W.Deflate().fixed([1, 2, 3, ("s", s)], eob=False).raw_bits(0, 16)
        out.append(_case(f"fixed_{s}", W.wrap(d), f"fixed_{s}", want=BAD_LIT))
    for ds in (30, 31):
        d = W.Deflate().fixed([1, 2, 3, ("s", 257), ("d", ds)], eob=False).raw_bits(0, 16)
        out.append(_case(f"fixed_dist{ds}", W.wrap(d), f"fixed_d{ds}", want=BAD_DIST))
    d = W.Deflate().fixed(_rb(rnd, 100) + [("m", 50, 20)]).stored(bytes(_rb(rnd, 300))).fixed([("m", 258, 301), 7, ("m", 30, 1)], final=True)
    out.append(_case("fixed_stored_fixed", W.wrap(d), "chain_fixed_stored_fixed"))
    d = W.Deflate().dynamic(_rb(rnd, 500, 40, 60) + [("m", 20, 77)]).fixed([("m", 258, 400), 200, 201], final=True)
    out.append(_case("dynamic_fixed", W.wrap(d), "chain_dynamic_fixed"))
    d = W.Deflate()
    for _ in range(3000):
        d.fixed([])
    d.fixed([ord("z")], final=True)
    out.append(_case("empty_fixed_3000", W.wrap(d), "empty_fixed_many"))
    d = W.Deflate()
    for k in range(1500):
        d.dynamic([] if k % 2 else [k & 255], final=False)
    d.fixed([ord("z")], final=True)
    out.append(_case("empty_dynamic_1500", W.wrap(d), "empty_dynamic_many"))
    d = W.Deflate().fixed([1]).btype3()
    out.append(_case("btype3", W.wrap(d), "bad_btype3", want=Err(-3, "invalid block type")))
    return out


# ---- stored blocks
def stored_cases():
    rnd = random.Random(4)
    out = []
    d = W.Deflate().stored(b"").stored(bytes(_rb(rnd, 65535))).stored(b"", final=True)
    out.append(_case("stored_0_65535_0", W.wrap(d), "stored_len0 stored_len65535"))
    for r in range(8):
        # a fixed block that ends on bit r of a byte, then a stored block
        d = W.Deflate()
        need = (r - 3 - 7) % 8  # header 3 bits + literals + end-of-block 7 bits = r (mod 8)
        d.fixed(_lits_of_bits(rnd, 8 * 10 + need))
        d.stored(bytes(_rb(rnd, 33 + r))).fixed([("m", 20, 30 + r)], final=True)
        out.append(_case(f"stored_after_bit{r}", W.wrap(d), f"stored_after_bit{r}"))
    d = W.Deflate().fixed([1, 2]).stored(b"abc", nlen_field=0x1234).raw_bits(0, 8)
    out.append(_case("stored_nlen_mismatch", W.wrap(d), "bad_stored_nlen", want=Err(-3, "invalid stored block lengths")))
    d = W.Deflate().fixed([1, 2]).stored(bytes(_rb(rnd, 3000)), final=True)
    s = W.wrap(d)
    hdr = [r for r in s.layout if r.kind == "block" and r.sym == 0][0]
    out.append(_case("stored_cut_in_len", s, "cut_stored_len", cut=(hdr.bit + hdr.nbits) // 8 - 3))
    out.append(_case("stored_cut_in_payload", s, "cut_stored_payload", cut=(hdr.bit + hdr.nbits) // 8 + 1500))
    return out


# ---- the speculative walk
def walk_cases():
    rnd = random.Random(5)
    out = []
    # 1-bit tokens: a lane's row (256 tokens) fills inside its own 320-bit segment
    lit = [0] * 257
    lit[97], lit[98], lit[256] = 1, 2, 2
    d = W.Deflate().dynamic([97] * 30000 + [98] + [97] * 3000, lit, [0]).fixed([1], final=True)
    out.append(_case("one_bit_tokens", W.wrap(d), "tok_1bit"))
    # token lengths all multiples of 3, or of 5: chains that start off the true boundary by a non-multiple never join it
    for m, lens in ((3, {s: 3 for s in range(7)} | {s: 6 for s in range(7, 14)} | {256: 6}), (5, {s: 5 for s in range(31)} | {s: 10 for s in range(31, 62)} | {256: 10})):
        lit = _complete(lens, 257)
        syms = [s for s in lens if s != 256]
        d = W.Deflate().dynamic([rnd.choice(syms) for _ in range(20000)], lit, [0], final=True)
        out.append(_case(f"tokens_mult{m}", W.wrap(d), f"tok_mult{m}"))
    # a fixed block of one byte: 8-bit tokens, and one of long matches
    d = W.Deflate().fixed([65] * 30000).fixed([200] * 7000 + [("m", 258, 1)] * 2000, final=True)
    out.append(_case("fixed_runs", W.wrap(d), "fixed_run"))
    # a one-code distance set: every wrong chain that reads a distance from a 1 bit is invalid
    lit = W.lengths_for({**{s: 3 for s in range(97, 110)}, 256: 1, 258: 8, 259: 3}, 15, 260)
    toks = [97] + [rnd.choice([rnd.randrange(97, 110), ("m", 4, 1), ("m", 5, 1)]) for _ in range(20000)]
    d = W.Deflate().dynamic(toks, lit, [1], final=True)
    out.append(_case("walk_one_dist_code", W.wrap(d), "walk_decoys dist_one_code"))
    # fixed blocks full of 286 / 287 / distance 30 / 31 patterns at wrong offsets: literals 0xC6..0xCF, 0x18..0x1F
    toks = [rnd.choice([0xC6, 0xC7, 0xCF, 0x18, 0x1F, 0xFE, ("m", 3, 1), ("m", 10, 2)]) for _ in range(20000)]
    d = W.Deflate().fixed(toks, final=True)
    out.append(_case("walk_fixed_decoys", W.wrap(d), "walk_decoys"))
    # a block end at, and one straddling, k segments from the super-round's start; the input cut inside that token
    for k in (1, 63, 64, 65):
        for shift, tag in ((0, "at"), (5, "straddle")):
            d = W.Deflate().fixed(_lits_of_bits(rnd, k * S_BITS - shift)).fixed(_rb(rnd, 40) + [("m", 30, 17)], final=True)
            s = W.wrap(d)
            out.append(_case(f"eob_{tag}_seg{k}", s, f"eob_{tag}_seg{k}"))
            if shift:
                eob = [r for r in s.layout if r.kind == "eob"][0]
                out.append(_case(f"cut_in_token_seg{k}", s, f"cut_in_token_seg{k}", cut=(eob.bit + eob.nbits - 1) // 8))
        # the same in a dynamic block: bytes 0..254 at 8 bits, 255 and the end-of-block code at 9
        lit = [8] * 255 + [9, 9]
        t = k * S_BITS - 5
        a = t % 8
        toks = [255] * a + [rnd.randrange(255) for _ in range((t - 9 * a) // 8)]
        d = W.Deflate().dynamic(toks, lit, [0]).fixed([9, 9, 9], final=True)
        out.append(_case(f"dyn_eob_straddle_seg{k}", W.wrap(d), f"eob_straddle_seg{k}"))
    return out


# ---- the executor
def executor_cases():
    rnd = random.Random(6)
    out = []
    toks = _rb(rnd, 20)
    for dd in range(1, 18):
        toks += [("m", 3 + 13 * dd % 250, dd), ("m", 258, dd), rnd.randrange(256)]
    d = W.Deflate().fixed(toks, final=True)
    out.append(_case("distances_1_to_17", W.wrap(d), "dist_1_to_17"))
    # a 258-byte match that starts at each byte near a chunk end
    for p in [CHUNK_BYTES - 258 + e for e in (-1, 0, 1)] + [CHUNK_BYTES - GROUP + e for e in (-1, 0, 1)] + [CHUNK_BYTES + e for e in (-2, -1, 0, 1, 2)]:
        d = W.Deflate().fixed(_rb(rnd, p, 0, 144) + [("m", 258, 1000 if p >= 1000 else p), 1, 2, ("m", 258, 3)], final=True)
        out.append(_case(f"m258_at_{p}", W.wrap(d), "m258_near_chunk_end"))
    # 64 matches of 258 bytes in one group (16 KiB: more than a chunk); then chunks of 3-byte matches only (> MQ_CAP per chunk)
    d = W.Deflate().fixed(_rb(rnd, 64) + [("m", 258, 1 + k) for k in range(64)] + _rb(rnd, 64) + [("m", 3, 1 + k % 700) for k in range(3000)],
                          final=True)
    out.append(_case("group_64x258_and_3byte_chunks", W.wrap(d), "group_64x258 mq_over_cap"))
    # "too far back" at tokens 0, 63, 64, 65 of a group; the distance that equals the output so far is fine
    for i in (0, 63, 64, 65):
        for dd, ok in ((i, True), (i + 1, False)):
            if dd == 0:
                continue
            d = W.Deflate().fixed(_rb(rnd, i, 0, 144) + [("m", 5, dd), 1, 2], final=True)
            out.append(_case(f"far_tok{i}_{'ok' if ok else 'bad'}", W.wrap(d), f"dist_eq_out" if ok else f"far_tok{i} dist_out_plus1",
                             want=None if ok else FAR))
    # at output 32767 / 32768 / 32769, behind a stored block and behind matches in one dynamic block
    for p, ok in ((32767, False), (32768, True), (32769, True)):
        d = W.Deflate().stored(bytes(_rb(rnd, p))).fixed([("m", 10, 32768), 5], final=True)
        out.append(_case(f"far_out{p}_stored", W.wrap(d), f"far_out{p}" if not ok else f"ok_out{p}", want=None if ok else FAR))
        toks = [7] * (1 + (p - 1) % 258) + [("m", 258, 1)] * ((p - 1) // 258) + [("m", 10, 32768), 5]
        d = W.Deflate().dynamic(toks, final=True)
        out.append(_case(f"far_out{p}_tokens", W.wrap(d), f"far_out{p}" if not ok else f"ok_out{p}", want=None if ok else FAR))
    # a few MB of output from 2-bit tokens (length 258, distance 1)
    lit = [0] * 286
    lit[285], lit[120], lit[256] = 1, 2, 2
    d = W.Deflate().dynamic([120] + [("m", 258, 1)] * 16000, lit, [1], final=True)
    out.append(_case("big_2bit_tokens", W.wrap(d), "big_2bit_tokens"))
    # a match at distance 32768 just behind a block boundary, more than DEC_DROP_OUT into the stream
    d = W.Deflate()
    n = DEC_DROP_OUT + WINDOW
    for k in range(0, n, 65535):
        d.stored(bytes(_rb(rnd, min(65535, n - k))))
    d.fixed([("m", 258, 32768), 1, 2, ("m", 100, 32000)], final=True)
    out.append(_case("dist32768_after_drop", W.wrap(d), "dist32768_after_drop"))
    return out


# ---- wrappers
def wrapper_cases():
    rnd = random.Random(7)
    out = []

    def body():
        return W.Deflate().fixed(_rb(rnd, 50, 97, 123) + [("m", 20, 7)]).stored(b"stored!").fixed([1, 2, ("m", 4, 1)], final=True)

    d = body()
    for cinfo, ok in ((7, True), (8, False)):
        want = None if ok else Err(-3, "invalid window size")
        out.append(_case(f"zlib_cinfo{cinfo}", W.wrap(d, "zlib", header=W.zlib_header(cinfo=cinfo)), "zlib_cinfo", "zlib", want))
    out.append(_case("zlib_fcheck", W.wrap(d, "zlib", header=W.zlib_header(fcheck=5)), "zlib_fcheck", "zlib", Err(-3, "incorrect header check")))
    out.append(_case("zlib_cm7", W.wrap(d, "zlib", header=W.zlib_header(cm=7)), "zlib_cm", "zlib", Err(-3, "unknown compression method")))
    out.append(_case("zlib_fdict", W.wrap(d, "zlib", header=W.zlib_header(fdict=True, dictid=0x12345678)), "zlib_fdict", "zlib", Err(2, None)))
    for lv in (0, 1, 3):
        out.append(_case(f"zlib_flevel{lv}", W.wrap(d, "zlib", header=W.zlib_header(flevel=lv, cinfo=lv)), "zlib_flevel", "zlib"))
    out.append(_case("zlib_adler", W.wrap(d, "zlib", trailer=W.zlib_trailer(b"", 0x01020304)), "zlib_bad_adler", "zlib",
                     Err(-3, "incorrect data check")))
    s = W.wrap(d, "zlib")
    for c in range(len(s.data) - 4, len(s.data)):
        out.append(_case(f"zlib_trailer_cut{c - len(s.data) + 4}", s, "trailer_cut", "zlib", cut=c))
    for fmt in ("zlib", "gzip"):
        out.append(_case(f"auto_{fmt}", W.wrap(d, fmt), "auto_" + fmt, "auto"))
    # gzip header fields
    for n in (0, 63, 64, 65, 300):
        name = bytes(_rb(rnd, n, 1, 256))
        out.append(_case(f"gzip_name{n}", W.wrap(d, "gzip", header=W.gzip_header(name=name)), f"gz_name{n}", "gzip"))
        out.append(_case(f"gzip_comment{n}", W.wrap(d, "gzip", header=W.gzip_header(comment=name, name=b"n")), f"gz_comment{n}", "gzip"))
        hdr = W.gzip_header(name=name, comment=name[::-1], hcrc=True, extra=bytes(_rb(rnd, n)))
        out.append(_case(f"gzip_all{n}_auto", W.wrap(d, "gzip", header=hdr), "gz_hcrc_ok gz_extra", "auto"))
        if n in (64, 300):
            for c in range(3, len(hdr), max(1, len(hdr) // 40)):
                out.append(_case(f"gzip_all{n}_cut{c}", W.wrap(d, "gzip", header=hdr), "gz_header_cut", "gzip", cut=c))
    for xl in (0, 1, 2, 1000):
        out.append(_case(f"gzip_extra{xl}", W.wrap(d, "gzip", header=W.gzip_header(extra=bytes(_rb(rnd, xl)))), "gz_extra", "gzip"))
    out.append(_case("gzip_hcrc_ok", W.wrap(d, "gzip", header=W.gzip_header(hcrc=True, mtime=0xDEADBEEF, xfl=2, os_=3)), "gz_hcrc_ok gz_fields", "gzip"))
    out.append(_case("gzip_hcrc_bad", W.wrap(d, "gzip", header=W.gzip_header(hcrc=0x1234, name=b"x")), "gz_hcrc_bad", "gzip",
                     Err(-3, "header crc mismatch")))
    out.append(_case("gzip_ftext", W.wrap(d, "gzip", header=W.gzip_header(flg=1)), "gz_fields", "gzip"))
    for bit in (0x20, 0x40, 0x80):
        out.append(_case(f"gzip_reserved{bit:x}", W.wrap(d, "gzip", header=W.gzip_header(flg=bit)), "gz_reserved", "gzip",
                         Err(-3, "unknown header flags set")))
    out.append(_case("gzip_cm7", W.wrap(d, "gzip", header=W.gzip_header(cm=7)), "gz_cm", "gzip", Err(-3, "unknown compression method")))
    out.append(_case("gzip_crc", W.wrap(d, "gzip", trailer=W.gzip_trailer(bytes(d.content), crc=5)), "gz_bad_crc", "gzip",
                     Err(-3, "incorrect data check")))
    out.append(_case("gzip_isize", W.wrap(d, "gzip", trailer=W.gzip_trailer(bytes(d.content), isize=len(d.content) + 1)), "gz_bad_isize", "gzip",
                     Err(-3, "incorrect length check")))
    s = W.wrap(d, "gzip")
    for c in range(len(s.data) - 8, len(s.data)):
        out.append(_case(f"gzip_trailer_cut{c - len(s.data) + 8}", s, "trailer_cut", "gzip", cut=c))
    # two members: the first finishes, the second is left over; raw streams with trailing bytes
    second = W.wrap(body(), "gzip").data
    out.append(_case("gzip_two_members", W.wrap(d, "gzip", tail=second), "gz_multi", "gzip", tail=len(second)))
    out.append(_case("raw_trailing", W.wrap(d, "raw", tail=b"\x00garbage"), "raw_trailing", tail=8))
    return out


def all_cases():
    return table_cases() + header_cases() + fixed_cases() + stored_cases() + walk_cases() + executor_cases() + wrapper_cases()


# ---- features, each a predicate over a case's layout records
def _toks(c):
    return [r for r in c.layout if r.kind in ("lit", "match", "eob", "sym", "dsym")]


def _dyn(c):
    return [b[3] for b in c.blocks if b[1] == 2 and len(b) > 3]


def _lens_used(c, key):
    """code lengths of the symbols tokens use, per dynamic block"""
    out = set()
    for bi, b in enumerate(c.blocks):
        if b[1] != 2:
            continue
        t = b[3]
        for r in c.layout:
            if r.block != bi:
                continue
            if key == "lit" and r.kind in ("lit", "match", "eob"):
                out.add(t["lit"][r.sym])
            if key == "dist" and r.kind == "match":
                out.add(t["dist"][r.dsym])
    return out


def _straddles(lens, root):
    """every length above the root (but the longest) ends inside a root prefix, so one prefix holds it and the next length"""
    end, ends = 0, {}
    for l in range(1, 16):
        end += sum(1 << (15 - l) for x in lens if x == l)
        ends[l] = end
    top = max(lens)
    return top == 15 and all(ends[l] % (1 << (15 - root)) for l in range(root + 1, top))


def _stored_after_bit(c, r):
    blocks = [r_ for r_ in c.layout if r_.kind == "block"]
    return any(b.sym == 0 and b.bit % 8 == r and i > 0 for i, b in enumerate(blocks))


def _seg_eob(c, k, straddle):
    for bi, b in enumerate(c.blocks):
        recs = [r for r in c.layout if r.block == bi and r.kind != "block"]
        if not recs:
            continue
        t0 = recs[0].bit
        for r in recs:
            if r.kind == "eob":
                edge = t0 + k * S_BITS
                if (r.bit < edge < r.bit + r.nbits) if straddle else r.bit == edge:
                    return True
    return False


def _cut_in_seg_token(c, k):
    if not isinstance(c.want, Cut):
        return False
    end = 8 * len(c.data)
    for bi, b in enumerate(c.blocks):
        recs = [r for r in c.layout if r.block == bi and r.kind != "block"]
        if recs and any(r.bit < end < r.bit + r.nbits and r.bit < recs[0].bit + k * S_BITS < r.bit + r.nbits for r in recs):
            return True
    return False


def _seq_of(c):
    return [t["cl_seq"] for t in _dyn(c)]


def _rep16_after(c, sym):
    return any(any(a[0] == sym and b[0] == 16 for a, b in zip(s, s[1:])) for s in _seq_of(c))


def _seam(c, zeros):
    for t in _dyn(c):
        nl, pos = len(t["lit"]), 0
        for s, x in t["cl_seq"]:
            n = 1 if s < 16 else (3 + x if s == 16 else (3 if s == 17 else 11) + x)
            if pos < nl < pos + n and ((s in (17, 18)) if zeros else s == 16):
                return True
            pos += n
    return False


def _group_matches(c, n, length):
    run = 0
    for r in _toks(c):
        run = run + 1 if r.kind == "match" and r.length == length else 0
        if run >= n:
            return True
    return False


def _far_tok(c, i):
    t = [r for r in _toks(c) if r.block == 0]
    return len(t) > i and t[i].kind == "match" and t[i].dist > t[i].out and t[i].out == i


def _err(c, msg_part):
    return isinstance(c.want, Err) and c.want.msg is not None and msg_part in c.want.msg


def _hdr(c):
    return bytes(c.data[: c.layout[0].bit // 8]) if c.layout else b""


def _gz_flag(c, bit):
    h = _hdr(c)
    return len(h) >= 10 and h[:2] == b"\x1f\x8b" and h[3] & bit


def _gz_field_len(c, which):
    """length of FNAME (which = 8) or FCOMMENT (16) in a gzip header"""
    h = _hdr(c)
    if not _gz_flag(c, which):
        return None
    k = 10
    if h[3] & 4:
        k += 2 + h[10] + 256 * h[11]
    if which == 16 and h[3] & 8:
        k = h.index(0, k) + 1
    return h.index(0, k) - k


PREDICATES = {
    "len_all_lit": lambda c: _lens_used(c, "lit") >= set(range(1, 16)),
    "len_all_dist": lambda c: _lens_used(c, "dist") >= set(range(1, 16)),
    "lit_only_eob": lambda c: any(sum(1 for x in t["lit"] if x) == 1 and t["lit"][256] == 1 for t in _dyn(c)),
    "lit_twin_hit": lambda c: c.want == BAD_LIT and any(sum(1 for x in t["lit"] if x) == 1 for t in _dyn(c)),
    "dist_one_code": lambda c: any(sum(1 for x in t["dist"] if x) == 1 and max(t["dist"]) == 1 for t in _dyn(c)),
    "dist_twin_hit": lambda c: c.want == BAD_DIST and any(sum(1 for x in t["dist"] if x) == 1 for t in _dyn(c)),
    "dist_none": lambda c: any(not any(t["dist"]) for t in _dyn(c)),
    "dist_none_match": lambda c: c.want == BAD_DIST and any(not any(t["dist"]) for t in _dyn(c)) and any(r.kind == "sym" for r in c.layout),
    "hlit_286": lambda c: any(len(t["lit"]) == 286 for t in _dyn(c)),
    "hdist_30": lambda c: any(len(t["dist"]) == 30 for t in _dyn(c)),
    "dist_32768": lambda c: any(r.kind == "match" and r.dist == 32768 and r.dsym == 29 and r.extra[1] == 8191 for r in c.layout),
    "use_285": lambda c: any(r.kind == "match" and r.sym == 285 for r in c.layout),
    "len258_284": lambda c: any(r.kind == "match" and r.sym == 284 and r.extra[0] == 31 for r in c.layout),
    "lit_straddle_all": lambda c: any(len(t["lit"]) == 286 and _straddles(t["lit"], LIT_ROOT) for t in _dyn(c)) and _lens_used(c, "lit") >= set(range(LIT_ROOT, 16)),
    "dist_straddle_all": lambda c: any(len(t["dist"]) == 30 and _straddles(t["dist"], DIST_ROOT) for t in _dyn(c)) and _lens_used(c, "dist") >= set(range(DIST_ROOT, 16)),
    "root_edge_lit": lambda c: _lens_used(c, "lit") >= {LIT_ROOT, LIT_ROOT + 1},
    "root_edge_dist": lambda c: _lens_used(c, "dist") >= {DIST_ROOT, DIST_ROOT + 1},
    "cl_7bit": lambda c: any(max(t["cl"]) == 7 and any(t["cl"][s] == 7 for s, _ in t["cl_seq"]) for t in _dyn(c)),
    "hdr_longest": lambda c: any(r.kind == "block" and r.sym == 2 and r.nbits == 3 + 14 + 57 + 316 * 7 for r in c.layout),
    "cl_all_zero": lambda c: any(not any(t["cl"]) for t in _dyn(c)),
    "rep16_after_17": lambda c: _rep16_after(c, 17),
    "rep16_after_18": lambda c: _rep16_after(c, 18),
    "rep16_seam": lambda c: _seam(c, False),
    "zeros_seam": lambda c: _seam(c, True),
    "bad_hlit": lambda c: _err(c, "too many") and _hlit_field(c) > 29,
    "bad_hdist": lambda c: _err(c, "too many") and _hdist_field(c) > 29,
    "bad_cl_over": lambda c: any(W.kraft(t["cl"]) > 32768 for t in _dyn(c)),
    "bad_cl_incomplete": lambda c: _err(c, "code lengths set") and any(W.kraft(t["cl"]) < 32768 for t in _dyn(c)),
    "cl_one_code": lambda c: any(sum(1 for x in t["cl"] if x) == 1 for t in _dyn(c)),
    "bad_rep_first": lambda c: _err(c, "repeat") and any(t["cl_seq"][0][0] == 16 for t in _dyn(c)),
    "bad_rep_past_end": lambda c: _err(c, "repeat") and any(W.expand_cl_seq(t["cl_seq"]) is not None and len(W.expand_cl_seq(t["cl_seq"])) > len(t["lit"]) + len(t["dist"]) for t in _dyn(c)),
    "bad_no_eob": lambda c: _err(c, "missing end-of-block") and any(t["lit"][256] == 0 and any(t["lit"]) for t in _dyn(c)),
    "bad_lit_over": lambda c: _err(c, "literal/lengths set") and any(W.kraft(t["lit"]) > 32768 for t in _dyn(c)),
    "bad_lit_incomplete": lambda c: _err(c, "literal/lengths set") and any(W.kraft(t["lit"]) < 32768 for t in _dyn(c)),
    "bad_dist_over": lambda c: _err(c, "distances set") and any(W.kraft(t["dist"]) > 32768 for t in _dyn(c)),
    "bad_dist_incomplete": lambda c: _err(c, "distances set") and any(W.kraft(t["dist"]) < 32768 for t in _dyn(c)),
    "hdr_cut": lambda c: isinstance(c.want, Cut) and any(r.kind == "block" and r.sym == 2 and 8 * len(c.data) < r.bit + r.nbits for r in c.layout),
    "fixed_286": lambda c: any(r.kind == "sym" and r.sym == 286 and c.blocks[r.block][1] == 1 for r in c.layout),
    "fixed_287": lambda c: any(r.kind == "sym" and r.sym == 287 and c.blocks[r.block][1] == 1 for r in c.layout),
    "fixed_d30": lambda c: any(r.kind == "dsym" and r.dsym == 30 and c.blocks[r.block][1] == 1 for r in c.layout),
    "fixed_d31": lambda c: any(r.kind == "dsym" and r.dsym == 31 and c.blocks[r.block][1] == 1 for r in c.layout),
    "chain_fixed_stored_fixed": lambda c: any(a[1] == 1 and b[1] == 0 and d[1] == 1 for a, b, d in zip(c.blocks, c.blocks[1:], c.blocks[2:])),
    "chain_dynamic_fixed": lambda c: any(a[1] == 2 and b[1] == 1 for a, b in zip(c.blocks, c.blocks[1:])),
    "empty_fixed_many": lambda c: sum(1 for bi, b in enumerate(c.blocks) if b[1] == 1 and _ntok(c, bi) == 0) >= 2000,
    "empty_dynamic_many": lambda c: sum(1 for bi, b in enumerate(c.blocks) if b[1] == 2 and _ntok(c, bi) == 0) >= 700,
    "bad_btype3": lambda c: any(b[1] == 3 for b in c.blocks) and _err(c, "block type"),
    "stored_len0": lambda c: any(r.kind == "stored" and r.nbits == 0 for r in c.layout),
    "stored_len65535": lambda c: any(r.kind == "stored" and r.nbits == 8 * 65535 for r in c.layout),
    **{f"stored_after_bit{r}": (lambda r: lambda c: _stored_after_bit(c, r))(r) for r in range(8)},
    "bad_stored_nlen": lambda c: _err(c, "stored block lengths"),
    "cut_stored_len": lambda c: isinstance(c.want, Cut) and any(r.kind == "stored" and r.bit - 32 < 8 * len(c.data) < r.bit for r in c.layout),
    "cut_stored_payload": lambda c: isinstance(c.want, Cut) and any(r.kind == "stored" and r.bit < 8 * len(c.data) < r.bit + r.nbits for r in c.layout),
    "tok_1bit": lambda c: _run(c, lambda r: r.nbits == 1) >= 2 * S_BITS,
    "tok_mult3": lambda c: _run(c, lambda r: r.nbits % 3 == 0) >= 10000 and all(r.nbits % 3 == 0 for r in _toks(c)),
    "tok_mult5": lambda c: _run(c, lambda r: r.nbits % 5 == 0) >= 10000 and all(r.nbits % 5 == 0 for r in _toks(c)),
    "fixed_run": lambda c: _run(c, lambda r: r.kind == "lit" and r.sym == 65 and c.blocks[r.block][1] == 1) >= 64 * S_BITS // 8,
    "walk_decoys": lambda c: len(_toks(c)) >= 10000 and (any(sum(1 for x in t["dist"] if x) == 1 for t in _dyn(c)) or
                                                         sum(1 for r in _toks(c) if r.kind == "lit" and r.sym in (0xC6, 0xC7, 0xCF, 0x18, 0x1F)) > 5000),
    **{f"eob_at_seg{k}": (lambda k: lambda c: _seg_eob(c, k, False))(k) for k in (1, 63, 64, 65)},
    **{f"eob_straddle_seg{k}": (lambda k: lambda c: _seg_eob(c, k, True))(k) for k in (1, 63, 64, 65)},
    **{f"cut_in_token_seg{k}": (lambda k: lambda c: _cut_in_seg_token(c, k))(k) for k in (1, 63, 64, 65)},
    "dist_1_to_17": lambda c: {r.dist for r in c.layout if r.kind == "match" and r.length > r.dist} >= set(range(1, 18)),
    "m258_near_chunk_end": lambda c: any(r.kind == "match" and r.length == 258 and abs(r.out - CHUNK_BYTES) <= 258 + 2 for r in c.layout),
    "group_64x258": lambda c: _group_matches(c, GROUP, 258),
    "mq_over_cap": lambda c: _group_matches(c, CHUNK_BYTES // 3, 3) and CHUNK_BYTES // 3 > MQ_CAP,
    **{f"far_tok{i}": (lambda i: lambda c: _far_tok(c, i) and c.want == FAR)(i) for i in (0, 63, 64, 65)},
    "dist_eq_out": lambda c: any(r.kind == "match" and r.dist == r.out for r in c.layout) and isinstance(c.want, bytes),
    "dist_out_plus1": lambda c: any(r.kind == "match" and r.dist == r.out + 1 for r in c.layout) and c.want == FAR,
    "far_out32767": lambda c: any(r.kind == "match" and r.out == 32767 and r.dist == 32768 for r in c.layout) and c.want == FAR,
    "ok_out32768": lambda c: any(r.kind == "match" and r.out == 32768 and r.dist == 32768 for r in c.layout) and isinstance(c.want, bytes),
    "ok_out32769": lambda c: any(r.kind == "match" and r.out == 32769 and r.dist == 32768 for r in c.layout) and isinstance(c.want, bytes),
    "big_2bit_tokens": lambda c: _run(c, lambda r: r.nbits == 2 and r.kind == "match" and r.length == 258) >= 10000,
    "dist32768_after_drop": lambda c: any(r.kind == "match" and r.dist == 32768 and r.out >= DEC_DROP_OUT + WINDOW and _first_tok(c, r) for r in c.layout),
    "zlib_cinfo": lambda c: c.fmt == "zlib" and c.data[0] >> 4 in (7, 8),
    "zlib_fcheck": lambda c: c.fmt == "zlib" and ((c.data[0] << 8) | c.data[1]) % 31 != 0,
    "zlib_cm": lambda c: c.fmt == "zlib" and c.data[0] & 15 != 8,
    "zlib_fdict": lambda c: c.fmt == "zlib" and c.data[1] & 0x20 and c.want == Err(2, None),
    "zlib_flevel": lambda c: c.fmt == "zlib" and c.data[1] >> 6 != 2,
    "zlib_bad_adler": lambda c: c.fmt == "zlib" and _err(c, "data check"),
    "trailer_cut": lambda c: isinstance(c.want, Cut) and c.layout[-1].bit + c.layout[-1].nbits <= 8 * len(c.data),
    "auto_zlib": lambda c: c.fmt == "auto" and c.data[0] & 15 == 8 and c.data[:2] != b"\x1f\x8b",
    "auto_gzip": lambda c: c.fmt == "auto" and c.data[:2] == b"\x1f\x8b",
    **{f"gz_name{n}": (lambda n: lambda c: _gz_field_len(c, 8) == n)(n) for n in (0, 63, 64, 65, 300)},
    **{f"gz_comment{n}": (lambda n: lambda c: _gz_field_len(c, 16) == n)(n) for n in (0, 63, 64, 65, 300)},
    "gz_extra": lambda c: bool(_gz_flag(c, 4)),
    "gz_hcrc_ok": lambda c: bool(_gz_flag(c, 2)) and isinstance(c.want, bytes),
    "gz_hcrc_bad": lambda c: bool(_gz_flag(c, 2)) and _err(c, "header crc"),
    "gz_fields": lambda c: c.fmt == "gzip" and (c.data[3] & 1 or c.data[4:10] != bytes([0, 0, 0, 0, 0, 255])),
    "gz_header_cut": lambda c: isinstance(c.want, Cut) and c.data[:2] == b"\x1f\x8b" and 8 * len(c.data) <= c.layout[0].bit,
    "gz_reserved": lambda c: c.data[:2] == b"\x1f\x8b" and c.data[3] & 0xE0,
    "gz_cm": lambda c: c.data[:2] == b"\x1f\x8b" and c.data[2] != 8,
    "gz_bad_crc": lambda c: c.fmt == "gzip" and _err(c, "data check"),
    "gz_bad_isize": lambda c: c.fmt == "gzip" and _err(c, "length check"),
    "gz_multi": lambda c: c.fmt == "gzip" and c.tail > 18 and c.data[len(c.data) - c.tail:][:2] == b"\x1f\x8b",
    "raw_trailing": lambda c: c.fmt == "raw" and c.tail > 0 and isinstance(c.want, bytes),
}
FEATURES = frozenset(PREDICATES)


def _hlit_field(c):
    b = [r for r in c.layout if r.kind == "block" and r.sym == 2][0]
    return (int.from_bytes(c.data, "little") >> (b.bit + 3)) & 31


def _hdist_field(c):
    b = [r for r in c.layout if r.kind == "block" and r.sym == 2][0]
    return (int.from_bytes(c.data, "little") >> (b.bit + 8)) & 31


def _ntok(c, bi):
    return sum(1 for r in c.layout if r.block == bi and r.kind in ("lit", "match", "sym"))


def _run(c, pred):
    best = run = 0
    for r in _toks(c):
        run = run + 1 if pred(r) else 0
        best = max(best, run)
    return best


def _first_tok(c, r):
    return next(x for x in c.layout if x.block == r.block and x.kind != "block") is r
