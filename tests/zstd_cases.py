"""Hand-built zstd frames (tests/zstd_writer.py), each aimed at forms of RFC 8878 the system libzstd seldom or never emits.

A case is (name, frame, want, tags, cuts, lax): `want` is the content the frame stands for or the ZSTD error code it must get;
`tags` name the features of FEATURES it reaches; `cuts` the frame offsets at which its blocks begin (streaming tests cut the input
there); `lax` is None, or the reason why libzstd 1.4.x accepts a frame that RFC 8878 (and the decoders here) reject."""
import random
from collections import namedtuple

import zstd_writer as W
from zstd_writer import new_offset as N

Case = namedtuple("Case", "name frame want tags cuts lax")

# The feature matrix: every entry must be reached by at least one case (tests/test_zstd_writer_cpu.py)
FEATURES = set(
    # forms libzstd 1.4.8 does not choose (or seldom does)
    "lit_rle huf_direct nseq_3byte rle_ll rle_of rle_ml rep_ll rep_of rep_ml fcs8 fcs2_window did1 did2 did4".split()
    # frame headers
    + "single_fcs1 single_fcs2 single_fcs4 fcs2_256 fcs2_65791 window_min window_mantissa window_nofcs window_fcs4 window_fcs8 "
      "did_zero did_nonzero checksum checksum_wrong unused_bit4 reserved_bit3 fcs_off_by_one empty_frame skippable".split()
    # blocks
    + "raw_block rle_block compressed_block reserved_block block_max_1k block_over_1k block_max_128k block_over_128k".split()
    # literals sections
    + "lit_raw_sf0 lit_raw_sf1 lit_raw_sf3 lit_rle_sf0 lit_rle_sf1 lit_rle_sf3 huf_1s_10 huf_4s_10 huf_4s_14 "
      "huf_4s_18 huf_4s_odd huf_4s_min huf_2sym huf_11bit huf_128w treeless_1s treeless_4s treeless_after_huf treeless_after_rawlit "
      "treeless_after_raw_block treeless_after_rle_block treeless_first".split()
    # table modes: repeat after each other mode, for each table
    + [f"rep_{t}_after_{m}" for t in ("ll", "of", "ml") for m in ("pre", "rle", "fse", "rep")]
    + "rep_after_noseq_block rep_first fse_lt1 fse_zero_runs fse_chained_zero_flags".split()
    + [f"fse_al{a}_{t}" for t in ("ll", "ml") for a in range(5, 10)] + [f"fse_al{a}_of" for a in range(5, 9)]
    # sequence counts
    + "nseq_0 nseq_1 nseq_127 nseq_128 nseq_1000 nseq_7eff nseq_7f00 nseq_big nseq_2byte_small".split()
    # RLE tables at the largest codes
    + "rle_ll35 rle_ml52 rle_of_large rle_of31".split()
    # repeat offsets
    + [f"ov{v}_{k}" for v in (1, 2, 3) for k in ("ll0", "llpos")]
    + "rep0_minus1_zero rep_across_blocks rep_across_raw rep_across_rle".split()
    + [f"repcode_at_{i}" for i in (0, 1, 2, 62, 63, 64, 65)] + [f"run{k}_before_repcode" for k in range(5)]
    # bitstreams, matches, placement
    + "seq_over_64_bits seq_stream_kib match_off1 match_off2 match_off3 offset_to_start offset_past_start "
      "tight_lits_first tight_lits_last tight_lits_interleaved".split()
    # malformed on purpose
    + "bad_lit_size bad_huf_size bad_seq_leftover bad_seq_overread bad_seq_zero_tail bad_huf_leftover bad_huf_overread bad_weights "
      "bad_weight_12 bad_short_block bad_accuracy bad_rle_symbol bad_fse_symbol bad_reserved_modes bad_nseq".split()
)


def _case(name, f, tags, err=None, lax=None, checksum_value=None):
    frame, content = f.finish(checksum_value)
    return Case(name, frame, content if err is None else err, frozenset(tags.split()), f.block_cuts(), lax)


def _rb(rnd, n, lo=97, hi=123):
    return bytes(rnd.randrange(lo, hi) for _ in range(n))


def header_cases():
    rnd = random.Random(1)
    out = []
    for n, tags in ((100, "single_fcs1"), (256, "single_fcs2 fcs2_256"), (65791, "single_fcs2 fcs2_65791"), (70000, "single_fcs4")):
        f = W.Frame(checksum=True)
        f.raw(rnd.randbytes(n), last=True)
        out.append(_case(f"fcs_{n}", f, tags + " raw_block checksum"))
    f = W.Frame(fcs=8)
    f.compressed(_rb(rnd, 40), [(10, 20, N(7))], last=True)
    out.append(_case("single_fcs8", f, "fcs8 compressed_block"))
    for fcs, tag in ((None, "window_nofcs"), (2, "fcs2_window"), (4, "window_fcs4"), (8, "window_fcs8")):
        f = W.Frame(fcs=fcs, window=(0, 0))
        for k in range(3):
            f.raw(rnd.randbytes(1000 if fcs != 2 else 300))
        f.compressed(_rb(rnd, 30), [(5, 100, N(800)), (3, 20, N(799))], last=True)
        out.append(_case(f"window1k_{fcs}", f, f"window_min {tag} raw_block"))
    f = W.Frame(fcs=None, window=(3, 5), checksum=True)
    f.raw(rnd.randbytes(9000))
    f.compressed(_rb(rnd, 10), [(2, 50, N(9000 + 2))], last=True)
    out.append(_case("window_mantissa", f, "window_mantissa window_nofcs checksum"))
    for b in (1, 2, 4):
        for v, ok in ((0, True), ((1 << (8 * b)) - 1, False), (1, False)):
            f = W.Frame(dict_id=(v, b))
            f.raw(b"dictionary id field ", last=True)
            out.append(_case(f"did{b}_{v:x}", f, f"did{b} " + ("did_zero" if ok else "did_nonzero"), None if ok else -32))
    f = W.Frame(window=(0, 0), fcs=None, dict_id=(0, 4))
    f.raw(b"dictionary id and window", last=True)
    out.append(_case("did4_window", f, "did4 did_zero window_min"))
    f = W.Frame(unused_bit=True, checksum=True)
    f.compressed(_rb(rnd, 20), [(4, 9, N(3))], last=True)
    out.append(_case("unused_bit4", f, "unused_bit4"))
    f = W.Frame(reserved_bit=True)
    f.raw(b"abc", last=True)
    out.append(_case("reserved_bit3", f, "reserved_bit3", -14))
    for d in (1, -1):
        for fcs in (True, 4):
            f = W.Frame(fcs=fcs, window=None if fcs is True else (1, 0), fcs_value=300 + d)
            f.raw(rnd.randbytes(200))
            f.compressed(_rb(rnd, 30), [(10, 70, N(150))], last=True)
            out.append(_case(f"fcs_off_by_{d}_{fcs}", f, "fcs_off_by_one", -20 if d > 0 else -70, lax=None if d > 0 else
                             "libzstd decodes a whole frame it is handed at once into a large enough buffer in a single pass, where more "
                             "content than the FCS is -20; in pieces (its buffered path, which the decoders here follow) it is -70"))
    f = W.Frame(checksum=True)
    f.raw(b"checksum", last=True)
    out.append(_case("checksum_wrong", f, "checksum_wrong checksum", -22, checksum_value=0x12345678))
    f = W.Frame()
    f.raw(b"", last=True)
    out.append(_case("empty_raw", f, "empty_frame single_fcs1"))
    f = W.Frame(fcs=None, window=(0, 0), checksum=True)
    f.compressed(b"", [], lit="rle", last=True)
    out.append(_case("empty_compressed", f, "empty_frame nseq_0 lit_rle_sf0 checksum"))
    f = W.Frame(fcs=None, window=(0, 0))
    f.raw(b"two-byte block next")
    f.compressed(b"", [], last=True)
    out.append(_case("compressed_2_bytes", f, "bad_short_block", -20))
    for nib, pay in ((0, b"abc"), (15, b""), (7, bytes(300))):
        out.append(Case(f"skippable_{nib}", W.skippable(pay, nib), b"", frozenset(["skippable"]), [], None))
    return out


def block_cases():
    rnd = random.Random(2)
    out = []
    for win, size, tag in (((0, 0), 1024, "block_max_1k"), ((7, 0), 128 * 1024, "block_max_128k"), ((10, 0), 128 * 1024, "block_max_128k")):
        for over in (0, 1):
            for kind in ("raw", "rle"):
                f = W.Frame(fcs=None, window=win)
                if kind == "raw":
                    f.raw(rnd.randbytes(size + over))
                else:
                    f.rle(0x5A, size + over)
                f.rle(7, 3, last=True)
                t = tag if not over else tag.replace("max", "over")
                out.append(_case(f"{kind}_{size}+{over}_w{win[0]}", f, f"{t} {kind}_block", -20 if over else None))
    f = W.Frame(fcs=None, window=(0, 0))
    f.raw(b"ab")
    f.reserved(b"xyz")
    out.append(_case("reserved_block", f, "reserved_block", -20))
    f = W.Frame(fcs=None, window=(0, 0))  # a compressed block whose Block_Size is above the window
    f.raw(rnd.randbytes(900))
    f.compressed(rnd.randbytes(1100), [], last=True)
    out.append(_case("compressed_over_1k", f, "block_over_1k compressed_block", -20))
    return out


def literal_cases():
    rnd = random.Random(3)
    out = []
    for kind in ("raw", "rle"):
        for sf, sizes in ((0, (1, 17, 31)), (1, (0, 5, 32, 1000, 4095)), (3, (0, 20, 4096, 100000))):
            f = W.Frame(checksum=True)
            f.raw(b"0123456789")
            for n in sizes:
                lits = rnd.randbytes(n) if kind == "raw" else bytes([rnd.randrange(256)]) * n
                seqs = [(min(n, 3), 10, N(7))] if n else []
                f.compressed(lits, seqs, lit=kind, sf=sf)
            f.rle(1, 1, last=True)
            out.append(_case(f"lit_{kind}_sf{sf}", f, f"lit_{kind}_sf{sf} " + ("lit_rle" if kind == "rle" else "")))
    # Huffman: one stream at the 10-bit format, four at 10, 14, 18 bits; sizes around the segment arithmetic of four streams
    for streams, sf, sizes in ((1, 0, (1, 2, 5, 1023)), (4, 1, (6, 7, 8, 9, 10, 11, 1021, 1023)), (4, 2, (1024, 5003, 16383)),
                               (4, 3, (16384, 70001, 131071))):
        f = W.Frame(checksum=True)
        f.raw(b"0123")
        for n in sizes:
            lits = _rb(rnd, n, 40, 100)
            f.compressed(lits, [(n // 2, 4, N(3))] if 2 <= n < 100000 else [], lit="huf", sf=sf, streams=streams)
        f.rle(9, 1, last=True)
        tags = f"huf_direct huf_{streams}s_{[10, 10, 14, 18][sf]}"
        if streams == 4:
            tags += " huf_4s_odd" + (" huf_4s_min" if sf == 1 else "")
        out.append(_case(f"huf_{streams}s_sf{sf}", f, tags))
    # trees: two symbols, an 11-bit code, 128 weights written
    f = W.Frame()
    f.compressed(b"ab" * 50 + b"bbbb", [], lit="huf", weights=[0] * 97 + [1, 1])
    lens = {40 + k: k + 1 for k in range(11)}
    lens[51] = 11
    data = bytes(s for s, d in lens.items() for _ in range(max(1, 600 >> d)))
    f.compressed(bytes(rnd.sample(data, len(data))), [], lit="huf", streams=4, weights=W.weights_of_lengths(lens))
    lens = {s: 7 for s in range(127)}
    lens.update({127: 8, 128: 8})
    f.compressed(bytes(rnd.randrange(129) for _ in range(3000)), [(100, 7, N(50))], lit="huf", streams=4, weights=W.weights_of_lengths(lens), last=True)
    out.append(_case("huf_trees", f, "huf_2sym huf_11bit huf_128w huf_direct"))
    # treeless literals after each kind of block in between
    for between, tag in (("none", "treeless_after_huf"), ("rawlit", "treeless_after_rawlit"), ("raw", "treeless_after_raw_block"),
                         ("rle", "treeless_after_rle_block")):
        for streams in (1, 4):
            f = W.Frame(checksum=True)
            f.compressed(bytes(range(60, 90)) + _rb(rnd, 900, 60, 90), [(100, 30, N(40))], lit="huf", streams=4)
            if between == "rawlit":
                f.compressed(rnd.randbytes(50), [(20, 5, 1)])
            elif between == "raw":
                f.raw(rnd.randbytes(77))
            elif between == "rle":
                f.rle(0x33, 500)
            f.compressed(_rb(rnd, 800, 60, 90), [(0, 9, 2), (300, 12, N(600))], lit="treeless", streams=streams)
            f.compressed(_rb(rnd, 60, 60, 90), [], lit="treeless", streams=1, last=True)
            out.append(_case(f"treeless_{between}_{streams}s", f, f"{tag} treeless_{streams}s"))
    f = W.Frame()
    f.compressed(_rb(rnd, 100, 60, 90), [], lit="treeless", weights=W.huf_weights(bytes(range(60, 90))), last=True)
    out.append(_case("treeless_first", f, "treeless_first", -30))
    return out


def _seqs_for(rnd, n, avail, ml_max=60):
    """`n` sequences over content of `avail` bytes: short literal runs, new offsets and repeat codes"""
    s = []
    for i in range(n):
        ll = rnd.choice([0, 0, 1, 2, 5, 17, 40])
        ov = rnd.choice([1, 2, 3, N(rnd.randrange(1, min(avail, 5000)))])
        s.append((ll, rnd.randrange(3, ml_max), ov))
    return s


def table_cases():
    rnd = random.Random(4)
    out = []
    idx = {"ll": 0, "of": 1, "ml": 2}
    # repeat mode on each table after each other mode; the other two tables in changing modes
    for t in ("ll", "of", "ml"):
        for m in ("pre", "rle", "fse", "rep"):
            f = W.Frame(checksum=True)
            f.raw(rnd.randbytes(3000))
            if m == "rle":
                seqs1 = [(5, 9, N(77))] * 4 if t != "of" else [(3, 20, N(40))] * 3
                seqs1 = [(s[0], s[1], s[2]) for s in seqs1]
            else:
                seqs1 = _seqs_for(rnd, 150, 3000)
            codes = W.seq_codes(seqs1)
            def mode_of(name, prev):
                c = codes[idx[name]]
                if prev == "rle":
                    return ("rle", c[0])
                if prev in ("fse", "rep"):
                    return ("fse", W.fit(c, 6 + idx[name] % 2, less_than_one=c[-1:]), 6 + idx[name] % 2)
                return "pre"
            if m == "rle":
                modes1 = tuple(("rle", codes[idx[n]][0]) if n == t else "pre" for n in ("ll", "of", "ml"))
            else:
                modes1 = tuple(mode_of(n, m if n == t else rnd.choice(["pre", "fse"])) for n in ("ll", "of", "ml"))
            f.compressed(rnd.randbytes(sum(s[0] for s in seqs1) + 20), seqs1, modes=modes1)
            if m == "rep":
                f.compressed(rnd.randbytes(sum(s[0] for s in seqs1)), seqs1, modes=tuple("rep" if n == t else "pre" for n in ("ll", "of", "ml")))
            # the block with the repeated table: its codes come from the first block's
            seqs2 = [seqs1[k] for k in rnd.sample(range(len(seqs1)), min(len(seqs1), 60))]
            seqs2 = [(s[0], s[1], s[2] if s[2] > 3 or t != "of" else s[2]) for s in seqs2]
            f.compressed(rnd.randbytes(sum(s[0] for s in seqs2) + 5), seqs2,
                         modes=tuple("rep" if n == t else "pre" for n in ("ll", "of", "ml")), last=True)
            out.append(_case(f"rep_{t}_after_{m}", f, f"rep_{t}_after_{m} rep_{t}" + (f" rle_{t}" if m == "rle" else "")))
    # a block without sequences in between keeps the tables; repeat mode in the first block is corruption
    f = W.Frame()
    f.raw(rnd.randbytes(2000))
    seqs = _seqs_for(rnd, 40, 2000)
    c = W.seq_codes(seqs)
    f.compressed(rnd.randbytes(300), seqs, modes=(("fse", W.fit(c[0], 7), 7), ("fse", W.fit(c[1], 5), 5), ("fse", W.fit(c[2], 8), 8)))
    f.compressed(rnd.randbytes(33), [])
    f.compressed(rnd.randbytes(300), seqs[::-1], modes=("rep", "rep", "rep"), last=True)
    out.append(_case("rep_after_noseq_block", f, "rep_after_noseq_block rep_ll rep_of rep_ml"))
    for t in ("ll", "of", "ml"):
        f = W.Frame()
        f.raw(rnd.randbytes(100))
        f.compressed(b"xyz", [(1, 5, N(50))], modes=tuple("rep" if n == t else "pre" for n in ("ll", "of", "ml")), last=True, invalid=1)
        out.append(_case(f"rep_first_{t}", f, "rep_first", -20))
    # table descriptions: every accuracy, "less than one" counts, zero runs with chained repeat flags
    for al in range(5, 10):
        f = W.Frame(checksum=True)
        f.raw(rnd.randbytes(4000))
        seqs = _seqs_for(rnd, 300, 4000, 20 if al == 5 else 60)
        seqs += [(0, 1000, N(3999)), (70, 3, 1)]  # codes far apart: long zero runs in the descriptions
        c = W.seq_codes(seqs)
        modes = (("fse", W.fit(c[0], al, less_than_one=[c[0][-2]]), al), ("fse", W.fit(c[1], min(al, 8), less_than_one=[c[1][-2]]), min(al, 8)),
                 ("fse", W.fit(c[2], al, less_than_one=[c[2][-2]]), al))
        f.compressed(rnd.randbytes(sum(s[0] for s in seqs) + 11), seqs, modes=modes, last=True)
        tags = f"fse_al{al}_ll fse_al{al}_ml fse_al{min(al, 8)}_of fse_lt1 fse_zero_runs fse_chained_zero_flags"
        out.append(_case(f"fse_accuracy_{al}", f, tags))
    return out


def count_cases():
    rnd = random.Random(5)
    out = []
    for n in (1, 127, 128, 1000):
        f = W.Frame(checksum=True)
        f.raw(rnd.randbytes(3000))
        seqs = _seqs_for(rnd, n, 3000)
        f.compressed(rnd.randbytes(sum(s[0] for s in seqs)), seqs, last=True)
        out.append(_case(f"nseq_{n}", f, f"nseq_{n}"))
    f = W.Frame()
    f.raw(rnd.randbytes(50))
    seqs = _seqs_for(rnd, 5, 50)
    f.compressed(rnd.randbytes(sum(s[0] for s in seqs)), seqs, nseq_form=2, last=True)
    out.append(_case("nseq_2byte_small", f, "nseq_2byte_small"))
    # many sequences: LL 0, ML 3, Offset_Value 1 (with LL 0: the second repeat offset, so the history alternates 4, 1, 4, ...);
    # every table in RLE mode, so that the bitstream is the closing bit alone
    for n, tag in ((0x7EFF, "nseq_7eff"), (0x7F00, "nseq_7f00 nseq_3byte"), (40000, "nseq_big nseq_3byte")):
        f = W.Frame(checksum=True)
        f.raw(rnd.randbytes(16))
        f.compressed(b"", [(0, 3, 1)] * n, modes=(("rle", 0), ("rle", 0), ("rle", 0)))
        f.compressed(b"!", [(1, 4, N(2))], last=True)
        out.append(_case(f"nseq_{n:x}", f, f"{tag} rle_ll rle_of rle_ml"))
    f = W.Frame()
    f.raw(rnd.randbytes(3000))
    seqs = _seqs_for(rnd, 300, 3000)
    f.compressed(rnd.randbytes(sum(s[0] for s in seqs)), seqs, nseq=301, last=True)
    out.append(_case("nseq_one_too_many", f, "bad_nseq", -20))
    return out


def rle_code_cases():
    rnd = random.Random(6)
    out = []
    f = W.Frame()
    f.raw(rnd.randbytes(100))
    ll = 65536 + 12345
    f.compressed(rnd.randbytes(ll + 10), [(ll, 50, N(90))], modes=(("rle", 35), "pre", "pre"), last=True)
    out.append(_case("rle_ll35", f, "rle_ll35 rle_ll lit_raw_sf3"))
    f = W.Frame()
    f.raw(rnd.randbytes(100))
    f.compressed(b"", [(0, 65539 + 23456, N(7))], modes=("pre", "pre", ("rle", 52)), last=True)
    out.append(_case("rle_ml52", f, "rle_ml52 rle_ml"))
    f = W.Frame()
    f.raw(rnd.randbytes(100000))
    f.raw(rnd.randbytes(100000))
    f.compressed(b"q", [(1, 33, N(150000)), (0, 40, N(140000))], modes=("pre", ("rle", 17), "pre"), last=True)
    out.append(_case("rle_of17", f, "rle_of_large rle_of"))
    for code in (28, 31):
        f = W.Frame(fcs=None, window=(10, 0))
        f.raw(rnd.randbytes(1000))
        f.compressed(b"", [(0, 5, (1 << code) + 77)], modes=("pre", ("rle", code), "pre"), last=True, invalid=1)
        out.append(_case(f"rle_of{code}_far", f, "rle_of31 rle_of" if code == 31 else "rle_of_large", -20))
    for t, code in (("ll", 36), ("of", 32), ("ml", 53)):
        f = W.Frame()
        f.raw(rnd.randbytes(100))
        f.compressed(b"ab", [(1, 5, N(3))], modes=tuple(("rle", {"ll": 1, "of": 2, "ml": 2}[n]) if n == t else "pre" for n in ("ll", "of", "ml")),
                     rle_code={t: code}, last=True)
        out.append(_case(f"rle_{t}_symbol_{code}", f, "bad_rle_symbol", -20))
    return out


def repeat_offset_cases():
    rnd = random.Random(7)
    out = []
    for v in (1, 2, 3):
        for ll in (0, 4):
            f = W.Frame(checksum=True)
            f.raw(rnd.randbytes(64))
            f.compressed(_rb(rnd, 20), [(2, 5, N(5)), (1, 6, N(9)), (3, 4, N(17)), (ll, 11, v), (0, 7, 1), (ll, 5, v)], last=True)
            out.append(_case(f"ov{v}_ll{ll}", f, f"ov{v}_" + ("ll0" if ll == 0 else "llpos")))
    f = W.Frame()
    f.raw(rnd.randbytes(30))
    f.compressed(b"abc", [(1, 6, N(1)), (0, 9, 3), (2, 4, 1), (0, 5, 3)], last=True)  # rep0 = 1, then rep0 - 1 = 0 -> 1
    out.append(_case("rep0_minus1_zero", f, "rep0_minus1_zero ov3_ll0"))
    # repeat codes at chosen indices of a block, after a run of exactly k new offsets
    for i in (0, 1, 2, 62, 63, 64, 65):
        f = W.Frame(checksum=True)
        f.raw(rnd.randbytes(2500))
        tags = {f"repcode_at_{i}"}
        for k in range(min(i, 4) + 1):
            seqs = _seqs_for(rnd, 140, 2500)
            for j in range(i - k, i):
                seqs[j] = (seqs[j][0], seqs[j][1], N(rnd.randrange(1, 2400)))
            if i - k - 1 >= 0:
                seqs[i - k - 1] = (seqs[i - k - 1][0], seqs[i - k - 1][1], rnd.randrange(1, 4))
            seqs[i] = (rnd.choice([0, 3]), seqs[i][1], 1 + (k + i) % 3)
            f.compressed(rnd.randbytes(sum(s[0] for s in seqs) + 3), seqs)
            tags.add(f"run{k}_before_repcode")
        f.rle(1, 1, last=True)
        out.append(_case(f"repcode_at_{i}", f, " ".join(tags)))
    # history across blocks, through raw and RLE blocks in between
    for between, tag in (("none", "rep_across_blocks"), ("raw", "rep_across_raw"), ("rle", "rep_across_rle")):
        f = W.Frame(checksum=True)
        f.raw(rnd.randbytes(1000))
        f.compressed(b"hello", [(1, 5, N(300)), (2, 5, N(500)), (2, 5, N(700))])
        if between == "raw":
            f.raw(rnd.randbytes(40))
        elif between == "rle":
            f.rle(0, 60)
        f.compressed(b"world", [(0, 8, 1), (1, 8, 2), (0, 8, 3), (4, 8, 3)])
        f.compressed(b"", [(0, 20, 1), (0, 20, 2)], last=True)
        out.append(_case(f"rep_history_{between}", f, tag))
    return out


def sequence_cases():
    rnd = random.Random(8)
    out = []
    # sequences of more than 64 bits: LL code 34, ML code 51 and OF code 17, each with count 1 in tables of the largest accuracy
    f = W.Frame(checksum=True)
    f.raw(rnd.randbytes(100000))
    f.raw(rnd.randbytes(80000))
    seqs = [(32768 + 77, 32771 + 999, N(140000)), (16384 + 7, 32771 + 1, N(170001)), (5, 5, N(9)), (0, 40, 1)]
    lits = rnd.randbytes(sum(s[0] for s in seqs))
    c = W.seq_codes(seqs)
    modes = (("fse", W.fit(c[0] + [0] * 200, 9, [33, 34]), 9), ("fse", W.fit(c[1] + [3] * 100, 8, [17]), 8), ("fse", W.fit(c[2] + [2] * 300, 9, [51]), 9))
    f.compressed(lits, seqs, modes=modes, last=True)
    out.append(_case("seq_over_64_bits", f, "seq_over_64_bits fse_al9_ll fse_al9_ml fse_al8_of lit_raw_sf3"))
    # a sequence bitstream of several KiB under FSE tables
    f = W.Frame(checksum=True)
    f.raw(rnd.randbytes(20000))
    seqs = [(rnd.randrange(0, 20), rnd.randrange(3, 50), rnd.choice([1, 2, 3, N(rnd.randrange(1, 20000))])) for _ in range(3000)]
    c = W.seq_codes(seqs)
    f.compressed(rnd.randbytes(sum(s[0] for s in seqs) + 100), seqs,
                 modes=(("fse", W.fit(c[0], 9), 9), ("fse", W.fit(c[1], 8), 8), ("fse", W.fit(c[2], 9), 9)), last=True)
    assert len(f.blocks) - 20003 > 4096 + 3 * 256
    out.append(_case("seq_stream_kib", f, "seq_stream_kib"))
    # matches: offsets 1 to 3 over long lengths; offsets that reach the frame's first byte, and one further
    f = W.Frame(checksum=True)
    f.compressed(b"abcdefgh", [(1, 20000, N(1)), (2, 30000, N(2)), (3, 40000, N(3)), (1, 1000, N(1))], last=False)
    f.compressed(b"", [(0, 65536, 3), (0, 3, 1)], last=True)
    out.append(_case("match_offsets_1_2_3", f, "match_off1 match_off2 match_off3"))
    for extra, tag in ((0, "offset_to_start"), (1, "offset_past_start")):
        f = W.Frame(fcs=None, window=(10, 0))
        f.raw(rnd.randbytes(1234))
        f.compressed(b"xy", [(2, 10, N(1236 + extra))], last=True, invalid=1)
        out.append(_case(f"offset_start_{extra}", f, tag, -20 if extra else None))
    f = W.Frame()
    f.compressed(b"abc", [(3, 10, N(3)), (0, 4, N(14))], last=True, invalid=1)
    out.append(_case("offset_past_start_block1", f, "offset_past_start", -20))
    return out


def tight_cases():
    """literal-heavy blocks (their Huffman literals are parked at the end of the output range) decoded at capacity = content"""
    rnd = random.Random(9)
    out = []
    for where in ("first", "last", "interleaved"):
        f = W.Frame(checksum=True)
        f.raw(rnd.randbytes(64))
        for blk in range(2):
            lits = _rb(rnd, 100000 + blk * 20000, 32, 120)
            if where == "first":
                seqs = [(len(lits), 3000, N(50000))] + [(0, 7, 1)] * 5
            elif where == "last":
                seqs = [(0, 4000, N(1)), (0, 7, N(2))] if blk == 0 else [(10, 4000, N(1000))]
            else:
                seqs = [(5000, 30, N(rnd.randrange(1, 4000))) for _ in range(len(lits) // 5000)]
            f.compressed(lits, seqs, lit="huf", streams=4)
        f.rle(0, 1, last=True)
        out.append(_case(f"tight_lits_{where}", f, f"tight_lits_{where} huf_4s_18"))
    return out


def malformed_cases():
    rnd = random.Random(10)
    out = []

    def base():
        f = W.Frame()
        f.raw(rnd.randbytes(500))
        return f

    f = base()
    f.compressed(rnd.randbytes(40), [(10, 5, N(100))], lit_regen=60, last=True)
    out.append(_case("raw_lit_size_too_big", f, "bad_lit_size", -20))
    f = base()
    f.compressed(_rb(rnd, 200), [(10, 5, N(100))], lit="huf", lit_regen=199, last=True)
    out.append(_case("huf_regen_short", f, "bad_huf_size", -20))
    seqs = [(3, 9, N(100)), (1, 5, 2), (0, 30, N(20))]
    for key, val, tag in (("seq_extra", 3, "bad_seq_leftover"), ("seq_extra", 9, "bad_seq_leftover"), ("seq_drop", 1, "bad_seq_overread"),
                          ("seq_drop", 5, "bad_seq_overread"), ("seq_zero_tail", True, "bad_seq_zero_tail")):
        f = base()
        f.compressed(b"abcd", seqs, modes=(("fse", W.fit([0, 1, 3], 6), 6), "pre", "pre"), last=True, **{key: val})
        out.append(_case(f"{key}_{val}", f, tag, -20, lax=None if key == "seq_zero_tail" else
                         "libzstd 1.4.x does not insist that the sequence bitstream ends exactly (1.5 does: BIT_endOfDStream)"))
    for key, val, tag in (("lit_extra", 5, "bad_huf_leftover"), ("lit_drop", 2, "bad_huf_overread")):
        for streams in (1, 4):
            f = base()
            f.compressed(_rb(rnd, 300, 60, 70), seqs, lit="huf", streams=streams, last=True, **{key: val})
            out.append(_case(f"{key}_{val}_{streams}s", f, tag, -20))
    lits = _rb(rnd, 100, 97, 100)
    for name, tree, tag in (("rest_not_pow2", bytes([127 + 2, 0x31]), "bad_weights"), ("all_zero", bytes([127 + 2, 0x00]), "bad_weights"),
                            ("weight_12", bytes([127 + 3, 0xC1, 0x10]), "bad_weight_12")):
        f = base()
        f.compressed(lits, [], lit="huf", weights=[0] * 97 + [2, 1, 1], tree_bytes=tree, last=True)
        out.append(_case(f"tree_{name}", f, tag, -20))
    for t, al in (("ll", 10), ("of", 9), ("ml", 10)):
        f = base()
        f.compressed(b"ab", [(1, 5, N(9))], modes=tuple(("fse", [2] * 16, 5) if n == t else "pre" for n in ("ll", "of", "ml")),
                     al_field={t: al}, invalid=1, last=True)
        out.append(_case(f"accuracy_{t}_{al}", f, "bad_accuracy", -20))
    for t, nsym in (("ll", 37), ("of", 33), ("ml", 54)):
        f = base()
        norm = [1] * (nsym - 1) + [64 - nsym + 1]
        f.compressed(b"ab", [(1, 5, N(9))], modes=tuple(("fse", norm, 6) if n == t else "pre" for n in ("ll", "of", "ml")),
                     invalid=1, last=True)
        out.append(_case(f"fse_symbols_{t}_{nsym}", f, "bad_fse_symbol", -20))
    for low in (1, 2, 3):
        f = base()
        f.compressed(b"ab", [(1, 5, N(9)), (0, 4, 1)], modes_low=low, last=True)
        out.append(_case(f"modes_reserved_{low}", f, "bad_reserved_modes", -20,
                         lax="libzstd 1.4.x does not look at the reserved low bits of Symbol_Compression_Modes"))
    return out


def all_cases():
    return (header_cases() + block_cases() + literal_cases() + table_cases() + count_cases() + rle_code_cases() + repeat_offset_cases()
            + sequence_cases() + tight_cases() + malformed_cases())
