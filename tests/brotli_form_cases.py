"""Hand-built brotli streams of every form the format allows and every error a decoder names (tests/brotli_writer.py):
Case(name, stream, out, err, tags, bounds) -- `out` the output of a valid stream (err None), `err` the BrotliDecoderErrorCode of an
error stream (out None), `tags` the forms the writer recorded while it wrote the stream, `bounds` the output positions at which
metablocks end.  tests/test_brotli_forms_cpu.py holds the table of tags that must be covered.

Shapes the lists asked for that do not exist, and what stands in for them:
  * RLEMAX 16 can be declared but its run code 16 (65536 zeros or more) cannot be used: a context map has at most 64 * 256
    entries.  The cases declare RLEMAX 16 and use run codes up to 7.
  * SIMPLE_HUFFMAN_ALPHABET cannot be raised in the literal alphabet (256) or in the distance alphabet of NPOSTFIX 0, NDIRECT 0
    (64): a simple code's symbol is written in as many bits as the largest symbol needs, and in an alphabet whose size is a power
    of two every value of those bits is a symbol.  It is built for 704, NBLTYPES + 2, NTREES + RLEMAX, the distance alphabet of
    520 symbols and the block count alphabet of 26."""
import collections
import random

import brotli_writer as W

Case = collections.namedtuple("Case", "name stream out err tags bounds")
ERR = dict(EXUBERANT_NIBBLE=-1, RESERVED=-2, EXUBERANT_META_NIBBLE=-3, SIMPLE_HUFFMAN_ALPHABET=-4, SIMPLE_HUFFMAN_SAME=-5,
           CL_SPACE=-6, HUFFMAN_SPACE=-7, CONTEXT_MAP_REPEAT=-8, BLOCK_LENGTH_1=-9, BLOCK_LENGTH_2=-10, TRANSFORM=-11,
           DICTIONARY=-12, WINDOW_BITS=-13, PADDING_1=-14, PADDING_2=-15, DISTANCE=-16)

_cases = None


def _varied(n, seed):
    rnd = random.Random(seed)
    return bytes(rnd.randrange(256) for _ in range(n))


# ---------------------------------------------------------------- valid forms

def _wbits(out):
    for wb in range(10, 25):
        s = W.Stream(wb)
        s.compressed([(b"w%d" % wb, ("dist", 2, 3))], islast=True)
        out.append(("wbits%d" % wb, s))


def _mlen_and_metadata(out):
    for n in (65536, 65537):
        s = W.Stream(17)
        s.compressed([(b"a" * n, None)], islast=True)  # one literal tree of one symbol: the literals take no bits
        out.append(("mlen_%d" % n, s))
    s = W.Stream(21)
    s.uncompressed(_varied(1048577, 11))
    s.last_empty()
    out.append(("mlen_1048577_stored", s))
    s = W.Stream(16)
    s.metadata(b"")
    s.metadata(b"m")
    s.metadata(_varied(256, 1))
    s.compressed([(b"between", None)])
    s.metadata(_varied(257, 2))
    s.last_empty()  # the compressed metablock ended mid-byte, the metadata did not
    out.append(("mskip_0_1_2", s))
    s = W.Stream(16)
    s.metadata(_varied(65537, 3))
    s.compressed([(b"after three length bytes", None)], islast=True)
    out.append(("mskip_3", s))
    s = W.Stream(16)
    s.uncompressed(b"stored, then metadata as the last metablock")
    s.metadata(b"the end", islast=True)
    out.append(("metadata_last", s))
    s = W.Stream(16)
    s.metadata(b"", islast=True)
    out.append(("metadata_last_empty", s))
    s = W.Stream(16)
    s.compressed([(b"abc", ("dist", 1, 2))], codes={("lit", 0): W.simple(3)})
    assert s.w.bitpos() % 8
    s.last_empty()
    out.append(("last_empty_mid_byte", s))


def _simple_forms(out):
    """NSYM 2, 3, 4 and 4 with the tree-select bit, symbols descending, in all six alphabets of one metablock"""
    for n, tsel in ((2, 0), (3, 0), (4, 0), (4, 1)):
        s = W.Stream(16)
        mk = W.simple(n, tsel)
        lits = b"abcd"[:n]
        ins, dists, counts = [4, 2, 3, 1][:n], [2, 3, 5, 6][:n], [3, 6, 10, 14][:n]
        cmds = [(bytes(lits[(i + j) % n] for j in range(ins[i % n])), ("dist", dists[i % n], 2)) for i in range(4 * n)]
        cmds.append((lits[:1] * ins[0], None))  # the command symbol of the first one
        lblocks = [(k % 2, counts[k % n]) for k in range(40)]
        codes = {("bt", 0): mk, ("bl", 0): mk, "lmap": mk, ("ic", 0): mk, ("d", 0): mk}
        codes.update({("lit", t): mk for t in range(n)})
        s.compressed(cmds, islast=True, nbl=(2, 1, 1), blocks=(lblocks, None, None), lmap=[i % n for i in range(128)], ntl=n,
                     codes=codes)
        out.append(("simple%d%s" % (n, "_tree_select" if tsel else ""), s))
    # the distance context map and the block codes of the other two categories
    s = W.Stream(16)
    mk = W.simple(4, 1)
    cmds = [(b"xy", ("dist", 1 + i % 2, 2 + i % 4)) for i in range(12)] + [(b"z", None)]
    s.compressed(cmds, islast=True, nbl=(1, 2, 2), blocks=(None, [(k % 2, 2) for k in range(20)], [(k % 2, 3) for k in range(20)]),
                 dmap=[0, 1, 2, 3, 3, 2, 1, 0], ntd=4,
                 codes={"dmap": mk, ("bt", 1): W.simple(3), ("bl", 1): W.simple(2), ("bt", 2): W.simple(2), ("bl", 2): W.simple(3)})
    out.append(("simple_dmap_and_blocks", s))


def _depth_mix():
    """35 lengths of a complete code with three 8-bit prefixes that need second-level tables of 2, 4 and 7 bits"""
    return [1, 2, 3, 4, 5, 6, 8] + [12] * 16 + [10] * 4 + [9, 10, 11, 12, 13, 14, 15, 15]


def _complex_forms(out):
    s = W.Stream(16)
    s.compressed([(b"abcdefgh" * 2, None)], islast=True, codes={("lit", 0): W.complex_code(hskip=2)})
    out.append(("hskip2", s))
    s = W.Stream(16)
    s.compressed([(b"abcdefghijklmnop" * 2, None)], islast=True, codes={("lit", 0): W.complex_code(hskip=3, spell="rep")})
    out.append(("hskip3_rep16_chain", s))
    s = W.Stream(16)
    s.compressed([(b"ace" * 3, None)], islast=True, codes={("lit", 0): W.complex_code(hskip=0)})
    out.append(("hskip0", s))
    # a code length code of one symbol: every length is read in no bits
    s = W.Stream(16)
    s.compressed([(bytes(range(256)), None)], islast=True,
                 codes={("lit", 0): W.Complex({b: 8 for b in range(256)}, 256, tokens=[(8, 0)] * 256)})
    out.append(("cl_single_8", s))
    s = W.Stream(16)
    s.compressed([(bytes(range(127, -1, -1)), None)], islast=True,
                 codes={("lit", 0): W.Complex({b: 7 for b in range(128)}, 256, tokens=[(7, 0)] * 128)})
    out.append(("cl_single_7", s))
    # a 16 first of all repeats the length 8; 256 of them take a chain of four links
    s = W.Stream(16)
    s.compressed([(bytes(range(255, -1, -1)), None)], islast=True,
                 codes={("lit", 0): W.Complex({b: 8 for b in range(256)}, 256, tokens=[(16, e) for e in W.chain(256, 2)])})
    out.append(("rep16_first", s))
    # 16 chains of two links (15 repeats) and three links (31 repeats), in two literal trees
    s = W.Stream(16)
    lits = bytes(range(80, 97)) + bytes(range(97, 104)) + bytes([88, 111, 90, 80])  # a byte of 96 or more leads to tree 1
    s.compressed([(lits, None)], islast=True, lmap=[0] * 32 + [1] * 32, ntl=2,
                 codes={("lit", 0): W.Complex({b: 5 for b in range(80, 112)}, 256, spell="rep"),
                        ("lit", 1): W.Complex({b: 4 for b in range(88, 104)}, 256, spell="rep")})
    out.append(("rep16_chains", s))
    s = W.Stream(16)
    s.compressed([(bytes(range(32, 48)), None)], islast=True, codes={("lit", 0): W.Complex({b: 4 for b in range(32, 48)}, 256, spell="rep")})
    out.append(("rep16_chain2", s))
    # the same runs cut so that no repeat code follows another
    s = W.Stream(16)
    s.compressed([(bytes(range(64, 96)), None)], islast=True, codes={("lit", 0): W.Complex({b: 5 for b in range(64, 96)}, 256, spell="rep1")})
    out.append(("rep16_unchained", s))
    # 17 chains in the insert-and-copy alphabet: 66 zeros (two links) and 147 zeros (three links)
    s = W.Stream(16)
    cmds = [(b"abcd", ("last", 2)), (b"abc" * 5, ("dist", 3, 12)), (b"c" * 140, ("dist", 1, 3)), (b"", ("dist", 2, 2)), (b"d", None)]
    s.compressed(cmds, islast=True, codes={("ic", 0): W.complex_code(spell="rep", fill=2)})
    out.append(("rep17_chains_704", s))
    # a 16 directly after a 17 (and a 17 after a 16): three zeros, six eights by a 16, then lengths that complete the code
    s = W.Stream(16)
    ln = {3: 8, 4: 8, 5: 8, 6: 8, 7: 8, 8: 8, 9: 1, 10: 2, 11: 3, 12: 0, 13: 0, 14: 0, 15: 4, 16: 5, 17: 7}
    tok = [(17, 0), (16, 3), (1, 0), (2, 0), (3, 0), (17, 0), (4, 0), (5, 0), (7, 0)]
    s.compressed([(bytes([9, 3, 10, 8, 11, 15, 16, 17, 4]), None)], islast=True, codes={("lit", 0): W.Complex(ln, 256, tokens=tok)})
    out.append(("rep16_after_17", s))
    s = W.Stream(16)
    ln = {0: 8, 1: 8, 2: 8, 3: 8, 7: 1, 8: 2, 9: 3, 10: 4, 11: 5, 12: 6}
    tok = [(16, 1), (17, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0)]
    s.compressed([(bytes([0, 7, 3, 12, 9, 1]), None)], islast=True, codes={("lit", 0): W.Complex(ln, 256, tokens=tok)})
    out.append(("rep17_after_16", s))
    # lengths 1, 2, ..., 14, 15, 15
    s = W.Stream(16)
    ln = {40 + i: i + 1 for i in range(15)} | {55: 15}
    s.compressed([(bytes(range(40, 56)) + bytes(range(55, 39, -1)), None)], islast=True, codes={("lit", 0): W.Complex(ln, 256)})
    out.append(("depth15_literals", s))
    # 704 symbols' alphabet, second-level tables of three widths; every command's symbol sits at another depth
    s = W.Stream(16)
    cmds = [(b"abcd", ("last", 2)), (b"abcabcabcabc", ("dist", 3, 12)), (b"c" * 140, ("dist", 1, 3)), (b"", ("dist", 2, 2)),
            (b"xyz", ("dist", 4, 80)), (b"q" * 10, ("dist", 7, 5)), (b"w", ("last", 9)), (b"e", None)]
    depth = _depth_mix()

    def ic_code(used, alpha):
        used = sorted(used)
        rest = [k for k in range(3, alpha, 19) if k not in used]
        picks = [6, 9, 25, 27, 30, 34, 33, 20]  # where in `depth` the used symbols go: lengths 8, 12, 10, 9, 12, 15, 14, 12
        ln = {}
        for u, p in zip(used, picks):
            ln[u] = depth[p]
        left = [d for i, d in enumerate(depth) if i not in picks[:len(used)]]
        for k, d in zip(rest, left):
            ln[k] = d
        return W.Complex(ln, alpha, spell="rep")
    s.compressed(cmds, islast=True, codes={("ic", 0): ic_code})
    out.append(("depth15_704", s))


def _mode_literals(mode):
    """literals after which every context ID 0..63 of the mode has chosen a tree at least once"""
    lits = bytearray()
    if mode == 1:
        for a in range(64):
            lits += bytes([4 * a + (a & 3), 0x55 ^ a])
    elif mode == 2:
        p1s = [0, 9, 32, 33, 34, 37, 40, 41, 44, 46, 61, 48, 65, 66, 97, 98]  # one byte for each value of Lut0 below 128
        p2s = [0, 33, 48, 97]                                                   # and for each value of Lut1
        for a in p1s:
            for b in p2s:
                lits += bytes([b, a, (a * 7 + b) & 255])
        lits += bytes([0x80, 0x41, 0x81, 0x41, 0xC0, 0x41, 0xC1, 0x41, 0xE1, 0xE2, 0x41])  # the continuation and lead bytes
    else:
        reps = [0, 7, 40, 100, 150, 200, 250, 255]
        for a in reps:
            for b in reps:
                lits += bytes([b, a, (a + 3 * b) & 255])
    return bytes(lits)


def _context_modes(out):
    for mode in (1, 2, 3):
        s = W.Stream(16)
        s.compressed([(_mode_literals(mode), None)], islast=True, modes=[mode], lmap=[(5 * c + 3) % 64 for c in range(64)], ntl=64)
        assert "mode_%s_ctx64" % W.MODE_NAMES[mode] in s.tags
        out.append(("mode_%s_64_trees" % W.MODE_NAMES[mode], s))
    # MSB6 alone on a handful of bytes: a stream small enough for the cut and streaming tests
    s = W.Stream(16)
    s.compressed([(bytes([0x10, 0xF3, 0x41, 0x83, 0xC2, 0x07, 0xFF]), ("dist", 3, 3))], islast=True, modes=[1],
                 lmap=[c % 4 for c in range(64)], ntl=4)
    out.append(("mode_msb6_small", s))
    for mode in (2, 3):
        s = W.Stream(16)
        s.compressed([(bytes([0x10, 0xF3, 0x41, 0x20, 0x61, 0xC2, 0x00, 0xFF, 0xFF]), ("dist", 3, 3))], islast=True, modes=[mode],
                     lmap=[(c >> 2 if mode == 2 else c >> 3 ^ c) % 4 for c in range(64)], ntl=4)
        out.append(("mode_%s_small" % W.MODE_NAMES[mode], s))
    # two block types, MSB6 and SIGNED, switched to and fro; then UTF8 and LSB6
    s = W.Stream(16)
    lits = _mode_literals(1)[:60] + _mode_literals(3)[:60]
    s.compressed([(lits, ("dist", 5, 4)), (lits[::-1], None)], nbl=(2, 1, 1), modes=[1, 3],
                 blocks=([(0, 25), (1, 30, 0), (0, 40, 0), (1, 35, 1), (0, 1000, 1)], None, None),
                 lmap=[(3 * c) % 8 for c in range(64)] + [(c >> 3) for c in range(64)], ntl=8)
    s.compressed([(lits[:50], ("dist", 5, 4)), (b"end", None)], islast=True, nbl=(2, 1, 1), modes=[2, 0],
                 blocks=([(0, 20), (1, 20), (0, 1000)], None, None), lmap=[c % 4 for c in range(128)], ntl=4)
    assert "mode_switch" in s.tags
    out.append(("mode_switches", s))
    # the first literals' context comes from an uncompressed metablock's last two bytes
    for mode in (1, 2, 3):
        s = W.Stream(16)
        s.uncompressed(b"stored \xe2\x82")
        s.compressed([(b"\xac = euro", ("dist", 4, 4))], islast=True, modes=[mode], lmap=[(7 * c + 1) % 64 for c in range(64)], ntl=64)
        assert "ctx_from_stored" in s.tags
        out.append(("mode_%s_after_stored" % W.MODE_NAMES[mode], s))


def _context_maps(out):
    """for the literal map of one block type, the distance map, and the literal map of several block types"""
    for which in ("lmap", "dmap", "lmapN"):
        size = {"lmap": 64, "dmap": 256, "lmapN": 192}[which]
        rnd = random.Random(size)
        maps = {
            # RLEMAX 1 (runs of 2 and 3), the last run ending on the last entry
            "rlemax1": ((1, False), 4, [0, 0, 1, 0, 0, 0, 2, 3, 0, 0, 0, 0, 0, 1]
                        + [rnd.choice([0, 0, 0, 1, 2, 3]) for _ in range(size - 17)] + [3, 0, 0]),
            # RLEMAX 16 declared, the inverse move-to-front, tree 255: runs of equal trees become runs of zeros
            "rlemax16_imtf": ((16, True), 256, [255] * 20 + [7] * 9 + [255, 255, 0, 0, 0, 254]
                              + [(k // 5) % 256 for k in range(size - 35)]),
            "imtf": ((0, True), 6, [rnd.choice([5, 5, 4, 0, 1, 3]) for _ in range(size)]),
            "rle": ((5, False), 256, [0] * 40 + [255] + [0] * (size - 44) + [9, 0, 0]),
            # few trees and few literals: a stream short enough for the cut-prefix and streaming tests
            "small": ((2, True), 3, [rnd.choice([0, 0, 1, 2, 2]) for _ in range(size - 6)] + [1, 1, 1, 1, 0, 0]),
        }
        for form, (enc, nt, mp) in maps.items():
            assert len(mp) == size
            s = W.Stream(16)
            cmds = []
            if which == "dmap":
                for i in range(80):
                    cmds.append((bytes([97 + i % 5]), ("dist", 1 + i % 3, 2 + i % 5)))
                cmds.append((b".", None))
                s.compressed(cmds, islast=True, nbl=(1, 1, 64), blocks=(None, None, [(k % 64, 1 + k % 3) for k in range(200)]), dmap=mp, ntd=nt,
                             dmap_enc=enc)
            else:
                lits = bytes((37 * i + i // 7) & 255 for i in range(300 if form != "small" else 40))
                nb = size // 64
                s.compressed([(lits, ("dist", 11, 7)), (b"!", None)], islast=True, nbl=(nb, 1, 1), modes=[0, 1, 3][:nb],
                             blocks=([(k % nb, (17 if form != "small" else 5) + k) for k in range(40)] if nb > 1 else None, None, None), lmap=mp, ntl=nt, lmap_enc=enc)
            out.append(("%s_%s" % (which, form), s))


def _block_switches(out):
    counts = [3, 5, 9, 13, 25, 41, 65, 16625 + 12345678]
    for c, cat in enumerate(W.CATS):
        # NBLTYPES 3: code 0 as the first switch (type 1), code 0 again (type 0), code 1 up to the last type and round to 0
        bl = [(0, 3), (1, 5, 0), (0, 9, 0), (1, 13, 1), (2, 25, 1), (0, 41, 1), (2, 65), (0, 2, 0), (2, 4, 0), (0, counts[-1], 1)]
        n = sum(b[1] for b in bl[:-1]) + 20
        rnd = random.Random(c)
        if c == 0:
            cmds = [(bytes(rnd.randrange(97, 101) for _ in range(n)), ("dist", 3, 5)), (b"tail", None)]
        elif c == 1:
            cmds = [(bytes([97 + i % 3] * (1 + i % 3)), ("dist", 1 + i % 2, 2 + i % 4)) for i in range(n)] + [(b".", None)]
        else:
            cmds = [(bytes([97 + i % 3]), ("dist", 1 + i % 4, 2 + i % 2)) for i in range(n)] + [(b".", None)]
        nbl = [1, 1, 1]
        nbl[c] = 3
        blocks = [None, None, None]
        blocks[c] = bl
        s = W.Stream(16)
        kw = {}
        if c == 0:
            kw = dict(lmap=[0] * 64 + [1] * 64 + [2] * 64, ntl=3, modes=[0, 0, 0])
        elif c == 2:
            kw = dict(dmap=[0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2], ntd=3)
        s.compressed(cmds, islast=True, nbl=tuple(nbl), blocks=tuple(blocks), **kw)
        out.append(("switches_%s" % cat, s))
        # NBLTYPES 2: code 0 and code 1 both give the other type
        bl = [(0, 2), (1, 3, 0), (0, 4, 0), (1, 6, 1), (0, 1 << 20, 1)]
        nbl[c] = 2
        blocks[c] = bl
        s = W.Stream(16)
        if c == 0:
            kw = dict(lmap=[0] * 64 + [1] * 64, ntl=2, modes=[0, 0])
            cmds = [(b"abababbabaabbbab" * 2, None)]
        elif c == 2:
            kw = dict(dmap=[0, 0, 0, 0, 1, 1, 1, 1], ntd=2)
        if c:
            cmds = cmds[:24] + [(b".", None)]
        s.compressed(cmds, islast=True, nbl=tuple(nbl), blocks=tuple(blocks), **kw)
        out.append(("switches2_%s" % cat, s))
        # NBLTYPES 256: code 1 from type to type, round from 255 to 0 and on to 1, then code 0 twice
        bl = [(0, 1)] + [(k % 256, 1, 1) for k in range(1, 258)] + [(0, 2, 0), (1, 1 << 20, 0)]
        nbl[c] = 256
        blocks[c] = bl
        s = W.Stream(16)
        if c == 0:
            kw = dict(modes=[k % 4 for k in range(256)])
            cmds = [(bytes(97 + k % 7 for k in range(270)), None)]
        elif c == 1:
            kw = {}
            cmds = [(bytes([97 + i % 3]), ("dist", 1 + i % 2, 2 + i % 4)) for i in range(270)] + [(b".", None)]
        else:
            kw = dict(dmap=[k // 4 % 2 for k in range(1024)], ntd=2)
            cmds = [(bytes([97 + i % 3]), ("dist", 1 + i % 4, 2 + i % 2)) for i in range(270)] + [(b".", None)]
        s.compressed(cmds, islast=True, nbl=tuple(nbl), blocks=tuple(blocks), **kw)
        out.append(("switches256_%s" % cat, s))


def _commands(out):
    # every cell of the insert-and-copy alphabet: (insert, copy) from the three ranges of each, with and without a distance code
    s = W.Stream(16)
    lit = lambda n: bytes(97 + (k * k) % 23 for k in range(n))
    cmds = [(lit(5), ("dist", 2, 3)), (lit(3), ("last", 4)), (lit(0), ("last", 12)), (lit(2), ("dist", 7, 9)), (lit(0), ("dist", 9, 40)),
            (lit(12), ("dist", 5, 6)), (lit(100), ("dist", 90, 60)), (lit(7), ("dist", 33, 75)), (lit(131), ("dist", 64, 8)),
            (lit(20), ("dist", 6, 300)), (lit(200), ("dist", 150, 11)), (lit(140), ("dist", 13, 71)), (lit(4), None)]
    s.compressed(cmds, islast=True)
    assert all("cell%d" % k in s.tags for k in range(11))
    out.append(("cells", s))
    # insert code 23 through a literal tree of one symbol, copy code 23 from distance 1: the metablock ends after the copy
    s = W.Stream(16)
    s.compressed([(b"a" * 22594, ("dist", 1, 2118))], islast=True)
    out.append(("insert23_copy23", s))
    s = W.Stream(16)
    s.compressed([(b"ab", ("dist", 2, 3000)), (b"", ("dist", 1, 2118 + 70000))], islast=True)
    out.append(("copy23_long", s))
    s = W.Stream(16)
    s.compressed([(b"abc", ("dist", 3, 5))])
    s.compressed([(b"", ("last", 4)), (b"", ("dist", 2, 2))])
    s.compressed([(b"xyz", None)], islast=True)
    out.append(("ends_and_insert0", s))


def _distances(out):
    # every ring code, with what it does to the ring; a dictionary reference and code 0 leave the ring as it is
    s = W.Stream(16)
    cmds = [(_varied(40, 5), ("dist", 20, 4))]
    for dc in range(16):  # behind two known distances, so that each code's own distance is a back reference
        cmds += [(b"", ("dist", 21 + dc, 3)), (b"", ("dist", 30 + dc, 3)), (b"r", ("code", dc, 3 + dc % 3))]
    for dc in (3, 2, 1, 0, 15, 9, 4):  # and one after the other on the ring they leave
        cmds.append((b"r", ("code", dc, 3 + dc % 3)))
    cmds.append((b"", ("dist", 1000, 4)))  # far beyond the output so far: a dictionary word
    cmds += [(b"", ("code", 0, 3)), (b"", ("code", 1, 3)), (b"s", ("last", 2)), (b"", ("code", 3, 5)), (b"t", None)]
    s.compressed(cmds)
    # the ring goes on into the next metablock
    s.compressed([(b"u", ("code", 1, 4)), (b"", ("code", 2, 3)), (b"", ("code", 3, 3)), (b"", ("last", 3)), (b"", ("code", 10, 4))],
                 islast=True)
    assert all("ring_code%d" % k in s.tags for k in range(16)) and "ring_carried" in s.tags
    out.append(("ring_codes", s))
    # WBITS 10 with more than 1008 bytes of output: distance 1008 reaches back, 1009 is dictionary word 0, transform 0
    s = W.Stream(10)
    s.uncompressed(_varied(1100, 6))
    s.compressed([(b"", ("dist", 1008, 5)), (b"", ("dist", 1009, 4)), (b"x", ("dist", 1008, 1100)), (b"", ("dist", 1010, 4)),
                  (b"", ("last", 6))], islast=True)
    assert {"edge_window_back", "edge_window_dict"} <= s.tags
    out.append(("window_edge_wbits10", s))
    # the same edge while the position is below the window
    s = W.Stream(10)
    s.compressed([(_varied(50, 7), ("dist", 50, 6)), (b"", ("dist", 57, 4)), (b"", ("dist", 60, 60)), (b"", ("dist", 121, 5)),
                  (b"y", None)], islast=True)
    assert {"edge_pos_back", "edge_pos_dict"} <= s.tags
    out.append(("position_edge", s))
    # overlapping copies: the three branches of the copy (distance >= length is in every other case)
    s = W.Stream(16)
    cmds = [(_varied(70, 8), ("dist", 1, 10))]
    for d, n in ((63, 200), (64, 200), (65, 200), (2, 129), (1, 64), (64, 65), (65, 66), (63, 64), (3, 5), (40, 64)):
        cmds.append((b"o", ("dist", d, n)))
    s.compressed(cmds, islast=True)
    out.append(("overlaps", s))


def _find_word(pred, lens=range(4, 25)):
    d = W.dictionary()
    for n in lens:
        for k in range(1 << W.NDBITS[n]):
            w = d[W.DICT_OFFSET[n] + k * n:][:n]
            if pred(w):
                return n, k
    raise LookupError


def _mb_end(word):
    i = 0
    while i < len(word):
        step = 1 if word[i] < 0xC0 else 2 if word[i] < 0xE0 else 3
        if step > 1 and i + step > len(word):
            return True
        i += step
    return False


def _dictionary(out):
    first = [t for t in range(121) if W.transform_kind(t) == "first"]
    every = [t for t in range(121) if W.transform_kind(t) == "all"]
    empty = [t for t in range(121) if W.transform(b"abcd", t) == b""]
    s = W.Stream(16)
    cmds, pos = [], [0]

    def ref(n, k, t, lits=b""):
        pos[0] += len(lits)
        d = min(pos[0], (1 << 16) - 16) + 1 + (t << W.NDBITS[n]) + k
        cmds.append((lits, ("dist", d, n)))
        w = W.dictionary()[W.DICT_OFFSET[n] + k * n:][:n]
        pos[0] += len(W.transform(w, t))
    ref(4, 5, 0, b"dictionary: ")
    ref(24, 3, 0)
    ref(4, 9, empty[0])                      # omits more than the word holds: no output
    ref(24, (1 << W.NDBITS[24]) - 1, 120)    # the last transform, the last word
    ref(4, (1 << W.NDBITS[4]) - 1, 120)
    for lo, hi in ((0xC0, 0xE0), (0xE0, 0x100)):
        n, k = _find_word(lambda w: lo <= w[0] < hi)
        for t in (first[0], first[-1], every[0], every[-1]):
            ref(n, k, t)
    n, k = _find_word(_mb_end)               # a multi-byte character that runs past the word's end
    for t in every[:3] + first[:1]:
        ref(n, k, t)
    n, k = _find_word(lambda w: w[-2] >= 0xC0 and w[-2] < 0xE0 and w[-3] < 0x80)  # one that ends exactly with the word
    ref(n, k, every[1])
    cmds.append((b".", None))
    s.compressed(cmds, islast=True)
    need = {"dict_len4", "dict_len24", "dict_empty", "dict_t120", "dict_last_index", "dict_upfirst_c0", "dict_upfirst_e0", "dict_upall_c0",
            "dict_upall_e0", "dict_upall_mb_end"}
    assert need <= s.tags, need - s.tags
    out.append(("dictionary_words", s))


# ---------------------------------------------------------------- error forms

def _head(s, mlen=1, islast=True, nbl0=1, pd=0):
    """a compressed metablock's header up to the context modes: one block type in every category (nbl0: NBLTYPESL is written and
    its codes are the caller's), the byte of NPOSTFIX and NDIRECT, mode LSB6"""
    w = s.w
    w.put(int(islast), 1)
    if islast:
        w.put(0, 1)
    s._mlen(mlen)
    if not islast:
        w.put(0, 1)
    if nbl0 > 1:
        W.varlen8(w, nbl0 - 1)
        return
    for _ in range(3):
        W.varlen8(w, 0)
    w.put(pd, 6)
    w.put(0, 2)


def _trees(s, ntl=1, ntd=1):
    W.varlen8(s.w, ntl - 1)
    W.varlen8(s.w, ntd - 1)


def _errors(out):
    def err(name, s, code, cut=None):
        s.tags.add("err:" + name)
        out.append((name, s, ERR[code], cut))

    s = W.Stream(16)
    s.put(0, 1), s.put(3, 2), s.put(1, 1)
    err("reserved", s, "RESERVED")
    for nib in (5, 6):
        s = W.Stream(16)
        s.put(0, 1), s.put(nib - 4, 2), s.put(0x0FFF, 4 * nib)
        err("exuberant_nibble_%d" % nib, s, "EXUBERANT_NIBBLE")
    for nb in (2, 3):
        s = W.Stream(16)
        s.put(0, 1), s.put(3, 2), s.put(0, 1), s.put(nb, 2), s.put(0x00FF, 8 * nb)
        err("exuberant_meta_nibble_%d" % nb, s, "EXUBERANT_META_NIBBLE")
    s = W.Stream(16)
    s.put(0, 1), s.put(3, 2), s.put(0, 1), s.put(1, 2), s.put(2, 8), s.put(1, 1)
    s.w.put_bytes(b"abc")
    err("padding_1_metadata", s, "PADDING_1")
    s = W.Stream(16)
    s.put(0, 1), s.put(0, 2), s.put(2, 16), s.put(1, 1), s.put(1, 3)
    s.w.put_bytes(b"abc")
    err("padding_1_uncompressed", s, "PADDING_1")
    s = W.Stream(16)
    s.put(1, 1), s.put(1, 1), s.put(16, 5)
    err("padding_2_last_empty", s, "PADDING_2")
    s = W.Stream(16)
    s.compressed([(b"abc", ("dist", 1, 2))], islast=True, codes={("lit", 0): W.simple(3)})
    assert s.w.bitpos() % 8 not in (0, 7)
    s.put(2, 2)
    err("padding_2_compressed", s, "PADDING_2")
    s = W.Stream(16)
    s.w = W.Bits()
    s.put(1, 1), s.put(0, 3), s.put(1, 3), s.put(0, 9)
    err("window_bits", s, "WINDOW_BITS")

    # SIMPLE_HUFFMAN_ALPHABET: a symbol of the alphabet's size, in every alphabet whose size is no power of two
    one = lambda sym, alpha: W.Simple([sym], alpha, check=False)
    s = W.Stream(16)
    _head(s), _trees(s)
    one(65, 256).write_def(s.w), one(704, 704).write_def(s.w), s.put(0, 8)
    err("alphabet_704", s, "SIMPLE_HUFFMAN_ALPHABET")
    s = W.Stream(16)
    _head(s), _trees(s)
    one(65, 256).write_def(s.w), W.Simple([3, 2, 1023, 5], 704, check=False).write_def(s.w), s.put(0, 8)
    err("alphabet_704_third_symbol", s, "SIMPLE_HUFFMAN_ALPHABET")
    s = W.Stream(16)
    _head(s, nbl0=3)
    one(5, 5).write_def(s.w), s.put(0, 8)
    err("alphabet_nbltypes", s, "SIMPLE_HUFFMAN_ALPHABET")
    s = W.Stream(16)
    _head(s, nbl0=2)
    one(2, 4).write_def(s.w), one(26, 26).write_def(s.w), s.put(0, 8)
    err("alphabet_block_count", s, "SIMPLE_HUFFMAN_ALPHABET")
    s = W.Stream(16)
    _head(s)
    W.varlen8(s.w, 1), s.put(1, 1), s.put(2, 4)  # NTREESL 2, RLEMAX 3: five symbols
    one(6, 5).write_def(s.w), s.put(0, 8)
    err("alphabet_context_map", s, "SIMPLE_HUFFMAN_ALPHABET")
    s = W.Stream(16)
    _head(s, pd=3 | (120 >> 3 << 2)), _trees(s)
    one(65, 256).write_def(s.w), one(130, 704).write_def(s.w), one(520, 520).write_def(s.w), s.put(0, 8)
    err("alphabet_distance_520", s, "SIMPLE_HUFFMAN_ALPHABET")

    # SIMPLE_HUFFMAN_SAME: the equal pair at every position of NSYM 2, 3, 4
    for n in (2, 3, 4):
        for i in range(n):
            for j in range(i + 1, n):
                syms = [65, 66, 67, 68][:n]
                syms[j] = syms[i]
                s = W.Stream(16)
                _head(s), _trees(s)
                W.Simple(syms, 256, check=False).write_def(s.w), s.put(0, 8)
                err("same_%d_%d%d" % (n, i, j), s, "SIMPLE_HUFFMAN_SAME")

    def cl(s, values, hskip=0):
        s.put(hskip, 2)
        for v in values:
            s.put(*W.CL_FIXED[v])
    for name, values in (("all_zero", [0] * 18), ("over", [2, 2, 2, 1]), ("space_left", [2, 2] + [0] * 16), ("all_zero_hskip3", [0] * 15)):
        s = W.Stream(16)
        _head(s), _trees(s)
        cl(s, values, 3 if "hskip" in name else 0), s.put(0, 16)
        err("cl_space_" + name, s, "CL_SPACE")

    def bad_code(name, tokens, clens):
        s = W.Stream(16)
        _head(s), _trees(s)
        W.Complex({0: 8}, 256, tokens=tokens, cl=clens, check=False).write_def(s.w)
        s.put(0, 16)
        err("huffman_space_" + name, s, "HUFFMAN_SPACE")
    bad_code("single_9", [(9, 0)] * 256, {9: 1})                         # 256 lengths of 9 fill half the space
    bad_code("repeat_past_end", [(8, 0)] + [(16, 3)] * 6, {8: 1, 16: 1})  # the chain reaches 342 repeats at its fourth link
    bad_code("zeros_past_end", [(1, 0), (17, 7), (17, 7), (17, 7)], {1: 1, 17: 1})  # 10, 74, 586 zeros behind one length
    bad_code("over", [(1, 0), (2, 0), (1, 0)] + [(0, 0)] * 253, {1: 1, 2: 2, 0: 2})  # the third length overshoots
    bad_code("space_left", [(1, 0)] + [(0, 0)] * 255, {0: 1, 1: 1})

    s = W.Stream(16)
    _head(s)
    W.varlen8(s.w, 1), s.put(1, 1), s.put(0, 4)  # NTREESL 2, RLEMAX 1
    W.Simple([1], 3).write_def(s.w)              # every symbol is the run code 1, read in no bits
    for _ in range(21):
        s.put(1, 1)                              # 21 runs of 3
    s.put(0, 1), s.put(0, 16)                    # and one of 2: 65 entries in a map of 64
    err("context_map_repeat_literal", s, "CONTEXT_MAP_REPEAT")
    s = W.Stream(16)
    _head(s)
    W.varlen8(s.w, 0), W.varlen8(s.w, 1), s.put(1, 1), s.put(1, 4)  # NTREESD 2, RLEMAX 2
    W.Simple([2], 4).write_def(s.w)
    s.put(1, 2), s.put(0, 16)                    # a run of 5 in a map of 4
    err("context_map_repeat_distance", s, "CONTEXT_MAP_REPEAT")

    s = W.Stream(16)
    s.compressed([(b"ab", None)], islast=True, mlen=1)
    err("block_length_2_insert", s, "BLOCK_LENGTH_2")
    s = W.Stream(16)
    s.compressed([(b"ab", ("dist", 1, 4))], islast=True, mlen=3)
    err("block_length_2_copy", s, "BLOCK_LENGTH_2")
    s = W.Stream(16)
    s.compressed([(b"ab", ("dist", 3, 4))], islast=True, mlen=3)
    err("block_length_2_dictionary", s, "BLOCK_LENGTH_2")
    # the input ends inside literals that already passed MLEN: what libbrotlidec flushes then fails
    s = W.Stream(16)
    s.compressed([(b"abcdabcdab", None), (b"dcba", None)], islast=True, mlen=1)
    err("block_length_1_input_ends", s, "BLOCK_LENGTH_1", cut=-2)
    # behind 1020 stored bytes the insert, the copy or the dictionary word passes MLEN and crosses the 1024 bytes of
    # libbrotlidec's ring buffer, which is flushed there
    for name, cmds in (("insert", [(b"abcdabcdab", None)]), ("copy", [(b"a", ("dist", 1, 10))]), ("dictionary", [(b"a", ("dist", 1022, 4))])):
        s = W.Stream(16)
        s.uncompressed(_varied(1020, 9))
        s.compressed(cmds, islast=True, mlen=1 if name == "insert" else 2)
        err("block_length_1_ring_" + name, s, "BLOCK_LENGTH_1")

    s = W.Stream(16)
    s.compressed([(b"A", ("dist", 1, 2)), (b"", ("code", 4, 2))], islast=True, mlen=5)
    err("distance_code4", s, "DISTANCE")
    s = W.Stream(16)
    s.compressed([(b"AB", ("dist", 2, 2)), (b"", ("dist", 1, 2)), (b"", ("code", 14, 2))], islast=True, mlen=8)  # second last 2, minus 3
    err("distance_code14", s, "DISTANCE")
    for n in (2, 3, 25):
        s = W.Stream(16)
        s.compressed([(b"", ("last", n))], islast=True, mlen=n)
        err("dictionary_length_%d" % n, s, "DICTIONARY")
    for t in (121, 127, 4000):
        s = W.Stream(16)
        s.compressed([(b"", ("dist", 1 + (t << 10), 4))], islast=True, mlen=4)
        err("transform_%d" % t, s, "TRANSFORM")


def all_cases():
    """the cases, built once"""
    global _cases
    if _cases is None:
        valid, errors = [], []
        for fn in (_wbits, _mlen_and_metadata, _simple_forms, _complex_forms, _context_modes, _context_maps, _block_switches, _commands,
                   _distances, _dictionary):
            fn(valid)
        _errors(errors)
        _cases = []
        for name, s in valid:
            assert not s.invalid, name
            comp, outp = s.finish()
            _cases.append(Case(name, comp, outp, None, frozenset(s.tags), tuple(s.bounds)))
        for name, s, code, cut in errors:
            comp, _ = s.finish()
            _cases.append(Case(name, comp[:cut] if cut else comp, None, code, frozenset(s.tags), ()))
    return _cases
