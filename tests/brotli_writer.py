"""A small brotli stream writer for hand-built test streams (RFC 7932): every prefix code, block switch, context map and command is
chosen by the test, so that features an encoder rarely emits can be pinned.  The writer also computes the output the stream
stands for; libbrotlidec decoding the stream to that output is what checks the writer."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL_ORDER = [1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15]
CL_FIXED = {0: (0, 2), 4: (1, 2), 3: (2, 2), 2: (3, 3), 1: (7, 4), 5: (15, 4)}  # value -> (bits, length) of Section 3.5
INSERT_BASE = [0, 1, 2, 3, 4, 5, 6, 8, 10, 14, 18, 26, 34, 50, 66, 98, 130, 194, 322, 578, 1090, 2114, 6210, 22594]
INSERT_EXTRA = [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24]
COPY_BASE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 18, 22, 30, 38, 54, 70, 102, 134, 198, 326, 582, 1094, 2118]
COPY_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24]
CELLS = [(0, 0), (0, 8), (0, 0), (0, 8), (8, 0), (8, 8), (0, 16), (16, 0), (8, 16), (16, 8), (16, 16)]
BLEN_BASE = [1, 5, 9, 13, 17, 25, 33, 41, 49, 65, 81, 97, 113, 145, 177, 209, 241, 305, 369, 497, 753, 1265, 2289, 4337, 8433, 16625]
BLEN_EXTRA = [2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13, 24]
NDBITS = [0, 0, 0, 0, 10, 10, 11, 11, 10, 10, 10, 10, 10, 9, 9, 8, 7, 7, 8, 7, 7, 6, 6, 5, 5]
DICT_OFFSET = [0, 0, 0, 0, 0, 4096, 9216, 21504, 35840, 44032, 53248, 63488, 74752, 87040, 93696, 100864, 104704, 106752, 108928,
               113536, 115968, 118528, 119872, 121280, 122016]

_dict = None
_tr = None


def dictionary():
    global _dict
    if _dict is None:
        with open(os.path.join(ROOT, "compu_amd", "csrc", "brotli_dict.bin"), "rb") as f:
            _dict = f.read()
    return _dict


def transform(word, tidx):
    """BrotliTransformDictionaryWord of the system's libbrotlicommon"""
    global _tr
    c = C.CDLL("libbrotlicommon.so.1")
    if _tr is None:
        c.BrotliGetTransforms.restype = C.c_void_p
        _tr = c.BrotliGetTransforms()
    c.BrotliTransformDictionaryWord.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int]
    dst = C.create_string_buffer(64)
    n = c.BrotliTransformDictionaryWord(dst, word, len(word), _tr, tidx)
    return dst.raw[:n]


class Bits:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        for i in range(n):
            self.bits.append((v >> i) & 1)

    def put_code(self, code, n):  # a prefix code is read from its most significant bit
        for i in range(n - 1, -1, -1):
            self.bits.append((code >> i) & 1)

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + j] << j for j in range(8)) for i in range(0, len(b), 8))


def complete_lengths(syms):
    """a complete prefix code over the symbols (sorted): lengths L-1 and L"""
    syms = sorted(set(syms))
    k = len(syms)
    if k == 1:
        return {syms[0]: 0}
    L = (k - 1).bit_length()
    short = 2 ** L - k
    return {s: (L - 1 if i < short else L) for i, s in enumerate(syms)}


def canonical(lengths):
    codes, code, prev = {}, 0, 0
    for s, ln in sorted(((s, ln) for s, ln in lengths.items() if ln), key=lambda x: (x[1], x[0])):
        code <<= ln - prev
        prev = ln
        codes[s] = (code, ln)
        code += 1
    return codes


class Code:
    """a prefix code over the symbols a tree actually uses"""

    def __init__(self, syms, alpha):
        self.alpha = alpha
        self.lengths = complete_lengths(syms) if syms else {0: 0}
        self.codes = canonical(self.lengths)

    def write_def(self, w):
        if len(self.lengths) == 1:  # simple code with one symbol: reading it takes no bits
            w.put(1, 2)
            w.put(0, 2)
            w.put(next(iter(self.lengths)), (self.alpha - 1).bit_length())
            return
        last = max(self.lengths)
        seq = [self.lengths.get(s, 0) for s in range(last + 1)]
        cl = complete_lengths(set(seq))
        w.put(0, 2)  # HSKIP 0: a complex code
        if len(cl) == 1:
            for i in CL_ORDER:
                w.put(*CL_FIXED[1 if i == seq[0] else 0])
        else:
            space = 32
            for i in CL_ORDER:
                v = cl.get(i, 0)
                w.put(*CL_FIXED[v])
                if v:
                    space -= 32 >> v
                    if space == 0:
                        break
        clc = canonical(cl)
        for v in seq:
            if len(cl) > 1:
                w.put_code(*clc[v])

    def write(self, w, s):
        if len(self.lengths) > 1:
            w.put_code(*self.codes[s])


def varlen8(w, v):
    if v == 0:
        w.put(0, 1)
        return
    w.put(1, 1)
    n = v.bit_length() - 1
    w.put(n, 3)
    if n:
        w.put(v - (1 << n), n)


def _code_of(n, base, extra):
    for c in range(len(base) - 1, -1, -1):
        if base[c] <= n:
            assert n - base[c] < (1 << extra[c])
            return c, n - base[c], extra[c]


def encode_distance(d, npostfix, ndirect):
    """(distance code, extra bits, their count) of distance d"""
    if d <= ndirect:
        return 15 + d, 0, 0
    x = d - ndirect - 1
    lcode, y = x & ((1 << npostfix) - 1), x >> npostfix
    for hcode in range(48):
        nb = 1 + (hcode >> 1)
        off = ((2 + (hcode & 1)) << nb) - 4
        if off <= y < off + (1 << nb):
            return 16 + ndirect + (hcode << npostfix) + lcode, y - off, nb
    raise ValueError(d)


class Stream:
    """A brotli stream under construction; `out` is the output it stands for."""

    def __init__(self, wbits=16):
        self.w = Bits()
        self.wbits = wbits
        self.out = bytearray()
        self.ring = [16, 15, 11, 4]  # ring[-1] is the last distance
        if wbits == 16:
            self.w.put(0, 1)
        elif wbits > 17:
            self.w.put(1, 1)
            self.w.put(wbits - 17, 3)
        else:
            self.w.put(1, 1)
            self.w.put(0, 3)
            self.w.put(0 if wbits == 17 else wbits - 8, 3)

    def _mlen(self, mlen):
        nib = max(4, (max(mlen - 1, 1).bit_length() + 3) // 4)
        self.w.put(nib - 4, 2)
        self.w.put(mlen - 1, 4 * nib)

    def metadata(self, payload, islast=False):
        self.w.put(int(islast), 1)
        if islast:
            self.w.put(0, 1)
        self.w.put(3, 2)
        self.w.put(0, 1)
        n = len(payload)
        nb = 0 if n == 0 else ((n - 1).bit_length() + 7) // 8 or 1
        self.w.put(nb, 2)
        if nb:
            self.w.put(n - 1, 8 * nb)
        self.w.align()
        for b in payload:
            self.w.put(b, 8)

    def uncompressed(self, data):
        self.w.put(0, 1)
        self._mlen(len(data))
        self.w.put(1, 1)
        self.w.align()
        for b in data:
            self.w.put(b, 8)
        self.out += data

    def last_empty(self):
        self.w.put(1, 1)
        self.w.put(1, 1)

    def compressed(self, cmds, islast=False, nbl=(1, 1, 1), blocks=(None, None, None), npostfix=0, ndirect=0, modes=None, lmap=None,
                   ntl=1, dmap=None, ntd=1):
        """cmds: (literals, copy) with copy None (no copy: the metablock ends after the literals), ('last', n) for an implicit
        last distance, ('code', dc, n) a distance code 0..15, ('dist', d, n) a distance.  blocks[c]: list of (type, count), the
        first type 0; None = one block type.  Literal context mode LSB6 unless given."""
        modes = modes or [0] * nbl[0]
        lmap = lmap or [0] * (64 * nbl[0])
        dmap = dmap or [0] * (4 * nbl[2])
        dalpha = 16 + ndirect + (48 << npostfix)
        blocks = [list(b) if b else [(0, 1 << 24)] for b in blocks]
        ev = []  # ('bs', c, typecode, lencode, extra, nextra) / (cat, tree, sym, extra, nextra)
        used = {}
        cur = [[0, blocks[c][0][1], 0] for c in range(3)]  # type, left, next block index
        prev_t = [[1, 0] for _ in range(3)]  # second last, last

        def use(key, s):
            used.setdefault(key, set()).add(s)

        def sym(c):
            if cur[c][1] == 0:
                cur[c][2] += 1
                t, n = blocks[c][cur[c][2]]
                code = t + 2
                lc, le, ln = _code_of(n, BLEN_BASE, BLEN_EXTRA)
                use(("bt", c), code)
                use(("bl", c), lc)
                ev.append(("bs", c, code, lc, le, ln))
                prev_t[c] = [prev_t[c][1], t]
                cur[c][0], cur[c][1] = t, n
            cur[c][1] -= 1
            return cur[c][0]

        first_len = []
        for c in range(3):
            if nbl[c] >= 2:
                lc, le, ln = _code_of(blocks[c][0][1], BLEN_BASE, BLEN_EXTRA)
                use(("bl", c), lc)
                first_len.append((lc, le, ln))
            else:
                first_len.append(None)
        start = len(self.out)
        for lits, copy in cmds:
            t = sym(1)
            icode, ie, inb = _code_of(len(lits), INSERT_BASE, INSERT_EXTRA)
            clen = copy[-1] if copy else 2
            ccode, ce, cnb = _code_of(clen, COPY_BASE, COPY_EXTRA)
            if copy and copy[0] == "last" and icode < 8 and ccode < 16:
                cmd = (64 if ccode >= 8 else 0) + (icode << 3) + (ccode & 7)
            else:
                cell = next(k for k in range(2, 11) if CELLS[k] == (icode & ~7, ccode & ~7))
                cmd = cell * 64 + ((icode & 7) << 3) + (ccode & 7)
            use(("ic", t), cmd)
            ev.append((("ic", t), cmd, ie, inb, ce, cnb))
            for b in lits:
                lt = sym(0)
                p1 = self.out[-1] if self.out else 0
                tree = lmap[64 * lt + (p1 & 63)] if modes[lt] == 0 else None
                assert tree is not None, "the writer keeps to LSB6"
                use(("lit", tree), b)
                ev.append((("lit", tree), b, 0, 0))
                self.out.append(b)
            if copy is None:
                continue
            max_dist = min(len(self.out), (1 << self.wbits) - 16)
            if copy[0] == "last" and cmd < 128:
                d, push = self.ring[-1], False
            else:
                dt = sym(2)
                tree = dmap[4 * dt + (3 if clen > 4 else clen - 2)]
                if copy[0] in ("code", "last"):
                    dc = 0 if copy[0] == "last" else copy[1]
                    de = dnb = 0
                    base = [self.ring[-1], self.ring[-2], self.ring[-3], self.ring[-4]]
                    if dc < 4:
                        d = base[dc]
                    else:
                        k = dc - 4 if dc < 10 else dc - 10
                        d = (base[0] if dc < 10 else base[1]) + ((k >> 1) + 1) * (1 if k & 1 else -1)
                else:
                    d = copy[1]
                    dc, de, dnb = encode_distance(d, npostfix, ndirect)
                push = dc != 0
                use(("d", tree), dc)
                ev.append((("d", tree), dc, de, dnb))
            if d > max_dist:
                addr = d - max_dist - 1
                widx, tidx = addr & ((1 << NDBITS[clen]) - 1), addr >> NDBITS[clen]
                word = dictionary()[DICT_OFFSET[clen] + widx * clen:][:clen]
                self.out += transform(word, tidx)
            else:
                if push:
                    self.ring.append(d)
                for _ in range(clen):
                    self.out.append(self.out[-d])
        mlen = len(self.out) - start
        w = self.w
        w.put(int(islast), 1)
        if islast:
            w.put(0, 1)
        self._mlen(mlen)
        if not islast:
            w.put(0, 1)
        codes = {}
        for c in range(3):
            varlen8(w, nbl[c] - 1)
            if nbl[c] >= 2:
                codes[("bt", c)] = Code(used.get(("bt", c), {2}), nbl[c] + 2)
                codes[("bl", c)] = Code(used[("bl", c)], 26)
                codes[("bt", c)].write_def(w)
                codes[("bl", c)].write_def(w)
                lc, le, ln = first_len[c]
                codes[("bl", c)].write(w, lc)
                w.put(le, ln)
        w.put(npostfix | ((ndirect >> npostfix) << 2), 6)
        for m in modes:
            w.put(m, 2)
        for mp, nt in ((lmap, ntl), (dmap, ntd)):
            varlen8(w, nt - 1)
            if nt >= 2:
                w.put(0, 1)  # no run lengths
                cm = Code(set(mp), nt)
                cm.write_def(w)
                for v in mp:
                    cm.write(w, v)
                w.put(0, 1)  # no inverse move-to-front
        for key_kind, n, alpha in (("lit", ntl, 256), ("ic", nbl[1], 704), ("d", ntd, dalpha)):
            for t in range(n):
                codes[(key_kind, t)] = Code(used.get((key_kind, t), set()), alpha)
                codes[(key_kind, t)].write_def(w)
        for e in ev:
            if e[0] == "bs":
                _, c, code, lc, le, ln = e
                codes[("bt", c)].write(w, code)
                codes[("bl", c)].write(w, lc)
                w.put(le, ln)
            elif e[0][0] == "ic":
                key, cmd, ie, inb, ce, cnb = e
                codes[key].write(w, cmd)
                w.put(ie, inb)
                w.put(ce, cnb)
            else:
                key, s, x, nx = e
                codes[key].write(w, s)
                w.put(x, nx)

    def finish(self):
        self.w.align()
        return self.w.bytes(), bytes(self.out)
