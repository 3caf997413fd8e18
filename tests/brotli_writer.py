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
        self.done = bytearray()  # whole bytes already packed (put_bytes)
        self.bits = []

    def put(self, v, n):
        for i in range(n):
            self.bits.append((v >> i) & 1)

    def put_code(self, code, n):  # a prefix code is read from its most significant bit
        for i in range(n - 1, -1, -1):
            self.bits.append((code >> i) & 1)

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def bitpos(self):
        return 8 * len(self.done) + len(self.bits)

    def put_bytes(self, data):  # at a byte boundary
        assert len(self.bits) % 8 == 0
        self.done += self._packed()
        self.bits = []
        self.done += data

    def _packed(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + j] << j for j in range(8)) for i in range(0, len(b), 8))

    def bytes(self):
        return bytes(self.done) + self._packed()


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


class Simple:
    """A simple prefix code (Section 3.4) given outright: the symbols in the order they are written and the tree-select bit.
    check=False writes symbols the format forbids (an error stream)."""

    def __init__(self, syms, alpha, tsel=0, check=True):
        self.syms, self.alpha, self.tsel = list(syms), alpha, tsel
        n = len(self.syms)
        assert 1 <= n <= 4 and (tsel == 0 or n == 4)
        if check:
            assert len(set(self.syms)) == n and all(0 <= s < alpha for s in self.syms)
        ln = {1: [0], 2: [1, 1], 3: [1, 2, 2], 4: [1, 2, 3, 3] if tsel else [2, 2, 2, 2]}[n]
        self.lengths = dict(zip(self.syms, ln))
        self.codes = canonical(self.lengths)

    def tags(self, kind):
        n = len(self.syms)
        form = f"simple{n}" + ("t" if self.tsel else "")
        t = {form, f"{form}_{kind}"}
        if n > 1 and all(a > b for a, b in zip(self.syms, self.syms[1:])):
            t.add("simple_desc")
        return t

    def write_def(self, w):
        w.put(1, 2)
        w.put(len(self.syms) - 1, 2)
        for s in self.syms:
            w.put(s, (self.alpha - 1).bit_length())
        if len(self.syms) == 4:
            w.put(self.tsel, 1)

    def write(self, w, s):
        if len(self.syms) > 1:
            w.put_code(*self.codes[s])


def chain(n, xb):
    """the extra bits of the chained repeat codes (16: xb = 2, 17: xb = 3) that stand for n repeats (Section 3.5)"""
    if n - 3 < (1 << xb):
        return [n - 3]
    return chain(((n - 3) >> xb) + 2, xb) + [(n - 3) & ((1 << xb) - 1)]


def spell_lengths(seq, spell):
    """code length tokens (symbol, extra) for the lengths seq[0 .. last non-zero]: 'plain' one token per length, 'rep' runs of
    three or more as chained 16s / 17s, 'rep1' the same without chains (a run is cut by a plain length)"""
    if spell == "plain":
        return [(v, 0) for v in seq]
    tok, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        v, n = seq[i], j - i
        if v:
            tok.append((v, 0))
            n -= 1
        xb, top = (3, 10) if v == 0 else (2, 6)
        while n >= 3:
            k = n if spell == "rep" else min(n, top)
            tok += [(17 if v == 0 else 16, e) for e in chain(k, xb)]
            n -= k
            if n:  # a plain length between two runs keeps them from chaining
                tok.append((v, 0))
                n -= 1
        tok += [(v, 0)] * n
        i = j
    return tok


def expand_tokens(tokens, alpha):
    """the decoder's side of Section 3.5: (lengths, tags of the forms met); stops where the code is complete"""
    lens, tags = [], set()
    prev, rep, rlen, space, link, last_rep = 8, 0, 0, 32768, 0, None
    seen_nonzero = False
    for sym, extra in tokens:
        assert len(lens) < alpha and space > 0, "tokens behind the end of the code"
        if sym < 16:
            rep, link, last_rep = 0, 0, None
            lens.append(sym)
            if sym:
                prev, seen_nonzero = sym, True
                space -= 32768 >> sym
            continue
        xb, nl = (2, prev) if sym == 16 else (3, 0)
        if rlen != nl or last_rep != sym:
            if last_rep is not None and last_rep != sym:
                tags.add("rep16_after17" if sym == 16 else "rep17_after16")
            rep, rlen, link = 0, nl, 0
        old = rep
        if rep:
            rep = (rep - 2) << xb
        rep += extra + 3
        link += 1
        last_rep = sym
        tags.add(f"rep{sym}")
        if link >= 2:
            tags.add(f"rep{sym}_chain")
            tags.add(f"rep{sym}_chain{min(link, 3)}")
        if sym == 16 and not seen_nonzero:
            tags.add("rep16_first")
        if sym == 17 and rep >= 64:
            tags.add("rep17_ge64")
        if sym == 17 and rep >= 138:
            tags.add("rep17_ge138")
        lens += [rlen] * (rep - old)
        if rlen:
            space -= (rep - old) << (15 - rlen)
    return lens, space, tags


class Complex:
    """A complex prefix code (Section 3.5) given outright: lengths {symbol: length}, HSKIP, and how runs are spelled -- spell
    'plain' / 'rep' / 'rep1' (spell_lengths) or the code length tokens themselves.  cl gives the code length code's own lengths
    {symbol 0..17: length}; by default it is a complete code over the symbols the tokens use."""

    def __init__(self, lengths, alpha, hskip=0, spell="plain", tokens=None, cl=None, check=True):
        self.alpha, self.hskip = alpha, hskip
        self.lengths = {s: n for s, n in lengths.items() if n}
        seq = [self.lengths.get(s, 0) for s in range(max(self.lengths) + 1)]
        self.tokens = tokens if tokens is not None else spell_lengths(seq, spell)
        self._tags = {f"hskip{hskip}"}
        if check:
            got, space, t = expand_tokens(self.tokens, alpha)
            assert space == 0 and len(got) <= alpha, (space, len(got))
            assert got[:len(seq)] == seq and not any(got[len(seq):]), "the tokens do not spell the lengths"
            self._tags |= t
        self.cl = dict(cl) if cl is not None else complete_lengths({s for s, _ in self.tokens})
        if len(self.cl) == 1:
            self.cl = {next(iter(self.cl)): 1}
            self._tags |= {"cl_single", f"cl_single_len{next(iter(self.cl))}"}
        if check:
            assert all(self.cl.get(CL_ORDER[i], 0) == 0 for i in range(hskip)), "HSKIP skips a length that is in use"
            assert all(1 <= n <= 5 for n in self.cl.values())
        self.clc = canonical(self.cl)
        self.codes = canonical(self.lengths)
        if self.lengths and max(self.lengths.values()) == 15:
            self._tags.add("depth15")
        deep = {}  # the longest code behind each 8-bit prefix: the width of its second-level table
        for code, n in self.codes.values():
            if n > 8:
                deep[code >> (n - 8)] = max(deep.get(code >> (n - 8), 0), n - 8)
        if len(set(deep.values())) >= 3:
            self._tags.add("subtable_widths3")

    def tags(self, kind):
        return self._tags | {f"complex_{kind}"}

    def write_def(self, w):
        w.put(self.hskip, 2)
        space = 32
        for i in CL_ORDER[self.hskip:]:
            v = self.cl.get(i, 0)
            w.put(*CL_FIXED[v])
            if v:
                space -= 32 >> v
                if space <= 0:
                    break
        for sym, extra in self.tokens:
            if len(self.cl) > 1:
                w.put_code(*self.clc[sym])
            if sym >= 16:
                w.put(extra, sym - 14)

    def write(self, w, s):
        w.put_code(*self.codes[s])


def simple(n, tsel=0, desc=True):
    """for Stream.compressed(codes=...): a simple code of n symbols over the symbols in use, filled up with unused ones"""
    def make(used, alpha):
        syms = sorted(used)
        assert len(syms) <= n
        syms += [s for s in range(alpha) if s not in used][: n - len(syms)]
        return Simple(sorted(syms, reverse=desc), alpha, tsel)
    return make


def complex_code(hskip=0, spell="plain", fill=0):
    """for Stream.compressed(codes=...): a complex code with the lengths of complete_lengths over the symbols in use and `fill`
    unused ones"""
    def make(used, alpha):
        syms = set(used)
        syms |= set([s for s in range(alpha) if s not in used][: max(fill, 2 - len(syms))])
        return Complex(complete_lengths(syms), alpha, hskip, spell)
    return make


# Section 7.1: the context ID of a literal from the two bytes in front of it (p1 the last).  Lut0/Lut1 (UTF8) and Lut2 (SIGNED)
# are written out from the RFC's description of their ranges, not taken from the decoder's table.
_L0_SPECIAL = {9: 4, 10: 4, 13: 4, 32: 8, 33: 12, 34: 16, 35: 12, 36: 12, 37: 20, 38: 12, 39: 16, 40: 24, 41: 28, 42: 12, 43: 12,
               44: 32, 45: 12, 46: 36, 47: 12, 58: 32, 59: 32, 60: 24, 61: 40, 62: 28, 63: 12, 64: 12, 91: 24, 92: 12, 93: 28,
               94: 12, 95: 12, 96: 12, 123: 24, 124: 12, 125: 28, 126: 12}


def _lut0(b):
    if b in _L0_SPECIAL:
        return _L0_SPECIAL[b]
    if 48 <= b <= 57:
        return 44
    if 65 <= b <= 90:
        return 48 if chr(b) in "AEIOU" else 52
    if 97 <= b <= 122:
        return 56 if chr(b) in "aeiou" else 60
    if 128 <= b <= 191:
        return b & 1
    if b >= 192:
        return 2 + (b & 1)
    return 0


def _lut1(b):
    if b < 33 or b == 127 or 128 <= b < 224:
        return 0
    if b >= 224 or 48 <= b <= 57 or 65 <= b <= 90:
        return 2
    if 97 <= b <= 122:
        return 3
    return 1


def _lut2(b):
    return 0 if b == 0 else 1 if b < 16 else 2 if b < 64 else 3 if b < 128 else 4 if b < 192 else 5 if b < 240 else 6 if b < 255 else 7


MODE_NAMES = ["lsb6", "msb6", "utf8", "signed"]


def context_id(mode, p1, p2):
    if mode == 0:
        return p1 & 63
    if mode == 1:
        return p1 >> 2
    if mode == 2:
        return _lut0(p1) | _lut1(p2)
    return (_lut2(p1) << 3) | _lut2(p2)


def encode_context_map(mp, rlemax, imtf):
    """the symbols of a context map (Section 7.3): (symbol, extra, extra bits); a tree v is symbol v + rlemax, a run of zeros of
    2^k + extra entries is symbol k <= rlemax.  With imtf the map goes through the forward move-to-front first."""
    if imtf:
        order, fwd = list(range(256)), []
        for v in mp:
            k = order.index(v)
            fwd.append(k)
            order.insert(0, order.pop(k))
        mp = fwd
    syms, i = [], 0
    while i < len(mp):
        if mp[i]:
            syms.append((mp[i] + rlemax, 0, 0))
            i += 1
            continue
        j = i
        while j < len(mp) and mp[j] == 0:
            j += 1
        n = j - i
        while n:
            k = min(rlemax, n.bit_length() - 1)
            if k == 0:
                syms.append((0, 0, 0))
                n -= 1
            else:
                r = min(n, (2 << k) - 1)
                syms.append((k, r - (1 << k), k))
                n -= r
        i = j
    return syms


def transform_kind(tidx):
    """'first' / 'all' for the uppercasing transforms, seen from what the transform does to a lowercase word"""
    t = transform(b"qwxyz", tidx)
    return "all" if b"QWXYZ" in t else "first" if b"Qwxyz" in t else None


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


CATS = ["lit", "ic", "dist"]


class Stream:
    """A brotli stream under construction; `out` is the output it stands for, `tags` the forms written so far, `bounds` the
    output positions at which a metablock ended.  `invalid` is set once a command was written that no decoder accepts."""

    def __init__(self, wbits=16):
        self.w = Bits()
        self.wbits = wbits
        self.out = bytearray()
        self.ring = [16, 15, 11, 4]  # ring[-1] is the last distance
        self.tags = {f"wbits{wbits}"}
        self.bounds = []
        self.invalid = False
        self.last_kind = None
        if wbits == 16:
            self.w.put(0, 1)
        elif wbits > 17:
            self.w.put(1, 1)
            self.w.put(wbits - 17, 3)
        else:
            self.w.put(1, 1)
            self.w.put(0, 3)
            self.w.put(0 if wbits == 17 else wbits - 8, 3)

    def put(self, v, n):
        """the raw escape: n bits of v at this point of the stream"""
        self.tags.add("raw")
        self.w.put(v, n)

    def _mlen(self, mlen, nibbles=None):
        nib = nibbles or max(4, (max(mlen - 1, 1).bit_length() + 3) // 4)
        assert 4 <= nib <= 6
        self.tags.add(f"mlen_nib{nib}")
        self.w.put(nib - 4, 2)
        self.w.put(mlen - 1, 4 * nib)

    def metadata(self, payload, islast=False, skipbytes=None):
        self.w.put(int(islast), 1)
        if islast:
            self.w.put(0, 1)
            self.tags.add("meta_last")
        self.w.put(3, 2)
        self.w.put(0, 1)
        n = len(payload)
        nb = 0 if n == 0 else ((n - 1).bit_length() + 7) // 8 or 1
        if skipbytes is not None:
            nb = skipbytes
        self.tags.add(f"mskip{nb}")
        self.w.put(nb, 2)
        if nb:
            self.w.put(n - 1, 8 * nb)
        self.w.align()
        self.w.put_bytes(payload)
        self.last_kind = "metadata"

    def uncompressed(self, data, nibbles=None):
        self.w.put(0, 1)
        self._mlen(len(data), nibbles)
        self.w.put(1, 1)
        self.w.align()
        self.w.put_bytes(data)
        self.out += data
        self.bounds.append(len(self.out))
        self.tags.add("uncompressed")
        self.last_kind = "uncompressed"

    def last_empty(self):
        if self.last_kind == "compressed" and self.w.bitpos() % 8:
            self.tags.add("last_empty_midbyte")
        self.w.put(1, 1)
        self.w.put(1, 1)

    def compressed(self, cmds, islast=False, nbl=(1, 1, 1), blocks=(None, None, None), npostfix=0, ndirect=0, modes=None, lmap=None,
                   ntl=1, dmap=None, ntd=1, codes=None, lmap_enc=None, dmap_enc=None, nibbles=None, mlen=None):
        """cmds: (literals, copy) with copy None (no copy: the metablock ends after the literals), ('last', n) for an implicit
        last distance, ('code', dc, n) a distance code 0..15, ('dist', d, n) a distance.  blocks[c]: list of (type, count) or
        (type, count, how), the first type 0; how 0 / 1 writes the switch as type code 0 (second last) / 1 (last + 1) and None
        as type + 2; None = one block type.  Literal context mode LSB6 unless given.
        codes: {key: code or function (symbols in use, alphabet size) -> code} for the prefix codes given outright (Simple,
        Complex; simple(), complex_code()), keys ('lit', t), ('ic', t), ('d', t), ('bt', c), ('bl', c), 'lmap', 'dmap'; the
        others are complete codes over the symbols in use.  lmap_enc / dmap_enc: (RLEMAX, IMTF bit) of the context map.
        nibbles: MNIBBLES; mlen: an MLEN other than what the commands produce (an error stream)."""
        modes = modes or [0] * nbl[0]
        lmap = lmap or [0] * (64 * nbl[0])
        dmap = dmap or [0] * (4 * nbl[2])
        codes = codes or {}
        dalpha = 16 + ndirect + (48 << npostfix)
        blocks = [list(b) if b else [(0, 1 << 24)] for b in blocks]
        ev = []  # ('bs', c, typecode, lencode, extra, nextra) / (cat, tree, sym, extra, nextra)
        used = {}
        tags = self.tags
        cur = [[0, blocks[c][0][1], 0] for c in range(3)]  # type, left, next block index
        prev_t = [[1, 0] for _ in range(3)]  # second last, last
        prev_how = [None] * 3
        ctx_seen = {}

        def use(key, s):
            used.setdefault(key, set()).add(s)

        def sym(c):
            if cur[c][1] == 0:
                cur[c][2] += 1
                t, n, how = (tuple(blocks[c][cur[c][2]]) + (None,))[:3]
                if how is None:
                    code = t + 2
                    tags.add(f"bt_explicit_{CATS[c]}")
                elif how == 0:
                    assert t == prev_t[c][0], "type code 0 is the second last type"
                    code = 0
                    tags.add(f"bt_code0_{CATS[c]}")
                    if cur[c][2] == 1:
                        tags.add(f"bt_code0_first_{CATS[c]}")
                    if prev_how[c] == 0:
                        tags.add(f"bt_code0_twice_{CATS[c]}")
                    if t != (prev_t[c][1] + 1) % nbl[c]:
                        tags.add(f"bt_code0_not_code1_{CATS[c]}")  # a decoder that took code 0 for code 1 goes wrong here
                else:
                    assert t == (prev_t[c][1] + 1) % nbl[c], "type code 1 is the last type + 1"
                    code = 1
                    tags.add(f"bt_code1_{CATS[c]}")
                    if t == 0:
                        tags.add(f"bt_code1_wrap_{CATS[c]}")
                    if t != prev_t[c][0]:
                        tags.add(f"bt_code1_not_code0_{CATS[c]}")
                prev_how[c] = how
                lc, le, ln = _code_of(n, BLEN_BASE, BLEN_EXTRA)
                tags.add(f"bl_code{lc}_{CATS[c]}")
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
                tags.add(f"bl_code{lc}_{CATS[c]}")
                tags.add(f"nbl{nbl[c]}_{CATS[c]}")
                use(("bl", c), lc)
                first_len.append((lc, le, ln))
            else:
                first_len.append(None)
        start = len(self.out)
        if self.last_kind == "uncompressed" and any(modes) and cmds and cmds[0][0]:
            tags.add("ctx_from_stored")
        for ci, (lits, copy) in enumerate(cmds):
            t = sym(1)
            icode, ie, inb = _code_of(len(lits), INSERT_BASE, INSERT_EXTRA)
            clen = copy[-1] if copy else 2
            ccode, ce, cnb = _code_of(clen, COPY_BASE, COPY_EXTRA)
            if copy and copy[0] == "last" and icode < 8 and ccode < 16:
                cmd = (64 if ccode >= 8 else 0) + (icode << 3) + (ccode & 7)
            else:
                cell = next(k for k in range(2, 11) if CELLS[k] == (icode & ~7, ccode & ~7))
                cmd = cell * 64 + ((icode & 7) << 3) + (ccode & 7)
            tags.add(f"cell{cmd >> 6}")
            if icode == 23:
                tags.add("insert_code23")
            if copy and ccode == 23:
                tags.add("copy_code23")
            if not lits:
                tags.add("insert0")
            use(("ic", t), cmd)
            ev.append((("ic", t), cmd, ie, inb, ce, cnb))
            for b in lits:
                lt = sym(0)
                p1 = self.out[-1] if self.out else 0
                p2 = self.out[-2] if len(self.out) > 1 else 0
                ctx = context_id(modes[lt], p1, p2)
                ctx_seen.setdefault(modes[lt], set()).add(ctx)
                tree = lmap[64 * lt + ctx]
                for m in range(4):  # a decoder that took mode m's table for this mode's would choose another tree here
                    if m != modes[lt] and lmap[64 * lt + context_id(m, p1, p2)] != tree:
                        tags.add(f"mode_{MODE_NAMES[modes[lt]]}_not_{MODE_NAMES[m]}")
                use(("lit", tree), b)
                ev.append((("lit", tree), b, 0, 0))
                self.out.append(b)
            if copy is None:
                if ci == len(cmds) - 1:
                    tags.add("end_after_literals")
                continue
            if ci == len(cmds) - 1:
                tags.add("end_after_copy")
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
                    tags.add(f"ring_code{dc}")
                else:
                    d = copy[1]
                    dc, de, dnb = encode_distance(d, npostfix, ndirect)
                push = dc != 0
                use(("d", tree), dc)
                ev.append((("d", tree), dc, de, dnb))
            if d <= 0:
                self.invalid = True
                tags.add("bad_ring_distance")
            elif d > max_dist:
                addr = d - max_dist - 1
                if not 4 <= clen <= 24 or addr >> NDBITS[clen] > 120:
                    self.invalid = True
                    tags.add("bad_dictionary_reference")
                    continue
                widx, tidx = addr & ((1 << NDBITS[clen]) - 1), addr >> NDBITS[clen]
                word = dictionary()[DICT_OFFSET[clen] + widx * clen:][:clen]
                piece = transform(word, tidx)
                self.out += piece
                tags.update({"dict", f"dict_len{clen}"})
                if d == max_dist + 1:
                    tags.add("edge_window_dict" if max_dist == (1 << self.wbits) - 16 else "edge_pos_dict")
                if not piece:
                    tags.add("dict_empty")
                if tidx == 120:
                    tags.add("dict_t120")
                if widx == (1 << NDBITS[clen]) - 1:
                    tags.add("dict_last_index")
                kind = transform_kind(tidx)
                if kind and word[0] >= 0xC0:
                    tags.add(f"dict_up{kind}_{'e0' if word[0] >= 0xE0 else 'c0'}")
                if kind == "all":
                    i = 0
                    while i < clen:
                        step = 1 if word[i] < 0xC0 else 2 if word[i] < 0xE0 else 3
                        if step > 1 and i + step >= clen:
                            tags.add("dict_upall_mb_end")
                        i += step
            else:
                if d == max_dist:
                    tags.add("edge_window_back" if max_dist == (1 << self.wbits) - 16 else "edge_pos_back")
                if clen > d and d in (1, 63, 64, 65):
                    tags.add(f"overlap_d{d}")
                if push:
                    self.ring.append(d)
                for _ in range(clen):
                    self.out.append(self.out[-d])
        for m, seen in ctx_seen.items():
            tags.add(f"mode_{MODE_NAMES[m]}")
            if len(seen) == 64:
                tags.add(f"mode_{MODE_NAMES[m]}_ctx64")
        if len(set(modes)) > 1 and len(ctx_seen) > 1:
            tags.add("mode_switch")
        if start and self.ring != [16, 15, 11, 4] and any(c and c[0] in ("code", "last") for _, c in cmds):
            tags.add("ring_carried")
        w = self.w
        w.put(int(islast), 1)
        if islast:
            w.put(0, 1)
        if mlen is not None:
            tags.add("mlen_override")
        self._mlen(len(self.out) - start if mlen is None else mlen, nibbles)
        if not islast:
            w.put(0, 1)
        built = {}

        def code_for(key, syms, alpha, kind):
            spec = codes.get(key)
            if spec is None:
                return Code(syms, alpha)
            if not hasattr(spec, "write_def"):
                spec = spec(set(syms), alpha)
            assert spec.alpha == alpha and set(syms) <= set(spec.lengths), (key, syms)
            tags.update(spec.tags(kind))
            return spec

        for c in range(3):
            varlen8(w, nbl[c] - 1)
            if nbl[c] >= 2:
                built[("bt", c)] = code_for(("bt", c), used.get(("bt", c), {2}), nbl[c] + 2, "bt")
                built[("bl", c)] = code_for(("bl", c), used[("bl", c)], 26, "bl")
                built[("bt", c)].write_def(w)
                built[("bl", c)].write_def(w)
                lc, le, ln = first_len[c]
                built[("bl", c)].write(w, lc)
                w.put(le, ln)
        w.put(npostfix | ((ndirect >> npostfix) << 2), 6)
        for m in modes:
            w.put(m, 2)
        for name, mp, nt, enc in (("lmap", lmap, ntl, lmap_enc), ("dmap", dmap, ntd, dmap_enc)):
            varlen8(w, nt - 1)
            if nt >= 2:
                rlemax, imtf = enc or (0, False)
                which = "lmapN" if name == "lmap" and nbl[0] > 1 else name
                w.put(int(rlemax > 0), 1)
                if rlemax:
                    w.put(rlemax - 1, 4)
                    tags.add(f"rlemax{rlemax}_{which}")
                syms = encode_context_map(mp, rlemax, imtf)
                if 0 < syms[-1][0] <= rlemax:
                    tags.add(f"cm_run_to_end_{which}")
                if imtf:
                    tags.add(f"imtf_{which}")
                if imtf and any(0 < s <= rlemax for s, _, _ in syms):
                    tags.add(f"rle_imtf_{which}")
                if 255 in mp:
                    tags.add(f"tree255_{which}")
                cm = code_for(name, {s for s, _, _ in syms}, nt + rlemax, "cmap")
                cm.write_def(w)
                for s, e, nb in syms:
                    cm.write(w, s)
                    w.put(e, nb)
                w.put(int(imtf), 1)
        for key_kind, n, alpha in (("lit", ntl, 256), ("ic", nbl[1], 704), ("d", ntd, dalpha)):
            for t in range(n):
                built[(key_kind, t)] = code_for((key_kind, t), used.get((key_kind, t), set()), alpha, {"d": "dist"}.get(key_kind, key_kind))
                built[(key_kind, t)].write_def(w)
        for e in ev:
            if e[0] == "bs":
                _, c, code, lc, le, ln = e
                built[("bt", c)].write(w, code)
                built[("bl", c)].write(w, lc)
                w.put(le, ln)
            elif e[0][0] == "ic":
                key, cmd, ie, inb, ce, cnb = e
                built[key].write(w, cmd)
                w.put(ie, inb)
                w.put(ce, cnb)
            else:
                key, s, x, nx = e
                built[key].write(w, s)
                w.put(x, nx)
        self.bounds.append(len(self.out))
        self.last_kind = "compressed"

    def finish(self):
        self.w.align()
        return self.w.bytes(), bytes(self.out)
