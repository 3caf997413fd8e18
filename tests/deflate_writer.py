"""A small DEFLATE writer for hand-built test streams (RFC 1951, with the RFC 1950 / 1952 wrappers): block types, the code lengths of
all three alphabets, the code-length symbol sequence, the length and distance symbols and extra bits of every token are chosen by
the test, so that the forms zlib's encoder never emits can be pinned.  The writer also computes the content the stream stands for;
the system zlib decoding the stream to that content is what checks the writer (tests/test_deflate_writer_cpu.py).

Besides the bytes, the writer keeps a layout record for every block and token: where it starts (bit offset in the stream, wrapper
included), how many bits it takes, the output offset it writes at and its kind.  Feature predicates are computed from these
records, so that a case's tags are facts about the stream.

Malformed fields are written on request (keyword arguments named in each method), one keyword per verdict of the decoder."""
import heapq
import struct
import zlib
from collections import namedtuple

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# A layout record.  kind: block (a block's header; `sym` = BTYPE), lit, match, eob, sym (a bare lit/len code the test chose, such
# as 286 or 287), dsym (a bare distance code), stored (a stored block's payload).  `bit` / `nbits`: where it lies in the stream
# (wrapper included), `out` the output offset it writes at, `dsym` / `length` / `dist` / `extra` those of a match, `block` the
# index of the block it belongs to.
Rec = namedtuple("Rec", "kind bit nbits out sym dsym length dist extra block")


def len_sym(length):
    """the usual symbol of a match length (258 is 285)"""
    if length == 258:
        return 285
    return 257 + max(i for i in range(28) if LBASE[i] <= length)


def dist_sym(dist):
    return max(i for i in range(30) if DBASE[i] <= dist)


class BitWriter:
    """LSB-first bit packing (RFC 1951 3.1.1)"""

    def __init__(self):
        self.buf, self.acc, self.nacc = bytearray(), 0, 0

    @property
    def n(self):
        """bits written so far"""
        return 8 * len(self.buf) + self.nacc

    def put(self, v, n):
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.acc |= v << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.nacc -= 8

    def put_code(self, code, n):
        """a Huffman code: its most significant bit first (an over-subscribed set's codes are cut to their length)"""
        self.put(int(format(code & ((1 << n) - 1), f"0{n}b")[::-1], 2), n)

    def align(self):
        self.put(0, -self.nacc & 7)

    def bytes(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.nacc else b"")


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code of `lengths` (RFC 1951 3.2.2); incomplete sets get their codes as well"""
    bl = [0] * 16
    for l in lengths:
        if l:
            bl[l] += 1
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lengths):
    """sum of 2^(15 - l) over the used lengths: 32768 = complete, more = over-subscribed"""
    return sum(1 << (15 - l) for l in lengths if l)


def lengths_for(freq, maxbits, n):
    """complete code lengths (a list of `n`) of a length-limited code over the symbols of `freq` {symbol: count}; a lone symbol
    gets a twin of the same length so that the set is complete"""
    freq = {s: f for s, f in freq.items() if f}
    if len(freq) == 1:
        s = next(iter(freq))
        freq[(s + 1) % n] = 1
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freq.items()))]
    heapq.heapify(heap)
    depth = {s: 0 for s in freq}
    k = len(heap)
    while len(heap) > 1:
        f1, _, a = heapq.heappop(heap)
        f2, _, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (f1 + f2, k, a + b))
        k += 1
    depth = {s: min(d, maxbits) for s, d in depth.items()}
    while sum(2.0 ** -d for d in depth.values()) > 1:
        s = max((s for s in depth if depth[s] < maxbits), key=lambda s: (depth[s], s))
        depth[s] += 1
    while True:
        slack = 1 - sum(2.0 ** -d for d in depth.values())
        if slack == 0:
            break
        s = min((s for s in depth if 2.0 ** -depth[s] <= slack), key=lambda s: (depth[s], s))
        depth[s] -= 1
    out = [0] * n
    for s, d in depth.items():
        out[s] = d
    return out


def rle_lengths(lens):
    """the code-length symbol sequence of `lens` (the lit/len and distance lengths as one run, as RFC 1951 allows): 17 / 18 for
    runs of zeros, 16 for repeats of the length before.  -> [(symbol, extra value)]"""
    out, i = [], 0
    while i < len(lens):
        l, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == l:
            r += 1
        if l == 0 and r >= 3:
            r = min(r, 138)
            out.append((18, r - 11) if r >= 11 else (17, r - 3))
        elif l and r >= 4:
            out.append((l, 0))
            r = 1 + min(r - 1, 6)
            out.append((16, r - 4))
        else:
            out.append((l, 0))
            r = 1
        i += r
    return out


def expand_cl_seq(seq):
    """the code lengths a code-length symbol sequence stands for (None: a 16 with no length before it)"""
    out = []
    for s, x in seq:
        if s < 16:
            out.append(s)
        elif s == 16:
            if not out:
                return None
            out += [out[-1]] * (3 + x)
        else:
            out += [0] * ((3 if s == 17 else 11) + x)
    return out


class Deflate:
    """One raw DEFLATE stream, block by block (the wrappers are added by wrap())."""

    def __init__(self):
        self.w = BitWriter()
        self.content = bytearray()
        self.layout = []
        self.blocks = []  # (first bit, BTYPE, final[, the code lengths of a dynamic block])

    def _rec(self, kind, bit, sym=None, dsym=None, length=None, dist=None, extra=None, out=None):
        r = Rec(kind, bit, self.w.n - bit, len(self.content) if out is None else out, sym, dsym, length, dist, extra, len(self.blocks) - 1)
        self.layout.append(r)
        return r

    def _header(self, final, btype):
        self.blocks.append((self.w.n, btype, final))
        b = self.w.n
        self.w.put(int(final), 1)
        self.w.put(btype, 2)
        return b

    # ---- blocks
    def stored(self, data, final=False, len_field=None, nlen_field=None):
        """a stored block; `len_field` / `nlen_field` write other LEN / NLEN values (malformed on request: a mismatched pair)"""
        data = bytes(data)
        b = self._header(final, 0)
        self.w.align()
        n = len(data) if len_field is None else len_field
        self.w.put(n, 16)
        self.w.put((~n & 0xFFFF) if nlen_field is None else nlen_field, 16)
        self._rec("block", b, sym=0)
        p = self.w.n
        for x in data:
            self.w.put(x, 8)
        self._rec("stored", p, out=len(self.content))
        self.content += data
        return self

    def fixed(self, tokens, final=False, eob=True):
        b = self._header(final, 1)
        self._rec("block", b, sym=1)
        self._tokens(tokens, canonical(FIXED_LIT), canonical(FIXED_DIST), eob)
        return self

    def btype3(self, final=True):
        b = self._header(final, 3)
        self._rec("block", b, sym=3)
        return self

    def dynamic(self, tokens, lit_lens=None, dist_lens=None, final=False, cl_lens=None, cl_seq=None, hlit=None, hdist=None, hclen=None,
                eob=True, nlit=257, ndist=1):
        """a dynamic block.  `lit_lens` (257..288 entries) / `dist_lens` (1..32): the code lengths; by default a complete code over
        the symbols `tokens` use, at least `nlit` / `ndist` entries long.  `cl_seq`: the code-length symbols [(symbol, extra)], by default rle_lengths() over both sets
        as one run.  `cl_lens`: the 19 lengths of the code-length code (by default a complete code over the symbols of `cl_seq`).
        HCLEN is the shortest that holds `cl_lens`.  Malformed on request: `hlit` / `hdist` / `hclen` write other field values (as
        they stand in the stream: HLIT - 257, HDIST - 1, HCLEN - 4)."""
        if lit_lens is None or dist_lens is None:
            lf, df = {256: 1}, {}
            for t in tokens:
                if isinstance(t, int):
                    lf[t] = lf.get(t, 0) + 1
                elif t[0] == "m":
                    s = t[3] if len(t) > 3 and t[3] is not None else len_sym(t[1])
                    d = t[4] if len(t) > 4 and t[4] is not None else dist_sym(t[2])
                    lf[s] = lf.get(s, 0) + 1
                    df[d] = df.get(d, 0) + 1
            if lit_lens is None:
                lit_lens = lengths_for(lf, 15, max(nlit, max(lf) + 1))
            if dist_lens is None:
                dist_lens = lengths_for(df, 15, max(ndist, max(df) + 1)) if df else [0] * ndist
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if cl_seq is None:
            cl_seq = rle_lengths(lit_lens + dist_lens)
        if cl_lens is None:
            cf = {}
            for s, _ in cl_seq:
                cf[s] = cf.get(s, 0) + 1
            cl_lens = lengths_for(cf, 7, 19)
        ncl = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        b = self._header(final, 2)
        self.w.put(len(lit_lens) - 257 if hlit is None else hlit, 5)
        self.w.put(len(dist_lens) - 1 if hdist is None else hdist, 5)
        self.w.put(ncl - 4 if hclen is None else hclen, 4)
        for i in range(ncl):
            self.w.put(cl_lens[CL_ORDER[i]], 3)
        cc = canonical(cl_lens)
        for s, x in cl_seq:
            self.w.put_code(*cc[s])
            if s in CL_EXTRA:
                self.w.put(x, CL_EXTRA[s])
        self._rec("block", b, sym=2)
        self.blocks[-1] = self.blocks[-1] + (dict(lit=lit_lens, dist=dist_lens, cl=list(cl_lens), cl_seq=list(cl_seq), ncl=ncl),)
        if tokens is not None:
            self._tokens(tokens, canonical(lit_lens), canonical(dist_lens), eob)
        return self

    def _tokens(self, tokens, lc, dc, eob):
        """tokens: an int (a literal); ("m", length, dist[, length symbol[, distance symbol]]) with the extra bits the values
        imply; ("s", symbol[, extra]) a bare lit/len code; ("d", symbol[, extra]) a bare distance code"""
        for t in tokens:
            b = self.w.n
            if isinstance(t, int):
                self.w.put_code(*lc[t])
                self._rec("lit", b, sym=t)
                self.content.append(t)
            elif t[0] == "m":
                length, dist = t[1], t[2]
                s = t[3] if len(t) > 3 and t[3] is not None else len_sym(length)
                d = t[4] if len(t) > 4 and t[4] is not None else dist_sym(dist)
                le, de = length - LBASE[s - 257], dist - DBASE[d]
                assert 0 <= le < (1 << LEXT[s - 257]) or (le == 0 and LEXT[s - 257] == 0), (length, s)
                assert 0 <= de < (1 << DEXT[d]) or (de == 0 and DEXT[d] == 0), (dist, d)
                self.w.put_code(*lc[s])
                self.w.put(le, LEXT[s - 257])
                self.w.put_code(*dc[d])
                self.w.put(de, DEXT[d])
                self._rec("match", b, sym=s, dsym=d, length=length, dist=dist, extra=(le, de))
                for _ in range(length):
                    self.content.append(self.content[-dist] if dist <= len(self.content) else 0)
            elif t[0] == "s":
                self.w.put_code(*lc[t[1]])
                if 257 <= t[1] < 286:
                    self.w.put(t[2] if len(t) > 2 else 0, LEXT[t[1] - 257])
                self._rec("sym", b, sym=t[1])
            elif t[0] == "d":
                self.w.put_code(*dc[t[1]])
                if t[1] < 30:
                    self.w.put(t[2] if len(t) > 2 else 0, DEXT[t[1]])
                self._rec("dsym", b, dsym=t[1])
            else:
                raise ValueError(t)
        if eob:
            b = self.w.n
            self.w.put_code(*lc[256])
            self._rec("eob", b, sym=256)

    def raw_bits(self, v, n):
        """bits as they are (garbage, or what follows a block written without its end)"""
        self.w.put(v, n)
        return self

    def body(self):
        return self.w.bytes()


# ---- wrappers (RFC 1950, 1952)
def zlib_header(cm=8, cinfo=7, flevel=2, fdict=False, dictid=0, fcheck=None):
    """CMF, FLG (FCHECK made right unless given), then DICTID when FDICT is set"""
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (int(fdict) << 5)
    if fcheck is None:
        fcheck = (31 - ((cmf << 8) | flg) % 31) % 31
    return bytes([cmf, flg | fcheck]) + (struct.pack(">I", dictid) if fdict else b"")


def gzip_header(flg=0, mtime=0, xfl=0, os_=255, extra=None, name=None, comment=None, hcrc=None, cm=8):
    """`flg`: bits besides the ones the fields below imply (FTEXT, the reserved ones); `hcrc`: True writes the right header
    CRC-16, an int writes that value"""
    flg |= (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc is not None else 0)
    h = bytearray([0x1F, 0x8B, cm, flg]) + struct.pack("<I", mtime) + bytes([xfl, os_])
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc is not None:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xFFFF) if hcrc is True else hcrc)
    return bytes(h)


def zlib_trailer(content, value=None):
    return struct.pack(">I", zlib.adler32(content) if value is None else value)


def gzip_trailer(content, crc=None, isize=None):
    return struct.pack("<II", zlib.crc32(content) if crc is None else crc, (len(content) & 0xFFFFFFFF) if isize is None else isize)


Stream = namedtuple("Stream", "data content layout hdr_len cuts blocks")


def wrap(d, fmt="raw", header=None, trailer=None, tail=b""):
    """-> Stream: the header of format "raw" | "zlib" | "gzip" (by default the plain one), the body of `d`, the trailer (by default
    the right one), then `tail` (bytes behind the stream).  `cuts`: the byte offsets at which the blocks begin; layout bit offsets
    count from the header's first bit."""
    content = bytes(d.content)
    if fmt == "raw":
        header, trailer = header or b"", trailer if trailer is not None else b""
    elif fmt == "zlib":
        header = zlib_header() if header is None else header
        trailer = zlib_trailer(content) if trailer is None else trailer
    else:
        header = gzip_header() if header is None else header
        trailer = gzip_trailer(content) if trailer is None else trailer
    h8 = 8 * len(header)
    layout = [r._replace(bit=r.bit + h8) for r in d.layout]
    blocks = [(b + h8,) + tuple(rest) for b, *rest in d.blocks]
    return Stream(header + d.body() + trailer + tail, content, layout, len(header), [len(header) + b // 8 for b, *_ in d.blocks], blocks)
