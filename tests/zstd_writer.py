"""A small zstd frame writer for hand-built test frames (RFC 8878): every header field, block type, literals section, Huffman tree,
table mode and sequence -- down to the exact Offset_Value of each -- is chosen by the test, so that the forms an encoder rarely emits
can be pinned.  The writer also computes the content the frame stands for; the system libzstd decoding the frame to that content is
what checks the writer (tests/test_zstd_writer_cpu.py).

Deliberately malformed fields are written on request (keyword arguments named in each method), so that a case can aim at one
verdict of the decoder.  FSE-compressed Huffman weights are not written: every Huffman block libzstd emits has them, and the direct
4-bit form is the one it never reaches."""
MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 128 * 1024

LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048,
           4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
          1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1]
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
MAX_AL = {"ll": 9, "of": 8, "ml": 9}
DEFAULTS = {"ll": (LL_DEF, 6), "of": (OF_DEF, 5), "ml": (ML_DEF, 6)}


def ll_code(v):
    return max(c for c in range(36) if LL_BASE[c] <= v)


def ml_code(v):
    return max(c for c in range(53) if ML_BASE[c] <= v)


def new_offset(off):
    """the Offset_Value of a new offset (RFC 8878 3.1.1.5): values 1 to 3 are repeat codes"""
    return off + 3


class FwdBits:
    """little-endian bit writer (FSE table descriptions)"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.v |= v << self.n
        self.n += n

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def back_stream(fields, extra_low=0, drop_low=0, zero_tail=False):
    """A backward bitstream (RFC 8878 4.1) whose reader takes `fields` ((value, nbits) pairs) in the order given: the fields are
    written in reverse, low bits first, then the closing 1 bit.  Malformed on request: `extra_low` zero bits below the first field
    written (bits the reader leaves over), `drop_low` bits cut from the bottom (the reader runs past the start), `zero_tail` a zero
    byte after the closing bit."""
    v, n = 0, extra_low
    for val, nb in reversed(fields):
        assert 0 <= val < (1 << nb) or (nb == 0 and val == 0), (val, nb)
        v |= val << n
        n += nb
    v >>= drop_low
    n -= drop_low
    v |= 1 << n
    out = v.to_bytes(n // 8 + 1, "little")
    return out + (b"\0" if zero_tail else b"")


# ---- FSE (RFC 8878 4.1.1) ----
class Fse:
    """the decoding table of a normalized distribution, built as the RFC (and every decoder) builds it"""

    def __init__(self, norm, al):
        size = 1 << al
        self.al = al
        sym = [0] * size
        high = size - 1
        nxt = []
        for s, c in enumerate(norm):
            if c == -1:
                sym[high] = s
                high -= 1
                nxt.append(1)
            else:
                nxt.append(c)
        step, pos = (size >> 1) + (size >> 3) + 3, 0
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0, "not a valid distribution"
        self.sym, self.nb, self.base = sym, [0] * size, [0] * size
        for u in range(size):
            ns = nxt[sym[u]]
            nxt[sym[u]] += 1
            nb = al - (ns.bit_length() - 1)
            self.nb[u], self.base[u] = nb, (ns << nb) - size

    @classmethod
    def rle(cls, s):
        t = cls.__new__(cls)
        t.al, t.sym, t.nb, t.base = 0, [s], [0], [0]
        return t

    def state_for(self, s, nxt=None):
        """a state that decodes `s` and (if `nxt` is given) moves on to state `nxt`: the one whose [base, base + 2^nb) covers it"""
        for u in range(len(self.sym)):
            if self.sym[u] == s and (nxt is None or self.base[u] <= nxt < self.base[u] + (1 << self.nb[u])):
                return u
        raise ValueError(f"symbol {s} is not in the table")


def ncount(norm, al, al_field=None):
    """the table description of a normalized distribution (RFC 8878 4.1.1): accuracy, then each count with the variable-width
    code the decoder's `threshold` / `max` arithmetic implies, zero runs after a 0 through 2-bit repeat flags (3 = three more
    and another flag).  `al_field` writes another accuracy than the table's (malformed on request)."""
    w = FwdBits()
    w.put((al if al_field is None else al_field) - 5, 4)
    remaining, threshold, nbits = (1 << al) + 1, 1 << al, al + 1
    s, last = 0, max(i for i, c in enumerate(norm) if c)
    while s <= last:
        c = norm[s]
        v = c + 1
        mx = (2 * threshold - 1) - remaining
        if v < mx:
            w.put(v, nbits - 1)
        elif v < threshold:
            w.put(v, nbits)
        else:
            w.put(v + mx, nbits)
        remaining -= abs(c)
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        s += 1
        if c == 0:
            z = 0
            while s + z <= last and norm[s + z] == 0:
                z += 1
            for _ in range(z // 3):
                w.put(3, 2)
            w.put(z % 3, 2)
            s += z
    assert remaining == 1, "counts do not add up to 1 << al"
    return w.bytes()


def normalize(counts, al):
    """a valid normalized distribution of accuracy `al` over the symbols with nonzero `counts` (any positive weights): -1 for
    symbols of weight < 0 (the "less than one" probability), the rest shared out in proportion"""
    size = 1 << al
    norm = [0] * len(counts)
    small = [s for s, c in enumerate(counts) if c < 0]
    for s in small:
        norm[s] = -1
    big = [s for s, c in enumerate(counts) if c > 0]
    left = size - len(small)
    assert left >= len(big)
    tot = sum(counts[s] for s in big)
    for s in big:
        norm[s] = max(1, counts[s] * left // tot)
    d = left - sum(norm[s] for s in big)
    order = sorted(big, key=lambda s: -norm[s])
    i = 0
    while d:
        s = order[i % len(order)]
        if d > 0:
            norm[s] += 1
            d -= 1
        elif norm[s] > 1:
            norm[s] -= 1
            d += 1
        i += 1
    return norm


# ---- Huffman literals (RFC 8878 4.2) ----
class Huf:
    """canonical codes from weights (the last symbol's weight is implied by the others in the tree description): the decoding
    table fills 2^max_bits entries in order of weight, then symbol, and a symbol's code is its first entry >> (weight - 1)"""

    def __init__(self, weights):
        total = sum(1 << (w - 1) for w in weights if w)
        self.max_bits = total.bit_length() - 1
        assert total == 1 << self.max_bits and self.max_bits <= 11, "weights do not make a complete code"
        self.codes, pos = {}, 0
        for wt in range(1, self.max_bits + 1):
            for s, w in enumerate(weights):
                if w == wt:
                    self.codes[s] = (pos >> (wt - 1), self.max_bits + 1 - wt)
                    pos += 1 << (wt - 1)
        self.weights = list(weights)

    def stream(self, data, extra_low=0, drop_low=0):
        return back_stream([self.codes[b] for b in data], extra_low, drop_low)


def seq_codes(seqs):
    """the LL, OF and ML codes of (literal length, match length, Offset_Value) triples"""
    return [ll_code(s[0]) for s in seqs], [s[2].bit_length() - 1 for s in seqs], [ml_code(s[1]) for s in seqs]


def fit(codes, al, less_than_one=()):
    """a normalized distribution of accuracy `al` in which every code of `codes` occurs (those in `less_than_one` with the
    "less than one" probability -1)"""
    counts = [0] * (max(codes) + 1)
    for c in codes:
        counts[c] += 1
    for c in less_than_one:
        counts[c] = -1
    return normalize(counts, al)


def direct_tree(weights):
    """tree description in the direct form: 127 + number of weights, then 4-bit weights, high nibble first; the last symbol's
    weight is left out"""
    ws = list(weights[:-1])
    assert len(ws) <= 128
    body = bytes(((ws[i] << 4) | (ws[i + 1] if i + 1 < len(ws) else 0)) for i in range(0, len(ws), 2))
    return bytes([127 + len(ws)]) + body


def huf_weights(data, max_bits=11):
    """weights of a length-limited code for the bytes of `data` (any valid code serves; nothing needs it to be optimal)"""
    import heapq

    freq = {}
    for b in data:
        freq[b] = freq.get(b, 0) + 1
    if len(freq) == 1:
        freq[(next(iter(freq)) + 1) & 255] = 1
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
    # limit the lengths: clamp, then lengthen the shortest codes until the Kraft sum is exact again
    depth = {s: min(d, max_bits) for s, d in depth.items()}
    while sum(2.0 ** -d for d in depth.values()) > 1:
        s = max((s for s in depth if depth[s] < max_bits), key=lambda s: (depth[s], s))
        depth[s] += 1
    while True:
        slack = 1 - sum(2.0 ** -d for d in depth.values())
        if slack == 0:
            break
        s = min((s for s in depth if 2.0 ** -depth[s] <= slack), key=lambda s: (depth[s], s), default=None)
        assert s is not None
        depth[s] -= 1
    mb = max(depth.values())
    w = [0] * (max(depth) + 1)
    for s, d in depth.items():
        w[s] = mb + 1 - d
    return w


def weights_of_lengths(lengths):
    """weights from code lengths {symbol: length}"""
    mb = max(lengths.values())
    w = [0] * (max(lengths) + 1)
    for s, d in lengths.items():
        w[s] = mb + 1 - d
    return w


def _lit_header(kind, sf, regen, comp=0):
    t = {"raw": 0, "rle": 1, "huf": 2, "treeless": 3}[kind]
    if t < 2:
        if sf in (0, 2):  # one bit of Size_Format: bit 3 is the low bit of the 5-bit size
            assert regen < 32
            return bytes([t | (regen << 3)])
        if sf == 1:
            assert regen < 4096
            return (t | (sf << 2) | (regen << 4)).to_bytes(2, "little")
        assert regen < 1 << 20
        return (t | (sf << 2) | (regen << 4)).to_bytes(3, "little")
    nb, hl = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[sf]
    assert regen < 1 << nb and comp < 1 << nb, (regen, comp, sf)
    return (t | (sf << 2) | (regen << 4) | (comp << (4 + nb))).to_bytes(hl, "little")


class Frame:
    """One zstd frame.  `fcs`: True writes the content size in the smallest form (1 byte only with Single_Segment), an int forces
    the field's byte count (1, 2, 4, 8), None leaves it out; `fcs_value` overrides the value written.  `window`: (exponent,
    mantissa) of the window descriptor, or None for Single_Segment.  `dict_id`: (value, bytes) of a Dictionary_ID field.
    `unused_bit` and `reserved_bit` set bits 4 and 3 of the frame header descriptor."""

    def __init__(self, fcs=True, window=None, checksum=False, dict_id=None, unused_bit=False, reserved_bit=False, fcs_value=None):
        self.fcs, self.window, self.checksum, self.dict_id = fcs, window, checksum, dict_id
        self.unused_bit, self.reserved_bit, self.fcs_value = unused_bit, reserved_bit, fcs_value
        self.blocks = bytearray()
        self.content = bytearray()
        self.rep = [1, 4, 8]
        self.huf = None
        self.tabs = {"ll": None, "of": None, "ml": None}
        self.nblocks = 0
        self.block_ends = []  # byte offset (in the frame body) just behind each block

    # -- blocks --
    def _block(self, btype, size_field, body, last):
        self.blocks += ((size_field << 3) | (btype << 1) | int(last)).to_bytes(3, "little") + body
        self.nblocks += 1
        self.block_ends.append(len(self.blocks))
        return self

    def raw(self, data, last=False):
        self.content += data
        return self._block(0, len(data), bytes(data), last)

    def rle(self, byte, n, last=False):
        self.content += bytes([byte]) * n
        return self._block(1, n, bytes([byte]), last)

    def reserved(self, body=b"\0", last=True):
        return self._block(3, len(body), body, last)

    def compressed(self, lits=b"", seqs=(), lit="raw", sf=None, streams=1, weights=None, tree="direct", modes=("pre", "pre", "pre"),
                   nseq_form=None, last=False, **bad):
        """A Compressed_Block.  `lits`: the literals; `seqs`: (literal length, match length, Offset_Value) triples, executed in
        order (the literals left over follow the last one).  `lit` is raw, rle, huf or treeless; `sf` the Size_Format (default:
        the smallest that holds the sizes); `weights` the Huffman weights of a huf section (default: computed from `lits`).
        `modes`: the table modes of LL, OF, ML -- "pre", ("rle", code), ("fse", norm, accuracy) or "rep".  `nseq_form`: bytes of
        the Number_of_Sequences field (1, 2, 3).
        Malformed on request (`bad`): lit_regen (regenerated size written), lit_extra/lit_drop (bits left over / missing in the
        first Huffman stream), tree_bytes (the tree description written), seq_extra/seq_drop/seq_zero_tail (the same for the sequence bitstream), modes_low (the reserved
        bits of the modes byte), al_field ({table: accuracy written}), rle_code ({table: code written}), nseq (count written),
        block_size (Block_Size written), body_tail (bytes appended to the block)."""
        lits = bytes(lits)
        body = self._literals(lits, lit, sf, streams, weights, tree, bad)
        body += self._sequences(lits, list(seqs), modes, nseq_form, bad)
        body += bad.get("body_tail", b"")
        return self._block(2, bad.get("block_size", len(body)), body, last)

    def _literals(self, lits, lit, sf, streams, weights, tree, bad):
        regen = bad.get("lit_regen", len(lits))
        if lit == "raw" or lit == "rle":
            if sf is None:
                sf = 0 if regen < 32 else 1 if regen < 4096 else 3
            if lit == "rle":
                assert len(set(lits)) <= 1
                return _lit_header("rle", sf, regen) + (lits[:1] or b"\0")
            return _lit_header("raw", sf, regen) + lits
        if lit == "huf":
            weights = weights or huf_weights(lits)
            self.huf = Huf(weights)
            desc = bad.get("tree_bytes") or direct_tree(weights)
        else:
            desc = b""  # treeless: the last block's table (`weights` only encodes the stream of a block that has none)
        h = self.huf if lit == "huf" or weights is None else Huf(weights)
        if streams == 1:
            payload = h.stream(lits, bad.get("lit_extra", 0), bad.get("lit_drop", 0))
        else:
            seg = (len(lits) + 3) // 4
            parts = [lits[k * seg:(k + 1) * seg] for k in range(3)] + [lits[3 * seg:]]
            ss = [h.stream(p, bad.get("lit_extra", 0) if k == 0 else 0, bad.get("lit_drop", 0) if k == 0 else 0) for k, p in enumerate(parts)]
            payload = b"".join(len(s).to_bytes(2, "little") for s in ss[:3]) + b"".join(ss)
        comp = len(desc) + len(payload)
        if sf is None:
            sf = (0 if streams == 1 else 1) if max(regen, comp) < 1024 else 2 if max(regen, comp) < 16384 else 3
        assert (sf == 0) == (streams == 1)
        return _lit_header(lit, sf, regen, comp) + desc + payload

    def _sequences(self, lits, seqs, modes, nseq_form, bad):
        n = bad.get("nseq", len(seqs))
        form = nseq_form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
        if form == 1:
            assert n < 128
            out = bytearray([n])
        elif form == 2:
            assert n < 0x7F00
            out = bytearray([128 + (n >> 8), n & 255])
        else:
            assert n >= 0x7F00
            out = bytearray([255]) + (n - 0x7F00).to_bytes(2, "little")
        # the content, the codes and the extra bits of each sequence
        codes, start = [], len(self.content)
        lp = 0
        for ll, ml, ov in seqs:
            self.content += lits[lp:lp + ll]
            lp += ll
            off = self._resolve(ll, ov)
            assert 0 < off <= len(self.content) or bad, f"offset {off} reaches behind the frame start"
            for k in range(ml):
                self.content.append(self.content[-off] if off <= len(self.content) else 0)
            oc = ov.bit_length() - 1
            lc, mc = ll_code(ll), ml_code(ml)
            codes.append((lc, oc, mc, (ov - (1 << oc), oc), (ml - ML_BASE[mc], ML_BITS[mc]), (ll - LL_BASE[lc], LL_BITS[lc])))
        assert lp <= len(lits)
        self.content += lits[lp:]
        assert len(self.content) - start <= BLOCK_MAX or bad, "the block regenerates more than Block_Maximum_Size"
        if n == 0 and not seqs:
            return bytes(out)
        # table modes
        mb, descs, tabs = 0, b"", {}
        for k, (name, mode) in enumerate(zip(("ll", "of", "ml"), modes)):
            if mode == "pre":
                m, t = 0, Fse(*DEFAULTS[name])
            elif mode == "rep":
                m, t = 3, self.tabs[name] or Fse(*DEFAULTS[name])
            elif mode[0] == "rle":
                m, t = 1, Fse.rle(mode[1])
                descs += bytes([bad.get("rle_code", {}).get(name, mode[1])])
            else:
                m, t = 2, Fse(mode[1], mode[2])
                descs += ncount(mode[1], mode[2], bad.get("al_field", {}).get(name))
            mb |= m << (6 - 2 * k)
            tabs[name] = t
        self.tabs.update(tabs)
        out.append(mb | bad.get("modes_low", 0))
        out += descs
        # states, from the last sequence back to the first: each state is the one of its symbol that leads to the next state
        st = {"ll": [], "of": [], "ml": []}
        for name, ci in (("ll", 0), ("of", 1), ("ml", 2)):
            t, nxt = tabs[name], None
            for c in reversed(codes):
                nxt = t.state_for(c[ci], nxt)
                st[name].append(nxt)
            st[name].reverse()
        fields = [(st["ll"][0], tabs["ll"].al), (st["of"][0], tabs["of"].al), (st["ml"][0], tabs["ml"].al)]
        for i, c in enumerate(codes):
            fields += [c[3], c[4], c[5]]
            if i + 1 < len(codes):
                for name in ("ll", "ml", "of"):
                    t, u = tabs[name], st[name][i]
                    fields.append((st[name][i + 1] - t.base[u], t.nb[u]))
        out += back_stream(fields, bad.get("seq_extra", 0), bad.get("seq_drop", 0), bad.get("seq_zero_tail", False))
        return bytes(out)

    def _resolve(self, ll, ov):
        """the offset an Offset_Value stands for, and the repeat-offset history after it (RFC 8878 3.1.2.5)"""
        r = self.rep
        if ov > 3:
            off = ov - 3
            self.rep = [off, r[0], r[1]]
            return off
        idx = ov - (ll != 0)  # 0: rep0 unchanged; 1, 2: rep1, rep2; 3: rep0 - 1
        if idx == 0:
            return r[0]
        off = r[0] - 1 if idx == 3 else r[idx]
        off = off or 1  # RFC 8878: an offset of 0 is read as 1 (rep0 - 1 == 0)
        self.rep = [off, r[0], r[1]] if idx != 1 else [off, r[0], r[2]]
        return off

    # -- the whole frame --
    def header(self):
        n = len(self.content)
        single = self.window is None
        fcs_bytes = 0
        if self.fcs is True:
            fcs_bytes = 1 if single and n < 256 else 2 if 256 <= n < 65536 + 256 else 4 if n < 1 << 32 else 8
        elif self.fcs:
            fcs_bytes = self.fcs
        assert single <= bool(fcs_bytes) and (single or fcs_bytes != 1), "Single_Segment needs a content size, and only it has a 1-byte one"
        flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
        did_v, did_b = self.dict_id or (0, 0)
        fhd = (flag << 6) | (int(single) << 5) | (int(self.unused_bit) << 4) | (int(self.reserved_bit) << 3) | (int(self.checksum) << 2)
        fhd |= {0: 0, 1: 1, 2: 2, 4: 3}[did_b]
        h = bytearray(MAGIC) + bytes([fhd])
        if not single:
            e, m = self.window
            h.append((e << 3) | m)
        h += did_v.to_bytes(did_b, "little")
        if fcs_bytes:
            v = n if self.fcs_value is None else self.fcs_value
            h += (v - 256 if fcs_bytes == 2 else v).to_bytes(fcs_bytes, "little")
        return bytes(h)

    def finish(self, checksum_value=None):
        """-> (frame, content)"""
        from oracle import oracle as O

        tail = b""
        if self.checksum:
            ck = O.xxh64(bytes(self.content)) & 0xFFFFFFFF if checksum_value is None else checksum_value
            tail = ck.to_bytes(4, "little")
        return self.header() + bytes(self.blocks) + tail, bytes(self.content)

    def block_cuts(self):
        """byte offsets of the frame at which each block begins and the checksum (or the frame's end) lies"""
        h = len(self.header())
        return [h] + [h + e for e in self.block_ends]


def window_size(e, m):
    w = 1 << (10 + e)
    return w + (w >> 3) * m


def skippable(payload, nibble=0):
    return (0x184D2A50 | nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + payload
