"""A reader of the zstd encoder's own frames (RFC 8878): what each block contains -- block type and size, the literals section's
type, Size_Format, sizes, streams and Huffman tree, Number_of_Sequences and its byte form, the three table modes with their accuracy
logs, and every sequence as (literal length code, literal length, match length code, match length, Offset_Value).  A test uses these
facts to prove that an input reaches the threshold it was built for, on the host core's frame and on the kernel's alike.  The reader
also regenerates the content, so every frame it explains it has also decoded.

It reads the forms this encoder writes (one frame, no dictionary, no Repeat_Mode, no treeless literals) and asserts on any other."""
from zstd_writer import DEFAULTS, LL_BASE, LL_BITS, MAGIC, ML_BASE, ML_BITS, Fse

BLOCK_TYPES = ("raw", "rle", "compressed")
LIT_TYPES = ("raw", "rle", "huf")
MODES = ("predefined", "rle", "fse")


class _Fwd:
    """little-endian bit reader (FSE table descriptions)"""

    def __init__(self, data, pos=0):
        self.d, self.p = data, pos * 8

    def peek(self, n):
        lo = self.p >> 3
        return (int.from_bytes(self.d[lo:lo + 8], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.p += n
        return v

    def byte_pos(self):
        return (self.p + 7) >> 3


class _Back:
    """backward bit reader (RFC 8878 4.1): starts below the closing 1 bit of the last byte and reads towards the first; bits
    below the start read as 0 and leave `left` negative"""

    def __init__(self, data):
        assert data and data[-1], "a backward stream ends in a byte with the closing bit"
        self.d = bytes(data)
        self.left = 8 * (len(data) - 1) + data[-1].bit_length() - 1

    def get(self, n):
        self.left -= n
        lo = self.left
        if lo < 0:
            v = self.get_from(0, n + lo) << -lo if n + lo > 0 else 0
            return v
        return self.get_from(lo, n)

    def get_from(self, lo, n):
        b = lo >> 3
        return (int.from_bytes(self.d[b:b + 8], "little") >> (lo & 7)) & ((1 << n) - 1)

    def peek(self, n):
        left = self.left
        v = self.get(n)
        self.left = left
        return v


def read_ncount(data, pos, max_sym):
    """An FSE table description at data[pos:] -> (norm, accuracy log, position behind it)."""
    r = _Fwd(data, pos)
    al = r.get(4) + 5
    remaining, threshold, nbits, norm = (1 << al) + 1, 1 << al, al + 1, []
    while remaining > 1 and len(norm) <= max_sym:
        mx = (2 * threshold - 1) - remaining
        v = r.peek(nbits)
        if v & (threshold - 1) < mx:
            v &= threshold - 1
            r.get(nbits - 1)
        else:
            r.get(nbits)
            if v >= threshold:
                v -= mx
        c = v - 1
        norm.append(c)
        remaining -= abs(c)
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        if c == 0:
            while True:
                z = r.get(2)
                norm += [0] * z
                if z != 3:
                    break
    assert remaining == 1 and len(norm) <= max_sym + 1, "bad FSE table description"
    return norm, al, r.byte_pos()


def _read_tree(b, p):
    """The Huffman tree description at b[p:] -> (form, weights written, all weights, longest code, position behind it)."""
    hb = b[p]
    p += 1
    if hb >= 128:
        nw = hb - 127
        ws = []
        for i in range(nw):
            byte = b[p + i // 2]
            ws.append(byte >> 4 if i % 2 == 0 else byte & 15)
        form, p = "direct", p + (nw + 1) // 2
    else:
        norm, al, q = read_ncount(b, p, 12)
        assert al <= 6
        t = Fse(norm, al)
        r = _Back(b[q:p + hb])
        s1, s2 = r.get(al), r.get(al)
        ws = []
        while True:
            ws.append(t.sym[s1])
            s1 = t.base[s1] + r.get(t.nb[s1])
            if r.left < 0:
                ws.append(t.sym[s2])
                break
            ws.append(t.sym[s2])
            s2 = t.base[s2] + r.get(t.nb[s2])
            if r.left < 0:
                ws.append(t.sym[s1])
                break
        form, p = "fse", p + hb
    total = sum(1 << (w - 1) for w in ws if w)
    assert total, "no weights"
    max_bits = total.bit_length()
    left = (1 << max_bits) - total
    assert left & (left - 1) == 0 and left, "the weights leave no power of two for the last symbol"
    allw = ws + [left.bit_length()]
    assert max_bits <= 11, "code longer than 11 bits"
    longest = max_bits + 1 - min(w for w in allw if w)
    return form, len(ws), allw, longest, p


def _huf_table(weights):
    max_bits = sum(1 << (w - 1) for w in weights if w).bit_length() - 1
    table, pos = [None] * (1 << max_bits), 0
    for wt in range(1, max_bits + 1):
        for s, w in enumerate(weights):
            if w == wt:
                for i in range(pos, pos + (1 << (wt - 1))):
                    table[i] = (s, max_bits + 1 - wt)
                pos += 1 << (wt - 1)
    assert pos == 1 << max_bits
    return table, max_bits


def _huf_stream(data, table, max_bits, n):
    r = _Back(data)
    out = bytearray()
    for _ in range(n):
        s, nb = table[r.peek(max_bits)]
        out.append(s)
        r.left -= nb
    assert r.left == 0, "a Huffman stream must be used up exactly"
    return out


def _literals(b, blk):
    """parses the literals section at the start of the block content b into blk -> position behind it"""
    lt, sf = b[0] & 3, (b[0] >> 2) & 3
    assert lt != 3, "treeless literals are not written"
    blk["lit_type"], blk["size_format"] = LIT_TYPES[lt], sf
    if lt < 2:
        hs = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = b[0] >> 3 if hs == 1 else int.from_bytes(b[:hs], "little") >> 4
        blk.update(lit_header=hs, lit_regen=regen, lit_comp=None, streams=0)
        if lt == 0:
            blk["literals"] = bytes(b[hs:hs + regen])
            return hs + regen
        blk["literals"] = bytes(b[hs:hs + 1]) * regen
        return hs + 1
    hs, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
    v = int.from_bytes(b[:hs], "little") >> 4
    regen, comp = v & ((1 << bits) - 1), v >> bits
    streams = 1 if sf == 0 else 4
    form, nw, weights, longest, p = _read_tree(b, hs)
    blk.update(lit_header=hs, lit_regen=regen, lit_comp=comp, streams=streams, tree=form, n_weights=nw, weights=weights,
               longest_code=longest, tree_bytes=p - hs)
    table, max_bits = _huf_table(weights)
    end = hs + comp
    if streams == 1:
        lits = _huf_stream(b[p:end], table, max_bits, regen)
        blk["stream_sizes"] = [end - p]
    else:
        sz = [int.from_bytes(b[p + 2 * k:p + 2 * k + 2], "little") for k in range(3)]
        p += 6
        sz.append(end - p - sum(sz))
        assert sz[3] > 0
        seg = (regen + 3) // 4
        counts = [seg, seg, seg, regen - 3 * seg]
        lits = bytearray()
        for k in range(4):
            lits += _huf_stream(b[p:p + sz[k]], table, max_bits, counts[k])
            p += sz[k]
        blk["stream_sizes"], blk["stream_counts"] = sz, counts
    blk["literals"] = bytes(lits)
    return end


def _sequences(b, q, blk):
    """parses the sequences section b[q:] (to the end of the block) into blk"""
    n0 = b[q]
    if n0 < 128:
        nseq, nb = n0, 1
    elif n0 < 255:
        nseq, nb = ((n0 - 128) << 8) + b[q + 1], 2
    else:
        nseq, nb = b[q + 1] + (b[q + 2] << 8) + 0x7F00, 3
    q += nb
    blk.update(nseq=nseq, nseq_bytes=nb, seqs=[], modes=None, logs={})
    if nseq == 0:
        assert q == len(b), "bytes behind an empty sequences section"
        return
    mb = b[q]
    q += 1
    assert mb & 3 == 0
    modes, tabs = [], []
    for name, sh, max_sym in (("ll", 6, 35), ("of", 4, 31), ("ml", 2, 52)):
        m = (mb >> sh) & 3
        assert m != 3, "Repeat_Mode is not written"
        modes.append(MODES[m])
        if m == 0:
            tabs.append(Fse(*DEFAULTS[name]))
        elif m == 1:
            assert b[q] <= max_sym
            tabs.append(Fse.rle(b[q]))
            q += 1
        else:
            norm, al, q = read_ncount(b, q, max_sym)
            assert 5 <= al <= (8 if name == "of" else 9)
            tabs.append(Fse(norm, al))
            blk["logs"][name] = al
    blk["modes"] = tuple(modes)
    tl, to, tm = tabs
    r = _Back(b[q:])
    sl, so, sm = r.get(tl.al), r.get(to.al), r.get(tm.al)
    seqs = blk["seqs"]
    for i in range(nseq):
        ofc, mlc, llc = to.sym[so], tm.sym[sm], tl.sym[sl]
        ofv = (1 << ofc) + r.get(ofc)
        ml = ML_BASE[mlc] + r.get(ML_BITS[mlc])
        ll = LL_BASE[llc] + r.get(LL_BITS[llc])
        seqs.append((llc, ll, mlc, ml, ofv))
        if i + 1 < nseq:
            sl = tl.base[sl] + r.get(tl.nb[sl])
            sm = tm.base[sm] + r.get(tm.nb[sm])
            so = to.base[so] + r.get(to.nb[so])
    assert r.left == 0, "the sequence bitstream must be used up exactly"


def _execute(out, blk, rep):
    """appends what the block regenerates to `out`; records each sequence's resolved offset in blk['offsets']"""
    lits, lp, offs = blk["literals"], 0, []
    for _llc, ll, _mlc, ml, ofv in blk["seqs"]:
        out += lits[lp:lp + ll]
        lp += ll
        if ofv > 3:
            off = ofv - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = ofv - (1 if ll else 0)
            if idx == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if idx == 3 else rep[idx]
                assert off > 0
                rep[:] = [off, rep[0], rep[2]] if idx == 1 else [off, rep[0], rep[1]]
        assert 0 < off <= len(out), "offset reaches behind the frame's start"
        offs.append(off)
        if off >= ml:
            start = len(out) - off
            out += out[start:start + ml]
        else:
            pat = bytes(out[-off:])
            out += (pat * (ml // off + 1))[:ml]
    out += lits[lp:]
    assert lp <= len(lits)
    blk["offsets"] = offs


def read_frame(frame):
    """-> {'single', 'fcs', 'fcs_bytes', 'window_log', 'checksum', 'header_size', 'blocks': [...], 'content'}.  Every block is a
    dict: 'type', 'size' (Block_Size), 'last', 'at' (offset of its header in the frame), 'regen' (bytes it regenerates); a
    compressed block adds 'lit_type', 'size_format', 'lit_header', 'lit_regen', 'lit_comp', 'streams' and 'literals'; with
    Huffman literals 'tree' (direct | fse), 'n_weights', 'weights', 'longest_code', 'tree_bytes', 'stream_sizes'; then 'nseq',
    'nseq_bytes', 'modes' (LL, OF, ML), 'logs' (accuracy logs of the FSE-compressed tables), 'seqs' and 'offsets'."""
    frame = bytes(frame)
    assert frame[:4] == MAGIC
    fhd = frame[4]
    single, has_ck, fcs_flag = (fhd >> 5) & 1, (fhd >> 2) & 1, fhd >> 6
    assert fhd & 3 == 0 and (fhd >> 3) & 1 == 0 and (fhd >> 4) & 1 == 0
    p = 5
    info = {"single": bool(single), "checksum": bool(has_ck), "window_log": None, "fcs": None}
    if not single:
        assert frame[p] & 7 == 0, "the window has no mantissa"
        info["window_log"] = 10 + (frame[p] >> 3)
        p += 1
    fb = [1 if single else 0, 2, 4, 8][fcs_flag]
    info["fcs_bytes"] = fb
    if fb:
        info["fcs"] = int.from_bytes(frame[p:p + fb], "little") + (256 if fb == 2 else 0)
        p += fb
    info["header_size"] = p
    out, rep, blocks = bytearray(), [1, 4, 8], []
    while True:
        h = int.from_bytes(frame[p:p + 3], "little")
        last, btype, bsize = h & 1, (h >> 1) & 3, h >> 3
        assert btype != 3, "reserved block type"
        blk = {"type": BLOCK_TYPES[btype], "size": bsize, "last": bool(last), "at": p}
        p += 3
        before = len(out)
        if btype == 0:
            out += frame[p:p + bsize]
            p += bsize
        elif btype == 1:
            out += frame[p:p + 1] * bsize
            p += 1
        else:
            b = frame[p:p + bsize]
            assert len(b) == bsize
            p += bsize
            q = _literals(b, blk)
            _sequences(b, q, blk)
            _execute(out, blk, rep)
        blk["regen"] = len(out) - before
        assert blk["regen"] <= 128 << 10
        blocks.append(blk)
        if last:
            break
    assert len(frame) == p + 4 * has_ck, "bytes behind the frame"
    if info["fcs"] is not None:
        assert info["fcs"] == len(out)
    info["blocks"], info["content"] = blocks, bytes(out)
    return info


def first_difference(a, b):
    """Where two frames of the same input part: a sentence naming the first block that differs."""
    if a is None or b is None:
        return "one of the frames is missing"
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    msg = f"lengths {len(a)} / {len(b)}, first differing byte {n}"
    try:
        ia, ib = read_frame(a), read_frame(b)
    except Exception as e:  # a frame the reader cannot explain: the offsets are all there is
        return f"{msg} (unreadable: {e})"
    if n < ia["header_size"]:
        return msg + ": in the frame header"
    for k, (x, y) in enumerate(zip(ia["blocks"], ib["blocks"])):
        keys = [key for key in ("type", "size", "lit_type", "size_format", "lit_regen", "lit_comp", "streams", "tree", "n_weights",
                                "weights", "nseq", "modes", "logs") if x.get(key) != y.get(key)]
        if keys or x.get("literals") != y.get("literals") or x.get("seqs") != y.get("seqs"):
            detail = ", ".join(f"{key} {x.get(key)!r} / {y.get(key)!r}" for key in keys if key != "weights") or "same header facts"
            if x.get("seqs") != y.get("seqs") and x.get("seqs") is not None and y.get("seqs") is not None:
                j = next((j for j, (s, t) in enumerate(zip(x["seqs"], y["seqs"])) if s != t), min(len(x["seqs"]), len(y["seqs"])))
                sa = x["seqs"][j] if j < len(x["seqs"]) else None
                sb = y["seqs"][j] if j < len(y["seqs"]) else None
                detail += f"; first differing sequence {j}: {sa} / {sb}"
            return f"{msg}: block {k} at {x['at']} ({x['type']} / {y['type']}): {detail}"
    return msg + ": behind the last block both explain alike (checksum or block count)"
