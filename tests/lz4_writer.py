"""Builds LZ4 blocks from sequence lists and LZ4 frames from blocks and flags, bad ones included (tests only).  Nothing here is
the library's code; lz4_ref.py reads what this writes."""
import struct

import lz4_ref as R


def _length(base, extra_bytes=None):
    """nibble and extension bytes of a length field whose value (without the match's +4) is `base`; extra_bytes overrides the
    extension (any bytes, for non-canonical and damaged forms)"""
    if extra_bytes is not None:
        return 15, bytes(extra_bytes)
    if base < 15:
        return base, b""
    rest = base - 15
    return 15, b"\xff" * (rest // 255) + bytes([rest % 255])


def sequence(lits=b"", offset=None, mlen=None, low_nibble=0, ll_ext=None, ml_ext=None):
    """One sequence: literals, then (offset, mlen) unless offset is None -- a last sequence, whose low nibble is `low_nibble`."""
    ln, le = _length(len(lits), ll_ext)
    if offset is None:
        return bytes([(ln << 4) | (low_nibble & 15)]) + le + bytes(lits)
    assert mlen >= 4
    mn, me = _length(mlen - 4, ml_ext)
    return bytes([(ln << 4) | mn]) + le + bytes(lits) + struct.pack("<H", offset) + me


def block(seqs, last=b"", low_nibble=0, end=True):
    """A block of (lits, offset, mlen) sequences closed by a last sequence of `last` literals (end=False: no last sequence)"""
    out = b"".join(sequence(l, o, m) for l, o, m in seqs)
    return out + (sequence(last, low_nibble=low_nibble) if end else b"")


def expand(seqs, last=b"", history=b""):
    """the content a block of these sequences stands for"""
    out = bytearray(history)
    for l, o, m in seqs:
        out += l
        for _ in range(m):
            out.append(out[-o])
    out += last
    return bytes(out[len(history):])


def compress(data, history=b"", min_match=4, max_dist=65535):
    """A greedy hash-chain-free compressor: (seqs, last) for block(); matches may reach into `history` (linked blocks).  Keeps the
    format's end-of-block restrictions (the last 5 bytes are literals, no match starts in the last 12), like a real encoder."""
    buf = bytes(history) + bytes(data)
    base, n = len(history), len(buf)
    table, seqs, anchor, i = {}, [], base, base
    for j in range(max(0, base - max_dist), base - 3):
        table[buf[j:j + 4]] = j
    limit = n - 12
    while i < limit:
        key = buf[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is not None and i - cand <= max_dist:
            m = 4
            while i + m < n - 5 and buf[cand + m] == buf[i + m]:
                m += 1
            if m >= min_match:
                seqs.append((buf[anchor:i], i - cand, m))
                i += m
                anchor = i
                continue
        i += 1
    return seqs, buf[anchor:]


def compress_block(data, history=b""):
    seqs, last = compress(data, history)
    return block(seqs, last)


def header(indep=True, bchk=False, csize=None, cchk=False, bd=4, version=1, flg_reserved=0, bd_extra=0, dict_id=None, hc=None, magic=R.MAGIC):
    flg = (version << 6) | (0x20 if indep else 0) | (0x10 if bchk else 0) | (8 if csize is not None else 0) | (4 if cchk else 0) | (
        2 if flg_reserved else 0) | (1 if dict_id is not None else 0)
    desc = bytes([flg, ((bd & 7) << 4) | bd_extra])
    if csize is not None:
        desc += struct.pack("<Q", csize)
    if dict_id is not None:
        desc += struct.pack("<I", dict_id)
    return struct.pack("<I", magic) + desc + bytes([(R.xxh32(desc) >> 8) & 0xFF if hc is None else hc])


def frame(blocks, content=None, indep=True, bchk=False, csize=False, cchk=False, bd=4, end_mark=True, csize_value=None, cchk_value=None,
          bchk_values=None, **hdr):
    """A frame of `blocks`, each (stored: bool, payload bytes).  content: what the frame decodes to (for C.Size and C.Checksum);
    None: found with lz4_ref.  csize / cchk / bchk: the flags; *_value(s) override what is stored ({index: value} for blocks)."""
    if content is None:
        out = bytearray()
        for stored, pay in blocks:
            out += pay if stored else R.block_decode(pay, history=b"" if indep else bytes(out[-65535:]))[0]
        content = bytes(out)
    size = None
    if csize:
        size = len(content) if csize_value is None else csize_value
    f = bytearray(header(indep, bchk, size, cchk, bd, **hdr))
    for i, (stored, pay) in enumerate(blocks):
        f += struct.pack("<I", len(pay) | (0x80000000 if stored else 0)) + pay
        if bchk:
            f += struct.pack("<I", (bchk_values or {}).get(i, R.xxh32(pay)))
    if end_mark:
        f += struct.pack("<I", 0)
        if cchk:
            f += struct.pack("<I", R.xxh32(content) if cchk_value is None else cchk_value)
    return bytes(f)


def frame_of(data, block_size, linked=False, stored_every=0, **kw):
    """`data` cut into blocks of block_size bytes (a list gives the cut lengths), each compressed by compress() -- every
    stored_every-th one stored instead -- and framed"""
    sizes = block_size if isinstance(block_size, (list, tuple)) else [block_size] * ((len(data) + block_size - 1) // block_size)
    blocks, at = [], 0
    for i, sz in enumerate(sizes):
        chunk = data[at:at + sz]
        if stored_every and i % stored_every == stored_every - 1:
            blocks.append((True, chunk))
        else:
            blocks.append((False, compress_block(chunk, data[max(0, at - 65535):at] if linked else b"")))
        at += sz
    assert at >= len(data)
    return frame(blocks, content=data[:at], indep=not linked, **kw)
