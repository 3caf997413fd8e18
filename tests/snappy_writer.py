"""Writes Snappy for the tests: raw blocks from element lists in any chosen tag form, framed streams from chunk lists, bad ones
included, and a small greedy compressor so that no test needs libsnappy.  An element is ("lit", bytes[, form]) -- form 0 the
inline length, 1..4 that many length bytes, None the shortest -- or ("copy", offset, length[, form]) -- form 1, 2 or 4 offset
bytes, None the shortest that holds it."""
import snappy_ref as R


def varint(n, nbytes=None):
    """n as a little-endian varint; nbytes: padded with continuation bits to that length (80 00 is 0 in two bytes)"""
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        more = n != 0 or (nbytes is not None and len(out) + 1 < nbytes)
        out.append(b | (0x80 if more else 0))
        if not more:
            return bytes(out)


def literal(data, form=None, stated=None):
    """`stated`: the length the header states (the bytes behind it are `data` whatever it says)"""
    n = len(data) if stated is None else stated
    if form is None:
        form = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
    if form == 0:
        assert 1 <= n <= 60
        return bytes([(n - 1) << 2]) + data
    assert 1 <= n <= 1 << (8 * form)
    return bytes([(59 + form) << 2]) + (n - 1).to_bytes(form, "little") + data


def copy(off, m, form=None):
    if form is None:
        form = 1 if 4 <= m <= 11 and off < 2048 else 2 if off < 65536 else 4
    if form == 1:
        assert 4 <= m <= 11 and off < 2048
        return bytes([1 | (m - 4) << 2 | (off >> 8) << 5, off & 0xFF])
    assert 1 <= m <= 64
    return bytes([(2 if form == 2 else 3) | (m - 1) << 2]) + off.to_bytes(form, "little")


def element(e):
    if isinstance(e, (bytes, bytearray)):
        return bytes(e)  # raw bytes, as they are
    if e[0] == "lit":
        return literal(e[1], *e[2:])
    return copy(*e[1:])


def expand(elems):
    out = bytearray()
    for e in elems:
        if e[0] == "lit":
            out += e[1]
        else:
            for _ in range(e[2]):
                out.append(out[-e[1]])
    return bytes(out)


def block(elems, n=None, preamble=None):
    """a raw block; n: the stated length (default: what the elements produce); preamble: its bytes as they are"""
    body = b"".join(element(e) for e in elems)
    if preamble is None:
        preamble = varint(len(expand([e for e in elems if not isinstance(e, (bytes, bytearray))])) if n is None else n)
    return preamble + body


def compress(data):
    """greedy, one hash probe per position: the element list of `data`"""
    elems, table, i, lit, n = [], {}, 0, 0, len(data)
    while i + 4 <= n:
        key = data[i:i + 4]
        j = table.get(key)
        table[key] = i
        if j is None or i - j > 65535:
            i += 1
            continue
        m = 4
        while i + m < n and m < 64 and data[j + m] == data[i + m]:
            m += 1
        if lit < i:
            elems.append(("lit", data[lit:i]))
        elems.append(("copy", i - j, m))
        i += m
        lit = i
    if lit < n:
        elems.append(("lit", data[lit:]))
    return elems


def compress_block(data):
    return block(compress(data), n=len(data))


# ---- the framing format ------------------------------------------------------------------------------------------------------------


def chunk(kind, payload, s=None):
    """a chunk header and its bytes; s: the length the header states"""
    return bytes([kind]) + (len(payload) if s is None else s).to_bytes(3, "little") + payload


def data_chunk(content, compressed=True, crc=None, body=None):
    """a data chunk of `content`; crc: the stored value instead of the right one; body: the bytes behind the CRC as they are"""
    if body is None:
        body = compress_block(content) if compressed else content
    c = R.mask(R.crc32c(content)) if crc is None else crc
    return chunk(0 if compressed else 1, c.to_bytes(4, "little") + body)


def padding(n):
    return chunk(0xFE, b"\0" * n)


def stream(chunks, ident=True):
    return (R.IDENT if ident else b"") + b"".join(chunks)


def stream_of(data, sizes, stored_every=0, between=()):
    """`data` cut into chunks of `sizes` (an int: that size throughout); every stored_every-th chunk is uncompressed; `between`:
    chunks put in front of every data chunk"""
    if isinstance(sizes, int):
        sizes = [sizes] * (len(data) // sizes) + ([len(data) % sizes] if len(data) % sizes else [])
    parts, p = [], 0
    for k, n in enumerate(sizes):
        parts += list(between)
        parts.append(data_chunk(data[p:p + n], compressed=not (stored_every and k % stored_every == stored_every - 1)))
        p += n
    assert p == len(data)
    return stream(parts)
