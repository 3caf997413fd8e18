"""The Snappy rules of include/compu_hip.h ("Snappy: blocks and framed streams") in plain Python: the block decode, CRC-32C, the walk
over a framed stream's chunk headers and the frame decode, each with status, out_len and in_used.  Written from the header's text,
not from the library's code: the tests hold the host decoder and the kernels against it."""

NEED_INPUT, NEED_OUTPUT, FINISHED = 0, 1, 2
E_PREAMBLE, E_OFFSET, E_LENGTH, E_HEADER, E_CHUNK, E_CHUNK_SIZE, E_BLOCK, E_CHECKSUM = -210, -211, -212, -213, -214, -215, -216, -217
OK, TRUNCATED, BAD_HEADER, TOO_LARGE = 0, 1, 2, 3  # CHIP_ZPLAN_*
MAX_BLOCKS = 1 << 20  # CHIP_ZPLAN_MAX_BLOCKS
IDENT = b"\xff\x06\x00\x00sNaPpY"
CHUNK_MAX = 65536

_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _TABLE.append(_c)


def crc32c(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def mask(x):
    return (((x >> 15) | (x << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _block(data, p, end, room, framed):
    """the block rules over data[p:end] with `room` bytes of output left (None: the size pass): (content, status, where it stopped)"""
    start, n, shift = p, 0, 0
    for i in range(5):
        if p == end:
            return b"", NEED_INPUT, start
        b = data[p]
        p += 1
        if i == 4 and b >= 16:
            return b"", E_PREAMBLE, start
        n |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    if framed and n > CHUNK_MAX:
        return b"", E_CHUNK_SIZE, start
    if room is not None and n > room:
        return b"", NEED_OUTPUT, start
    out = bytearray()
    while True:
        t = p
        if p == end:
            return bytes(out), (FINISHED if len(out) == n else NEED_INPUT), t
        if len(out) == n:
            return bytes(out), E_LENGTH, t
        tag = data[p]
        p += 1
        if tag & 3 == 0:
            length = tag >> 2
            if length >= 60:
                nb = length - 59
                if end - p < nb:
                    return bytes(out), NEED_INPUT, t
                length = int.from_bytes(data[p:p + nb], "little")
                p += nb
            length += 1
            if length > end - p:
                return bytes(out), NEED_INPUT, t
            if length > n - len(out):
                return bytes(out), E_LENGTH, t
            out += data[p:p + length]
            p += length
            continue
        nb = (0, 1, 2, 4)[tag & 3]
        if end - p < nb:
            return bytes(out), NEED_INPUT, t
        extra = int.from_bytes(data[p:p + nb], "little")
        p += nb
        if tag & 3 == 1:
            m, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | extra
        else:
            m, off = (tag >> 2) + 1, extra
        if off == 0 or off > len(out):
            return bytes(out), E_OFFSET, t
        if m > n - len(out):
            return bytes(out), E_LENGTH, t
        if off >= m:
            out += out[len(out) - off:len(out) - off + m]
        else:
            period = bytes(out[-off:])
            out += (period * (m // off + 1))[:m]


def block_decode(data, cap):
    """(content, out_len, in_used, status) of one raw block with cap bytes of room (None: ample, what the size pass answers)"""
    content, status, t = _block(data, 0, len(data), cap, False)
    used = len(data) if status == FINISHED else t
    return content, len(content), used, status


def _start(data):
    if len(data) < 4:
        return NEED_INPUT
    k = min(len(data), 10)
    if data[:k] != IDENT[:k]:
        return E_HEADER
    return NEED_INPUT if len(data) < 10 else None


def _header(data, q):
    """("data", type, s, crc) / ("skip", s) / a status"""
    n = len(data)
    if q == n:
        return FINISHED
    if n - q < 4:
        return NEED_INPUT
    kind, s = data[q], int.from_bytes(data[q + 1:q + 4], "little")
    if n - q - 4 < s:
        return NEED_INPUT
    if kind == 0xFF:
        return ("skip", s) if data[q:q + 10] == IDENT else E_HEADER
    if kind >= 0x80:
        return ("skip", s)
    if kind >= 2:
        return E_CHUNK
    if s < 4:
        return E_CHUNK_SIZE
    return ("data", kind, s, int.from_bytes(data[q + 4:q + 8], "little"))


def frame_decode(data, cap, checks=True):
    """(content, out_len, in_used, status) of one framed stream; cap None: ample; checks=False: the CRCs are not compared (the
    size pass)"""
    st = _start(data)
    if st is not None:
        return b"", 0, 0, st
    out, q = bytearray(), 10
    while True:
        h = _header(data, q)
        if h == FINISHED:
            return bytes(out), len(out), len(data), FINISHED
        if not isinstance(h, tuple):
            return bytes(out), len(out), q, h
        if h[0] == "skip":
            q += 4 + h[1]
            continue
        _, kind, s, want = h
        room = None if cap is None else cap - len(out)
        if kind == 1:
            if s - 4 > CHUNK_MAX:
                return bytes(out), len(out), q, E_CHUNK_SIZE
            if room is not None and s - 4 > room:
                return bytes(out), len(out), q, NEED_OUTPUT
            content = data[q + 8:q + 4 + s]
        else:
            content, status, _ = _block(data, q + 8, q + 4 + s, room, True)
            if status != FINISHED:
                out += content
                return bytes(out), len(out), q, (E_BLOCK if status == NEED_INPUT else status)
        if checks and mask(crc32c(content)) != want:
            return bytes(out), len(out), q, E_CHECKSUM
        out += content
        q += 4 + s


def chunks_walk(data, max_chunks=None):
    """chip_snappy_chunks: ([(offset, s, type, crc)] of the first min(n_chunks, max_chunks), (n_chunks, n_skipped, in_used, status))"""
    st = _start(data)
    if st is not None:
        return [], (0, 0, 0, TRUNCATED if st == NEED_INPUT else BAD_HEADER)
    rows, n, skipped, q = [], 0, 0, 10
    while True:
        h = _header(data, q)
        if h == FINISHED:
            status = OK
            break
        if h == NEED_INPUT:
            status = TRUNCATED
            break
        if not isinstance(h, tuple):
            status = BAD_HEADER
            break
        if h[0] == "skip":
            if skipped + 1 > MAX_BLOCKS:
                status = TOO_LARGE
                break
            skipped += 1
            q += 4 + h[1]
            continue
        if n + 1 > MAX_BLOCKS:
            status = TOO_LARGE
            break
        if max_chunks is None or n < max_chunks:
            rows.append((q, h[2], h[1], h[3]))
        n += 1
        q += 4 + h[2]
    return rows, (n, skipped, q, status)
