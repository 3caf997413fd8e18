"""The LZ4 rules of include/compu_hip.h ("LZ4: blocks and frames") in plain Python: XXH32, the block decode with its statuses,
the frame decode, and the walk over a frame's block headers.  Written from the format documents and the header comment, not from
the library's code: the tests compare the library with this."""
import struct

NEED_INPUT, NEED_OUTPUT, FINISHED = 0, 1, 2
E_HEADER, E_DICT, E_BLOCK_SIZE, E_BLOCK, E_OFFSET, E_BLOCK_CHECKSUM, E_CONTENT_SIZE, E_CONTENT_CHECKSUM = range(-200, -208, -1)
MAGIC = 0x184D2204
OK, TRUNCATED, BAD_HEADER, TOO_LARGE = 0, 1, 2, 3
UNSIZED = 0xFFFFFFFFFFFFFFFF
STORED, LAST = 1, 2
MAX_BLOCKS = 1 << 20

P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
M32 = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def xxh32(data, seed=0):
    data = bytes(data)
    n, k = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M32, (seed + P2) & M32, seed & M32, (seed - P1) & M32]
        words = struct.unpack_from("<%dI" % (n // 16 * 4), data)
        for i in range(0, len(words), 4):
            for c in range(4):
                v[c] = (_rotl((v[c] + words[i + c] * P2) & M32, 13) * P1) & M32
        k = n // 16 * 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M32
    else:
        h = (seed + P5) & M32
    h = (h + n) & M32
    while k + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, k)[0] * P3) & M32, 17) * P4) & M32
        k += 4
    while k < n:
        h = (_rotl((h + data[k] * P5) & M32, 11) * P1) & M32
        k += 1
    h ^= h >> 15
    h = (h * P2) & M32
    h ^= h >> 13
    h = (h * P3) & M32
    h ^= h >> 16
    return h


def block_decode(data, cap=None, history=b"", block_max=None, count_only=False):
    """One block by the block rules: (content, out_len, in_used, status).  cap None: no limit (the size pass).  history: the bytes
    an offset may reach in front of the block (a linked frame).  block_max: the growth beyond which the verdict is E_BLOCK_SIZE
    (frames only).  count_only: no bytes are produced (content is b""), lengths may be astronomic."""
    n, p, o = len(data), 0, 0
    out = bytearray()
    hist = len(history)

    def ext(q, length):
        while True:
            if q >= n:
                return None, None
            b = data[q]
            q += 1
            length += b
            if b != 255:
                return q, length

    while True:
        t = p
        if p >= n:
            return bytes(out), o, t, NEED_INPUT
        token = data[p]
        q = p + 1
        ll = token >> 4
        if ll == 15:
            q, ll = ext(q, ll)
            if q is None:
                return bytes(out), o, t, NEED_INPUT
        if ll > n - q:
            return bytes(out), o, t, NEED_INPUT
        if block_max is not None and o + ll > block_max:
            return bytes(out), o, t, E_BLOCK_SIZE
        if cap is not None and ll > cap - o:
            return bytes(out), o, t, NEED_OUTPUT
        if not count_only:
            out += data[q:q + ll]
        o += ll
        q += ll
        if q == n:
            return bytes(out), o, n, FINISHED
        if n - q < 2:
            return bytes(out), o, t, NEED_INPUT
        off = data[q] | (data[q + 1] << 8)
        q += 2
        if off == 0 or off > o + hist:
            return bytes(out), o, t, E_OFFSET
        ml = token & 15
        if ml == 15:
            q, ml = ext(q, ml)
            if q is None:
                return bytes(out), o, t, NEED_INPUT
        ml += 4
        if block_max is not None and o + ml > block_max:
            return bytes(out), o, t, E_BLOCK_SIZE
        if cap is not None and ml > cap - o:
            return bytes(out), o, t, NEED_OUTPUT
        if not count_only:
            for _ in range(ml):
                k = len(out) - off
                out.append(out[k] if k >= 0 else history[hist + k])
        o += ml
        p = q


def frame_header(data):
    """(status, dict): status None when the header is accepted"""
    n = len(data)
    if n < 7:
        return NEED_INPUT, None
    if struct.unpack_from("<I", data)[0] != MAGIC:
        return E_HEADER, None
    flg, bd = data[4], data[5]
    code = (bd >> 4) & 7
    if flg >> 6 != 1 or flg & 2 or bd & 0x8F or code < 4:
        return E_HEADER, None
    hs = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if n < hs:
        return NEED_INPUT, None
    if data[hs - 1] != (xxh32(data[4:hs - 1]) >> 8) & 0xFF:
        return E_HEADER, None
    if flg & 1:
        return E_DICT, None
    return None, dict(flg=flg, bd=bd, hs=hs, block_max=1 << (8 + 2 * code), indep=bool(flg & 0x20), bchk=bool(flg & 0x10),
                      size=struct.unpack_from("<Q", data, 6)[0] if flg & 8 else None, cchk=bool(flg & 4))


def frame_decode(data, cap=None, checks=True):
    """One frame by the frame rules: (content, out_len, in_used, status).  cap None: no limit.  checks False: the two XXH32
    comparisons of blocks and content are not made (the size pass)."""
    data = bytes(data)
    n = len(data)
    st, h = frame_header(data)
    if st is not None:
        return b"", 0, 0, st
    out = bytearray()
    q = h["hs"]
    extra = 4 if h["bchk"] else 0
    while True:
        b = q
        if n - q < 4:
            return bytes(out), len(out), b, NEED_INPUT
        w = struct.unpack_from("<I", data, q)[0]
        if w == 0:
            q += 4
            break
        size = w & 0x7FFFFFFF
        if size > h["block_max"]:
            return bytes(out), len(out), b, E_BLOCK_SIZE
        if n - q - 4 < size + extra:
            return bytes(out), len(out), b, NEED_INPUT
        body = data[q + 4:q + 4 + size]
        before = len(out)
        if w >> 31:
            if cap is not None and size > cap - len(out):
                return bytes(out), len(out), b, NEED_OUTPUT
            out += body
        else:
            got, _, _, bs = block_decode(body, None if cap is None else cap - len(out), b"" if h["indep"] else bytes(out[-65535:]), h["block_max"])
            out += got
            if bs != FINISHED:
                return bytes(out), len(out), b, E_BLOCK if bs == NEED_INPUT else bs
        if extra and checks and struct.unpack_from("<I", data, q + 4 + size)[0] != xxh32(body):
            return bytes(out[:before]), before, b, E_BLOCK_CHECKSUM
        q += 4 + size + extra
    if h["cchk"] and n - q < 4:
        return bytes(out), len(out), q - 4, NEED_INPUT
    end = q + (4 if h["cchk"] else 0)
    if h["size"] is not None and h["size"] != len(out):
        return bytes(out), len(out), end, E_CONTENT_SIZE
    if h["cchk"] and checks and struct.unpack_from("<I", data, q)[0] != xxh32(out):
        return bytes(out), len(out), end, E_CONTENT_CHECKSUM
    return bytes(out), len(out), end, FINISHED


def blocks_walk(data, max_blocks=None):
    """chip_lz4_blocks_host's answer: (records [(offset, size, flags, checksum)], (n_blocks, in_used, content_size, block_max, flg, bd,
    header_bytes, content_checksum, status))"""
    data = bytes(data)
    n = len(data)
    st, h = frame_header(data)
    if st is not None:
        return [], (0, 0, UNSIZED, 0, 0, 0, 0, 0, TRUNCATED if st == NEED_INPUT else BAD_HEADER)
    recs = []
    q = h["hs"]
    extra = 4 if h["bchk"] else 0

    def done(status, in_used=0, cc=0):
        k = len(recs) if max_blocks is None else min(len(recs), max_blocks)
        return recs[:k], (len(recs), in_used, UNSIZED if h["size"] is None else h["size"], h["block_max"], h["flg"], h["bd"], h["hs"], cc, status)

    while True:
        if n - q < 4:
            return done(TRUNCATED)
        w = struct.unpack_from("<I", data, q)[0]
        if w == 0:
            if recs and (max_blocks is None or len(recs) <= max_blocks):
                o, s, f, c = recs[-1]
                recs[-1] = (o, s, f | LAST, c)
            q += 4
            break
        size = w & 0x7FFFFFFF
        if size > h["block_max"]:
            return done(BAD_HEADER)
        if len(recs) + 1 > MAX_BLOCKS:
            return done(TOO_LARGE)
        if n - q - 4 < size + extra:
            return done(TRUNCATED)
        recs.append((q, size, STORED if w >> 31 else 0, struct.unpack_from("<I", data, q + 4 + size)[0] if extra else 0))
        q += 4 + size + extra
    cc = 0
    if h["cchk"]:
        if n - q < 4:
            return done(TRUNCATED)
        cc = struct.unpack_from("<I", data, q)[0]
        q += 4
    return done(OK, q, cc)
