"""The block finder's definitions (include/compu_hip.h, "one large stream: block starts") restated in Python: the candidate rule,
the starts of a buffer's chunks, and -- so that a start can be called true or false -- a small inflate that walks a raw deflate
stream and lists its block boundaries.  Shared by tests/test_inflate_parallel_cpu.py and tests/test_inflate_parallel_gpu.py."""
from functools import lru_cache

from deflate_writer import CL_ORDER, DBASE, DEXT, FIXED_DIST, FIXED_LIT, LBASE, LEXT


def bits(data, p, n):
    """n stream bits from bit p on, first bit lowest; bytes behind the buffer read as zero"""
    v = int.from_bytes(data[p >> 3:(p >> 3) + 6], "little") >> (p & 7)
    return v & ((1 << n) - 1)


def set_ok(lens, code_lengths=False):
    """zlib's inflate_table verdict on a set of code lengths: not over-subscribed; incomplete only as a single code of length 1, and
    never for the code-length alphabet; a set without codes passes"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    left, maxlen = 1, 0
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            return False
        if count[l]:
            maxlen = l
    if maxlen == 0:
        return True
    return not (left > 0 and (code_lengths or maxlen != 1))


def decoder_of(lens):
    """{(length, code with its first bit highest): symbol} of a canonical code"""
    table, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table


def read_sym(data, p, table, maxlen=15):
    """-> (symbol, bits) of the code at bit p, or (None, 0)"""
    code = 0
    for l in range(1, maxlen + 1):
        code = (code << 1) | bits(data, p + l - 1, 1)
        if (l, code) in table:
            return table[(l, code)], l
    return None, 0


def dynamic_header(data, p):
    """The dynamic block header whose three block bits start at bit p, by the decoder's rules -> (lit lens, dist lens, the bit
    behind the header), or None where the decoder's header path would stop.  BFINAL is not looked at."""
    end = 8 * len(data)
    if p + 17 > end or bits(data, p + 1, 2) != 2:
        return None
    nlen, ndist, ncode = bits(data, p + 3, 5) + 257, bits(data, p + 8, 5) + 1, bits(data, p + 13, 4) + 4
    if nlen > 286 or ndist > 30:
        return None
    q = p + 17
    if q + 3 * ncode > end:
        return None
    cl = [0] * 19
    for k in range(ncode):
        cl[CL_ORDER[k]] = bits(data, q + 3 * k, 3)
    q += 3 * ncode
    if not any(cl):  # zlib reads such a set as symbol 0 in one bit: every length is 0, the end-of-block code among them
        return None
    if not set_ok(cl, code_lengths=True):
        return None
    table = decoder_of(cl)
    lens, total = [], nlen + ndist
    while len(lens) < total:
        s, n = read_sym(data, q, table, 7)
        assert s is not None  # the code is complete
        eb = {16: 2, 17: 3, 18: 7}.get(s, 0)
        if q + n + eb > end:
            return None
        x = bits(data, q + n, eb)
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                return None
            lens += [lens[-1]] * (3 + x)
        else:
            lens += [0] * ((3 if s == 17 else 11) + x)
        if len(lens) > total:
            return None
        q += n + eb
    if lens[256] == 0:
        return None
    lit, dist = lens[:nlen], lens[nlen:]
    if not set_ok(lit) or not set_ok(dist):
        return None
    return lit, dist, q


def is_candidate(data, p):
    return bits(data, p, 3) == 4 and dynamic_header(data, p) is not None


def find_starts(data, first_bit, chunk_bytes):
    """the start of every chunk k >= 1 that has one, ascending"""
    out, n_chunks = [], -(-len(data) // chunk_bytes)
    for k in range(1, n_chunks):
        lo, hi = max(8 * k * chunk_bytes, first_bit + 1), min(8 * (k + 1) * chunk_bytes, 8 * len(data))
        for p in range(lo, hi):
            if bits(data, p, 3) == 4 and bits(data, p + 3, 5) <= 29 and bits(data, p + 8, 5) <= 29 and is_candidate(data, p):
                out.append(p)
                break
    return out


def true_starts(bounds, first_bit, chunk_bytes, length):
    """what the finder answers when no position but a real boundary is a candidate: per chunk the first boundary of a non-final
    dynamic block.  bounds: [(bit, out, btype, final)]"""
    out, n_chunks = [], -(-length // chunk_bytes)
    for k in range(1, n_chunks):
        lo, hi = 8 * k * chunk_bytes, 8 * (k + 1) * chunk_bytes
        hit = [b for b, _, t, f in bounds if lo <= b < hi and b > first_bit and t == 2 and not f]
        if hit:
            out.append(hit[0])
    return out


def first_bit_of(data, fmt):
    """the bit of the first block header behind a plain wrapper: fmt "raw" | "zlib" | "gzip" """
    if fmt == "raw":
        return 0
    if fmt == "zlib":
        return 16
    flg, k = data[3], 10
    if flg & 4:
        k += 2 + data[k] + 256 * data[k + 1]
    for bit in (8, 16):
        if flg & bit:
            k = data.index(0, k) + 1
    if flg & 2:
        k += 2
    return 8 * k


def walk(data, first_bit):
    """A small inflate: the blocks of the stream whose first header is at first_bit -> ([(bit, out, btype, final)], content)."""
    out, p, bounds = bytearray(), first_bit, []
    fixed = (decoder_of(FIXED_LIT), decoder_of(FIXED_DIST))
    while True:
        final, btype = bits(data, p, 1), bits(data, p + 1, 2)
        bounds.append((p, len(out), btype, bool(final)))
        if btype == 0:
            q = (p + 3 + 7) & ~7
            n = bits(data, q, 16)
            assert n ^ 0xFFFF == bits(data, q + 16, 16)
            out += data[(q >> 3) + 4:(q >> 3) + 4 + n]
            p = q + 32 + 8 * n
        else:
            assert btype in (1, 2)
            if btype == 1:
                (lt, dt), p = fixed, p + 3
            else:
                lit, dist, p = dynamic_header(data, p)
                lt, dt = decoder_of(lit), decoder_of(dist)
            while True:
                s, n = read_sym(data, p, lt)
                assert s is not None
                p += n
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    length = LBASE[s - 257] + bits(data, p, LEXT[s - 257])
                    p += LEXT[s - 257]
                    d, n = read_sym(data, p, dt)
                    assert d is not None
                    dist = DBASE[d] + bits(data, p + n, DEXT[d])
                    p += n + DEXT[d]
                    assert dist <= len(out)
                    for _ in range(length):
                        out.append(out[-dist])
        if final:
            return bounds, bytes(out)


@lru_cache(maxsize=None)
def walk_cached(data, first_bit):
    return walk(data, first_bit)
