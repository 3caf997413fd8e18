"""The definitions of the checkpoint index (include/compu_hip.h, "one large stream"), restated in Python: the points of a stream the
test wrote itself, from the block records of tests/deflate_writer.py; the chunks of an index (chip_inflate_index_units_host's
arithmetic and its layout check); and one chunk decoded by the system zlib from its bit position with its window as the dictionary,
which is what makes a chunk an independent unit.  Shared by tests/test_inflate_index_cpu.py and tests/test_inflate_index_gpu.py."""
import zlib
from functools import lru_cache

import deflate_writer as W

WINDOW = 32768
GZPLAN_WINDOW = (1 << 29) - 64
CAP_MAX = (1 << 32) - 16 - WINDOW
READ_OK, READ_BAD_LAYOUT = 0, 2
FMT = {"raw": -15, "zlib": 15, "gzip": 31}
WRAP = {"raw": 0, "zlib": 1, "gzip": 2}


def check_of(wrap, content):
    """the running check of a prefix of the content: CRC-32 (gzip), Adler-32 (zlib), 0 (raw)"""
    return zlib.crc32(content) if wrap == 2 else zlib.adler32(content) if wrap == 1 else 0


def boundaries(stream):
    """[(first bit of block j's header, decoded bytes in front of block j)] from the writer's records"""
    heads = [r for r in stream.layout if r.kind == "block"]
    assert [r.bit for r in heads] == [b[0] for b in stream.blocks]
    return [(r.bit, r.out) for r in heads]


def points(stream, wrap, spacing, n_blocks=None):
    """the walk: [(bit, out, check)] over the first n_blocks boundaries (None: all)"""
    spacing = spacing or 1 << 20
    out = []
    for j, (bit, o) in enumerate(boundaries(stream)[:n_blocks]):
        if j == 0 or o - out[-1][1] >= spacing:
            assert j > 0 or o == 0
            out.append((bit, o, check_of(wrap, stream.content[:o])))
    return out


def window(content, o):
    return content[max(0, o - WINDOW):o]


def units(wrap, length, pt_bit, pt_out, pt_check, total_out):
    """-> (status, bad_index, rows): rows[k] = (in_off, in_len, out_cap, win_len, [six resume words]); no rows on a bad layout"""
    n = len(pt_bit)
    rows = []
    for k in range(n):
        bit, o, more = pt_bit[k], pt_out[k], k + 1 < n
        end_out = pt_out[k + 1] if more else total_out
        end_in = (pt_bit[k + 1] + 7) // 8 if more else length
        in_off = (bit >> 3) - (1 if bit % 8 == 0 and bit != 0 else 0)
        bad = ((k == 0 and o != 0) or bit >= 8 * length or (more and pt_bit[k + 1] <= bit) or end_out < o or end_out - o > CAP_MAX
               or end_in - in_off > GZPLAN_WINDOW)
        if bad:
            return READ_BAD_LAYOUT, k, []
        wl = min(WINDOW, o)
        rows.append((in_off, end_in - in_off, end_out - o, wl,
                     [bit - 8 * in_off, wl, wrap, pt_check[k], o & 0xFFFFFFFF, (o - wl) & 0xFFFFFFFF]))
    return READ_OK, 0, rows


@lru_cache(maxsize=None)
def _prefix(phase):
    """(bytes, bits) of blocks without output whose length in bits is `phase` modulo 8: what zlib reads in front of a chunk that
    starts `phase` bits into a byte (the stream cannot be shifted instead: stored blocks align to ITS bytes)"""
    if phase == 0:
        return b"", 0
    for nlit in range(257, 287):
        for ndist in range(1, 31):
            for k in range(4):
                d = W.Deflate()
                d.dynamic([], nlit=nlit, ndist=ndist)
                for _ in range(k):
                    d.fixed([])
                if d.w.n % 8 == phase:
                    return d.body(), d.w.n
    raise AssertionError(phase)


def zlib_chunk(data, bit, win, n_out, end_bit=None):
    """what the system zlib decodes from bit offset `bit` of `data` (up to the byte that holds end_bit, if given) with `win` in
    front: at most n_out bytes; None if zlib refuses the bits"""
    phase = bit & 7
    pre, nbits = _prefix(phase)
    end = len(data) if end_bit is None else (end_bit + 7) // 8
    body = bytearray(data[bit >> 3:end])
    if phase:
        body[0] = (body[0] & ~((1 << phase) - 1) & 255) | pre[-1]
        body = bytearray(pre[:-1]) + body
    d = zlib.decompressobj(-15, zdict=win) if win else zlib.decompressobj(-15)
    try:
        return d.decompress(bytes(body), n_out) if n_out else b""
    except zlib.error:
        return None
