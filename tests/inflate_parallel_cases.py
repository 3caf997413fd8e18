"""Inputs of the block-finder tests: (name, bytes, first_bit) triples.  Files compressed by the system zlib with small blocks, and
streams built with tests/deflate_writer.py so that the bit of every block is known: boundaries on a chunk's first and last bit, a
header cut by the end of the buffer, a stored payload that spells a header.  Shared by tests/test_inflate_parallel_cpu.py and
tests/test_inflate_parallel_gpu.py."""
import random
import zlib
from functools import lru_cache

import deflate_writer as W
import inflate_index_cases as IC
import inflate_parallel_ref as R

CHUNKS = (512, 2048)


def _text(rng, n):
    return [rng.choice(b"etaoin shrdlu\n") for _ in range(n)]


@lru_cache(maxsize=None)
def alice(fmt, mem_level=2, level=6):
    """alice29.txt with the small blocks of a small memLevel (117 blocks at memLevel 2)"""
    co = zlib.compressobj(level, zlib.DEFLATED, {"raw": -15, "zlib": 15, "gzip": 31}[fmt], mem_level)
    data = co.compress(IC.file_content("alice")) + co.flush()
    return data, R.first_bit_of(data, fmt)


def _stored_to(d, byte):
    """a stored block of zeros (no bit pattern 100: never a candidate) whose payload ends at byte offset `byte` of the body"""
    start = (d.w.n + 3 + 7) // 8 + 4
    assert byte >= start and byte - start < 65536, (byte, start)
    d.stored(bytes(byte - start))
    assert d.w.n == 8 * byte


@lru_cache(maxsize=None)
def chunk_edges(chunk_bytes):
    """raw deflate: a dynamic block whose header starts at exactly bit 8 B (chunk 1's first bit) and one at 8 * 3 B - 1 (chunk 2's
    last bit) -> (Stream, (the two bits))"""
    rng, b = random.Random(17), chunk_bytes
    d = W.Deflate()
    _stored_to(d, b)
    d.dynamic(_text(rng, 300) + [("m", 30, 100)])
    first = d.blocks[-1][0]
    # 19 + 10 + 10 bits of fixed blocks bring a byte boundary to phase 7
    _stored_to(d, (8 * 3 * b - 1 - 39) // 8)
    d.fixed([200]).fixed([]).fixed([])
    d.dynamic(_text(rng, 200) + [("m", 258, 7)])
    last = d.blocks[-1][0]
    d.fixed(_text(rng, 5), final=True)
    assert (first, last) == (8 * b, 8 * 3 * b - 1)
    return W.wrap(d, "raw"), (first, last)


@lru_cache(maxsize=None)
def decoy(chunk_bytes):
    """raw deflate: a stored block whose payload is the body of another writer's dynamic block, placed so that it is chunk 1's
    first candidate; the real dynamic blocks follow -> (Stream, the decoy's bit)"""
    rng, b = random.Random(23), chunk_bytes
    other = W.Deflate()
    other.dynamic(_text(rng, 150) + [("m", 10, 20)])
    d = W.Deflate()
    d.dynamic(_text(rng, 100))
    _stored_to(d, b + 16)
    d.stored(other.body())
    at = d.layout[-1].bit
    assert 8 * b <= at < 16 * b
    for i in range(6 * chunk_bytes // 512):  # three chunks and more of real blocks behind it
        d.dynamic(_text(rng, 400 + 50 * (i % 6)) + [("m", 100, 333)])
    d.dynamic(_text(rng, 20), final=True)
    return W.wrap(d, "raw"), at


def cut_header(chunk_bytes):
    """chunk_edges cut inside, and exactly at the end of, the header of its last dynamic block -> [(name, bytes)]"""
    s, (_, last) = chunk_edges(chunk_bytes)
    _, _, q = R.dynamic_header(s.data, last)
    whole = (q + 7) // 8
    return [("cut-in-header", s.data[:whole - 1]), ("cut-behind-header", s.data[:whole]), ("cut-in-fields", s.data[:(last + 17) // 8])]


EDGE_CHUNK = 256  # chunk_bytes of the built streams below


@lru_cache(maxsize=None)
def built_edges(fmt):
    """Dynamic blocks only where it matters, so that they are starts at chunk_bytes 256: early chunks with less than 32 KiB in front
    of them; an empty dynamic block and a text block each directly behind a stored block that ends on a chunk's first bit; a block
    whose first token is a length-258 match at distance 32 768; one whose first token starts 100 bytes inside the window and runs
    into the chunk; then eight blocks made only of matches at distance 32 768 (chunks of 100 KiB and more, whose every byte has
    travelled through every window in front of it); chunks shorter than 32 KiB behind them."""
    rng, b = random.Random(29), EDGE_CHUNK
    d = W.Deflate()
    for i in range(14):
        d.dynamic(_text(rng, 1500 + 100 * i) + [("m", 50 + i, 1000)])
    _stored_to(d, -(-(d.w.n + 40) // (8 * b)) * b)
    d.dynamic([])
    d.dynamic(_text(rng, 900))
    _stored_to(d, -(-(d.w.n + 40) // (8 * b)) * b)
    d.dynamic(_text(rng, 12000))
    assert len(d.content) > 33000
    for i in range(3):
        d.dynamic([("m", 258, 32768)] + _text(rng, 700))
        d.dynamic([("m", 258, 100), ("m", 3, 1)] + _text(rng, 650 + 10 * i))
    for i in range(8):
        d.dynamic([("m", 258, 32768)] * (400 + 50 * i))
    for i in range(6):
        d.dynamic(_text(rng, 500) + [("m", 258, 32768), ("m", 200, 20000)])
    d.dynamic(_text(rng, 30), final=True)
    return W.wrap(d, fmt, header=IC.GZIP_FIELDS if fmt == "gzip" else None)


@lru_cache(maxsize=None)
def too_far_back():
    """raw deflate: a few chunks in, a match reaches in front of stream byte 0"""
    rng = random.Random(31)
    d = W.Deflate()
    for i in range(4):
        d.dynamic(_text(rng, 700 + 20 * i))
    d.dynamic(_text(rng, 300) + [("m", 10, 5000)] + _text(rng, 300))
    for i in range(3):
        d.dynamic(_text(rng, 600))
    d.dynamic(_text(rng, 30), final=True)
    return W.wrap(d, "raw")


def finder_inputs(chunk_bytes):
    """every input of the finder tests at this chunk size: [(name, bytes, first_bit)]"""
    out = []
    for fmt in IC.WRAPPERS:
        data, fb = alice(fmt)
        out.append((f"alice-{fmt}", data, fb))
    for fmt in ("raw", "gzip"):
        s = IC.phases(fmt)
        out.append((f"phases-{fmt}", s.data, 8 * s.hdr_len))
    out.append(("chunk-edges", chunk_edges(chunk_bytes)[0].data, 0))
    out += [(name, data, 0) for name, data in cut_header(chunk_bytes)]
    out.append(("decoy", decoy(chunk_bytes)[0].data, 0))
    return out
