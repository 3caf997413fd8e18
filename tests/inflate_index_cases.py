"""Streams for the checkpoint-index tests.  Built ones (tests/deflate_writer.py: the first bit and the decoded count of every block
are known): `phases`, fixed, dynamic, stored and empty blocks whose boundaries fall on every bit phase; `edges`, the window edges of
a chunk; `damage`, stored payloads between Huffman blocks, where one flipped byte changes the content and nothing else.  And whole
files compressed by the system zlib.  Shared by tests/test_inflate_index_cpu.py and tests/test_inflate_index_gpu.py."""
import os
import random
import zlib
from functools import lru_cache

import deflate_writer as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WRAPPERS = ("raw", "zlib", "gzip")
GZIP_FIELDS = W.gzip_header(extra=b"ab\x02\x00xy", name=b"file.txt")  # FEXTRA and FNAME: the deflate stream starts at byte 27


def _text(rng, n):
    return [rng.choice(b"etaoin shrdlu\n") for _ in range(n)]


def _wrap(d, fmt, **kw):
    return W.wrap(d, fmt, header=GZIP_FIELDS if fmt == "gzip" and "header" not in kw else kw.pop("header", None), **kw)


@lru_cache(maxsize=None)
def phases(fmt, final_tokens=True):
    """60-odd blocks of every kind; lengths in bits of all residues, so the boundaries visit every phase"""
    rng = random.Random(11)
    d = W.Deflate()
    d.fixed(_text(rng, 5))
    for i in range(64):
        kind = i % 8
        if kind == 0:
            d.fixed([200 + i % 50])                           # one 9-bit literal: 19 bits
        elif kind == 1:
            d.fixed([])                                       # empty: 10 bits, never a point
        elif kind == 2:
            d.stored(bytes(_text(rng, 3 + i)))                # from whatever phase the block before left
        elif kind == 3:
            d.fixed(_text(rng, 2) + [("m", 3 + i % 30, 1 + i % 7)])  # directly behind a stored block: phase 0
        elif kind == 4:
            d.dynamic(_text(rng, 40 + i) + [("m", 20, 17), 255, ("m", 258, 1)])
        elif kind == 5:
            d.stored(b"")                                     # empty stored block
        elif kind == 6:
            d.fixed(_text(rng, 1 + i % 3) + [150])
        else:
            d.dynamic([("m", 9, 4)] + _text(rng, 10), nlit=270, ndist=8)
    d.fixed(_text(rng, 7) if final_tokens else [], final=True)
    return _wrap(d, fmt)


@lru_cache(maxsize=None)
def edges(fmt):
    """points at 1 000 (a match reaches content byte 0), at exactly 32 768 (a match at distance 32 768 is the chunk's first token),
    and further on one whose first token is a length-258 match at distance 100: it starts in the window and runs into the chunk"""
    rng = random.Random(5)
    d = W.Deflate()
    d.stored(bytes(rng.randrange(256) for _ in range(1000)))
    d.fixed([("m", 50, 1000), 1, 2, 3] + _text(rng, 100))
    d.stored(bytes(rng.randrange(256) for _ in range(32768 - len(d.content))))
    assert len(d.content) == 32768
    d.fixed([("m", 258, 32768), ("m", 258, 32768), 7] + _text(rng, 30))
    d.dynamic(_text(rng, 3000) + [("m", 100, 2000)])
    d.stored(bytes(rng.randrange(256) for _ in range(20000)))
    d.fixed([("m", 258, 100), ("m", 258, 32768)] + _text(rng, 20))
    d.dynamic([("m", 258, 32768), ("m", 3, 1)] + _text(rng, 500), final=True)
    return _wrap(d, fmt)


DAMAGE_BLOCK = 7  # a stored block of the `damage` stream


@lru_cache(maxsize=None)
def damage(fmt):
    rng = random.Random(3)
    d = W.Deflate()
    for i in range(5):
        d.dynamic(_text(rng, 600) + [("m", 40, 333)] + _text(rng, 50))
        d.stored(bytes(rng.randrange(256) for _ in range(700)))
        d.fixed(_text(rng, 100) + [("m", 30, 1000), ("m", 258, 1500)])
    d.fixed(_text(rng, 9), final=True)
    return _wrap(d, fmt)


def flipped_stored_byte(stream, block):
    """`stream.data` with one payload byte of stored block `block` changed -> (data, the content offset of that byte)"""
    rec = next(r for r in stream.layout if r.kind == "stored" and r.block == block)
    at = rec.bit // 8 + rec.nbits // 16
    data = bytearray(stream.data)
    data[at] ^= 0x55
    return bytes(data), rec.out + rec.nbits // 16


@lru_cache(maxsize=None)
def file_content(name):
    if name == "alice":
        return open(os.path.join(GOLDEN, "alice29.txt"), "rb").read()
    from bench_support import synth

    return synth.payloads(40, threads=4).tobytes()  # 2.5 MiB


@lru_cache(maxsize=None)
def compressed(name, level, fmt):
    co = zlib.compressobj(level, zlib.DEFLATED, {"raw": -15, "zlib": 15, "gzip": 31}[fmt])
    return co.compress(file_content(name)) + co.flush()
