"""Inputs of the slab-decode tests (chip_inflate_parallel_next): the streams of tests/inflate_parallel_cases.py and
tests/inflate_index_cases.py with the chunk size and the slabs each is cut into.  Shared by tests/test_inflate_stream_cpu.py and
tests/test_inflate_stream_gpu.py."""
import zlib
from functools import lru_cache

import deflate_writer as W
import inflate_index_cases as IC
import inflate_parallel_cases as PC

FMT = {"raw": -15, "zlib": 15, "gzip": 31}
TRAILER = {"raw": 0, "zlib": 4, "gzip": 8}
ALICE_CHUNK, ALICE_SLABS = 512, (4096, 5001, 8192)
EDGE_SLABS = (8192, 9001)


@lru_cache(maxsize=None)
def parallel_inputs():
    """[(name, fmt, data, first_bit, chunk_bytes, slabs)]: every call of every one of them runs on the parallel path"""
    out = []
    for fmt in IC.WRAPPERS:
        data, fb = PC.alice(fmt)
        out.append((f"alice-{fmt}", fmt, data, fb, ALICE_CHUNK, ALICE_SLABS))
    for fmt in IC.WRAPPERS:
        s = PC.built_edges(fmt)
        out.append((f"edges-{fmt}", fmt, s.data, 8 * s.hdr_len, PC.EDGE_CHUNK, EDGE_SLABS))
    return out


@lru_cache(maxsize=None)
def serial_inputs():
    """[(name, data, chunk_bytes, slabs)], raw deflate of alice29.txt and a built stream: the finder names no start in any slab"""
    content = IC.file_content("alice")
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 2, zlib.Z_FIXED)
    fixed = co.compress(content) + co.flush()
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    stored = co.compress(content) + co.flush()
    return [("fixed", fixed, content, 512, (4096, 8192)), ("stored", stored, content, 512, (70000,)),
            ("chunk-edges", PC.chunk_edges(512)[0].data, PC.chunk_edges(512)[0].content, 512, (2048,))]


@lru_cache(maxsize=None)
def alice_gzip_fields():
    """alice29.txt, small blocks, behind a gzip header with FEXTRA and FNAME -> (data, first_bit)"""
    content = IC.file_content("alice")
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 2)
    return IC.GZIP_FIELDS + co.compress(content) + co.flush() + W.gzip_trailer(content), 8 * len(IC.GZIP_FIELDS)


@lru_cache(maxsize=None)
def salted(copies=110):
    """about 16 MiB: alice29.txt repeated with a per-copy salt, zlib level 6 -> (data, content)"""
    alice = IC.file_content("alice")
    content = b"".join(b"%08d" % i + alice for i in range(copies))
    return zlib.compress(content, 6), content
