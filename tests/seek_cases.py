"""The seek tables of the tests of chip_zstd_seek_plan[_host] / chip_zstd_seek_table_write[_host]: built tables of every size at
every tail length the walk distinguishes, sums that cross 2^32, one case per line of the walk, and files of hand-built frames.
A case is (name, tail, file_len): the last len(tail) bytes of a file of file_len bytes -- the frames in front are never looked at
by the plan, so the synthetic cases carry none."""
import collections
import functools
import struct

import numpy as np

import seek_ref as R

Case = collections.namedtuple("Case", "name tail file_len")
NS = (0, 1, 2, 255, 256, 257, 1025, 70000)


@functools.lru_cache(maxsize=None)
def entries(n, seed=1):
    """(c_len, d_len, checksum) of n entries: small sizes, some of them 0, every bit of the checksum in use"""
    rng = np.random.default_rng(1000 * seed + n)
    c = rng.integers(9, 5000, n, dtype=np.uint32)
    d = rng.integers(0, 70000, n, dtype=np.uint32)
    d[rng.integers(0, 4, n) == 0] = 0
    x = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    return c, d, x


def built(n, cs, extra=0, cut=0, name=None):
    """the table of entries(n) behind `extra` bytes of the frames' area, its first `cut` bytes not in the tail"""
    c, d, x = entries(n)
    t = R.table(c.tolist(), d.tolist(), x.tolist() if cs else None)
    tail = (bytes((7 * i + 1) & 0xFF for i in range(extra)) + t)[cut:]
    return Case(name or f"n{n}_cs{int(cs)}_extra{extra}_cut{cut}", tail, len(t) + max(int(c.sum()), extra))


def _with(t, at, fmt, v):
    b = bytearray(t)
    struct.pack_into(fmt, b, at if at >= 0 else len(b) + at, v)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def tables():
    """every case of the plan tests"""
    out = []
    for n in NS:
        for cs in (False, True):
            T = 17 + (12 if cs else 8) * n
            out.append(built(n, cs))  # tail_len == T
            out += [built(n, cs, extra=k) for k in ((1, 2, 3, 4, 5, 6, 7) if n in (0, 2, 257) else (3,))]
            out.append(built(n, cs, extra=5000 if n else 40, name=f"n{n}_cs{int(cs)}_whole"))  # (with its frames' area in front)
            if n:
                out += [built(n, cs, cut=c, name=f"n{n}_cs{int(cs)}_need{T - c}") for c in (1, T - 17, T - 16)]  # tail_len T - 1, 17, 16
                out.append(Case(f"n{n}_cs{int(cs)}_need0", b"", built(n, cs).file_len))
    # sums that cross 2^32: no frame data is needed for the plan
    big = [0xFFFFFFF0] * 3
    out.append(Case("c_sum_crosses", R.table(big, [1, 2, 3], [7, 8, 9]), 3 * 0xFFFFFFF0 + 53))
    out.append(Case("d_sum_crosses", R.table([10, 20, 30, 40], [0xFFFFFFF0, 0xFFFFFFFE, 0, 0xFFFFFFF0]), 100 + 49))
    # one case per line of the walk
    c, d, x = (a.tolist() for a in entries(5))
    good, good_cs = R.table(c, d), R.table(c, d, x)
    C = sum(c)
    out.append(Case("short_file", good[-16:], 16))
    out.append(Case("footer_magic", _with(good, -4, "<I", 0x8F92EAB0), C + len(good)))
    for bit in (0x04, 0x08, 0x10, 0x20, 0x40):
        out.append(Case(f"reserved_{bit:02x}", _with(good, -5, "<B", bit), C + len(good)))
        out.append(Case(f"reserved_cs_{bit:02x}", _with(good_cs, -5, "<B", 0x80 | bit), C + len(good_cs)))
    out.append(Case("low_bits", R.table(c, d, desc_low=3), C + len(good)))  # still OK
    out.append(Case("low_bits_cs", R.table(c, d, x, desc_low=1), C + len(good_cs)))
    out.append(Case("n_over_limit", _with(good, -9, "<I", 0x8000001), 1 << 40))
    out.append(Case("n_at_limit_need_tail", _with(good, -9, "<I", 0x8000000), 1 << 40))  # T <= file_len: NEED_TAIL with T
    out.append(Case("table_over_file", _with(good, -9, "<I", 6), len(good)))  # T = 65 > 57
    for m in (0x184D2A5D, 0x184D2A5F, 0xFD2FB528):
        out.append(Case(f"skip_magic_{m:08x}", _with(good, 0, "<I", m), C + len(good)))
        out.append(Case(f"skip_magic_cs_{m:08x}", _with(good_cs, 0, "<I", m), C + len(good_cs)))
    for delta in (-1, 1):
        out.append(Case(f"size_field_{delta:+d}", _with(good, 4, "<I", len(good) - 8 + delta), C + len(good)))
    for name, at in (("first", [0]), ("middle", [2]), ("last", [4]), ("two", [3, 1])):
        dd = list(d)
        for k in at:
            dd[k] = 0xFFFFFFFF
        out.append(Case(f"unsized_{name}", R.table(c, dd, x), C + len(good_cs)))
    out.append(Case("layout_over_by_1", good, C + len(good) - 1))
    out.append(Case("layout_foreign_in_front", good, C + len(good) + 5))
    assert len({k.name for k in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(k for k in tables() if k.name == name)


def raw_frames_file(n=20, size=300, checksums=True, seed=3):
    """a file of n hand-built raw-block frames WITHOUT content checksum and a (checksummed) table: (file, contents, frames)"""
    import zstd_plan_cases as Z

    contents = [Z.text(size + 7 * k, seed + k) for k in range(n)]
    frames = [Z.raw_frame(c) for c in contents]
    t = R.table([len(f) for f in frames], [len(c) for c in contents], [R.xxh64(c) & 0xFFFFFFFF for c in contents] if checksums else None)
    return b"".join(frames) + t, contents, frames


XXH_LENGTHS = (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 95, 96, 127, 4095, 4096, 4097, 8191, 8192, 8193, 12288 + 31, 100003)
