"""The checkpoint index without a GPU: the built streams are what they claim (the system zlib decodes them, their boundaries visit
every bit phase, every chunk between two points decodes under zlib from its bit with its window as the dictionary); the damaged
inputs of the GPU tests leave their neighbours clean; chip_inflate_index_units_host against the restatement in inflate_index_ref.py
on hand-made point lists; every layout verdict with its bad_index; the argument refusals of the three entry points, which need no
device.  Without the feature the library tests fail at the missing symbols."""
import ctypes as C
import zlib

import numpy as np
import pytest

import inflate_index_cases as IC
import inflate_index_ref as R

INVALID = -101
FMT_AUTO, FMT_ZSTD, FMT_BROTLI = 47, 100, 101
FAKE = 0x10000  # a pointer that is only looked at: the refusals come before the device and before any access


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_built_streams_are_valid_and_cover_the_phases(fmt):
    for s in (IC.phases(fmt), IC.phases(fmt, False), IC.edges(fmt), IC.damage(fmt)):
        assert zlib.decompress(s.data, R.FMT[fmt]) == s.content
    s = IC.phases(fmt)
    assert s.hdr_len == {"raw": 0, "zlib": 2, "gzip": 27}[fmt]
    b = R.boundaries(s)
    pts = R.points(s, R.WRAP[fmt], 1)
    assert {bit & 7 for bit, _, _ in pts} == set(range(8))
    assert len(pts) < len(b), "empty blocks: boundaries that are no points"
    kind = {blk[0]: blk[1] for blk in s.blocks}
    assert any(kind[bit] == 0 and bit & 7 for bit, _, _ in pts), "a point whose block is stored and starts at an odd bit"
    stored_ends = {r.bit + r.nbits for r in s.layout if r.kind == "stored"}
    assert any(bit in stored_ends for bit, _, _ in pts), "a point directly behind a stored block"
    assert len(R.points(s, R.WRAP[fmt], 500)) in range(4, 8)
    e = R.points(IC.edges(fmt), R.WRAP[fmt], 1)
    assert [o for _, o, _ in e][:4] == [0, 1000, 1153, 32768]
    first = {r.block: r for r in reversed(IC.edges(fmt).layout) if r.kind in ("lit", "match")}
    assert (first[1].dist, first[3].dist, first[3].length, first[6].dist, first[6].length) == (1000, 32768, 258, 100, 258)


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
@pytest.mark.parametrize("spacing", [1, 500, 0])
def test_every_chunk_is_an_independent_unit_under_zlib(fmt, spacing):
    for s in (IC.phases(fmt), IC.edges(fmt), IC.damage(fmt)):
        pts = R.points(s, R.WRAP[fmt], spacing)
        ends = [o for _, o, _ in pts[1:]] + [len(s.content)]
        end_bits = [b for b, _, _ in pts[1:]] + [None]
        for (bit, o, _), end, end_bit in zip(pts, ends, end_bits):
            assert R.zlib_chunk(s.data, bit, R.window(s.content, o), end - o, end_bit) == s.content[o:end]


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_damaged_inputs_leave_their_neighbours_clean(fmt):
    s = IC.damage(fmt)
    pts = R.points(s, R.WRAP[fmt], 1)
    data, at = IC.flipped_stored_byte(s, IC.DAMAGE_BLOCK)
    ends = [o for _, o, _ in pts[1:]] + [len(s.content)]
    changed = []
    end_bits = [b for b, _, _ in pts[1:]] + [None]
    for k, ((bit, o, _), end, end_bit) in enumerate(zip(pts, ends, end_bits)):
        got = R.zlib_chunk(data, bit, R.window(s.content, o), end - o, end_bit)
        assert got is not None and len(got) == end - o, "every chunk still decodes to its end"
        if got != s.content[o:end]:
            changed.append(k)
    assert changed == [IC.DAMAGE_BLOCK] and pts[IC.DAMAGE_BLOCK][1] <= at < ends[IC.DAMAGE_BLOCK]


def units_host(fmt, length, pts, total_out):
    import compu_amd

    return compu_amd.inflate_index_units_host(R.FMT[fmt], length, [p[0] for p in pts], [p[1] for p in pts], [p[2] for p in pts], total_out)


HAND = [
    # every pt_bit & 7, a byte-aligned point (one byte early), a raw stream's point 0 at bit 0, wl below, at and above 32 768
    ("raw", 100000, [(0, 0, 0), (81, 100, 0), (162, 32767, 0), (243, 32768, 0), (324, 32769, 0), (405, 70000, 0), (486, 70001, 0),
                     (567, 1 << 20, 0), (640, 1 << 21, 0), (648, (1 << 32) - 17, 0)], (1 << 32) - 16),
    ("zlib", 5000, [(16, 0, 1), (24, 5, 0x12345678), (8 * 4999 + 7, 40000, 0xFFFFFFFF)], 40000),
    ("gzip", 1 << 20, [(80, 0, 0), (83, 0, 0), (1000, 32768, 5), (8 * (1 << 20) - 1, 3 << 30, 9)], (3 << 30) + 7),
    ("gzip", 77, [], 0),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_units_host_equals_the_restatement(case):
    fmt, length, pts, total = HAND[case]
    want = R.units(R.WRAP[fmt], length, [p[0] for p in pts], [p[1] for p in pts], [p[2] for p in pts], total)
    in_off, in_len, out_cap, win_len, resume, status, bad = units_host(fmt, length, pts, total)
    assert (int(status), bad) == want[:2] == (R.READ_OK, 0)
    got = [(int(a), int(b), int(c), int(d), [int(x) for x in r]) for a, b, c, d, r in zip(in_off, in_len, out_cap, win_len, resume)]
    assert got == want[2] and len(got) == len(pts)
    for (bit, o, chk), row in zip(pts, got):
        assert row[4][0] != 0 or bit == 0, "word 0 is 0 only at the stream's start"
        assert 8 * row[0] + row[4][0] == bit and row[3] == min(32768, o)


BAD_LAYOUTS = [
    ("pt_out[0] != 0", 1000, [(16, 1, 0), (90, 50, 0)], 100, 0),
    ("pt_out decreases", 1000, [(16, 0, 0), (90, 50, 0), (190, 49, 0), (300, 80, 0)], 100, 1),
    ("pt_out behind total_out", 1000, [(16, 0, 0), (90, 50, 0), (190, 101, 0)], 100, 2),
    ("pt_bit equal", 1000, [(16, 0, 0), (90, 50, 0), (90, 60, 0)], 100, 1),
    ("pt_bit decreases", 1000, [(16, 0, 0), (90, 50, 0), (190, 60, 0), (189, 70, 0)], 100, 2),
    ("pt_bit at 8 * len", 1000, [(16, 0, 0), (8000, 50, 0)], 100, 1),
    ("content above 2^32 - 16 - 32768", 1000, [(16, 0, 0), (90, 50, 0)], 50 + R.CAP_MAX + 1, 1),
    ("input above CHIP_GZPLAN_WINDOW", 2 * R.GZPLAN_WINDOW, [(16, 0, 0), (8 * (R.GZPLAN_WINDOW + 2) + 1, 50, 0), (8 * (R.GZPLAN_WINDOW + 9), 60, 0)], 100, 0),
]


@pytest.mark.parametrize("case", range(len(BAD_LAYOUTS)))
def test_layout_verdicts(case):
    what, length, pts, total, bad_index = BAD_LAYOUTS[case]
    want = R.units(2, length, [p[0] for p in pts], [p[1] for p in pts], [p[2] for p in pts], total)
    assert want == (R.READ_BAD_LAYOUT, bad_index, []), what
    *arrays, status, bad = units_host("gzip", length, pts, total)
    assert (int(status), bad) == (R.READ_BAD_LAYOUT, bad_index), what
    assert all(a.size == 0 for a in arrays)
    # the limits themselves pass
    if "2^32" in what:
        assert int(units_host("gzip", length, pts, total - 1)[5]) == R.READ_OK
    if "GZPLAN" in what:
        ok = [pts[0], (8 * R.GZPLAN_WINDOW + 8, 50, 0)]
        assert int(units_host("gzip", length, ok, total)[5]) == R.READ_OK


def test_refusals_need_no_device():
    import compu_amd
    from compu_amd.api import _InflateIndexSummary, _ReadSummary

    lib = compu_amd.lib()
    s, rs = _InflateIndexSummary(), _ReadSummary()
    build = lambda fmt=31, in_base=FAKE, length=100, out=FAKE, cap=100, max_points=0, arrays=(None,) * 4, summ=C.byref(s): \
        lib.chip_inflate_index_build(fmt, in_base, length, out, cap, 0, max_points, *arrays, summ, None)  # noqa: E731
    assert build(summ=None) == INVALID
    assert build(in_base=FAKE + 1) == INVALID and build(in_base=FAKE + 2) == INVALID
    assert build(in_base=None) == INVALID and build(out=None) == INVALID
    assert build(length=R.GZPLAN_WINDOW + 1) == INVALID
    assert build(cap=(1 << 32) - 15) == INVALID
    for fmt in (FMT_ZSTD, FMT_BROTLI, 0, 131):
        assert build(fmt=fmt) == INVALID
    for hole in range(4):
        arrays = [FAKE] * 4
        arrays[hole] = None
        assert build(max_points=1, arrays=tuple(arrays)) == INVALID

    read = lambda fmt=31, in_base=FAKE, n_points=1, arrays=(FAKE,) * 4, n_ranges=0, ranges=(None, None), dst=None, dst_cap=0, summ=C.byref(rs): \
        lib.chip_inflate_index_read(fmt, in_base, 100, n_points, *arrays, 100, n_ranges, *ranges, dst, dst_cap, None, None, summ, None)  # noqa: E731
    rs.n_units = rs.out_len = rs.status = 7
    assert read() == 0, "n_ranges == 0 is CHIP_OK"
    assert bytes(rs) == bytes(C.sizeof(rs)), "with an all-zero summary"
    assert read(summ=None) == INVALID
    assert read(in_base=FAKE + 1) == INVALID and read(in_base=None) == INVALID
    for fmt in (FMT_AUTO, FMT_ZSTD, FMT_BROTLI, 0):
        assert read(fmt=fmt) == INVALID
    for hole in range(4):
        arrays = [FAKE] * 4
        arrays[hole] = None
        assert read(arrays=tuple(arrays)) == INVALID
    assert read(n_ranges=1) == INVALID and read(n_ranges=1, ranges=(FAKE, None)) == INVALID
    assert read(dst_cap=1) == INVALID
    assert read(n_points=1 << 32) == INVALID

    st, bad = C.c_int32(0), C.c_uint64(0)
    one = np.zeros(1, np.uint64)
    p = one.ctypes.data_as(C.c_void_p)
    host = lambda fmt=31, n=1, arrays=(p, p, p), st_=C.byref(st), bad_=C.byref(bad): \
        lib.chip_inflate_index_units_host(fmt, 100, n, *arrays, 0, None, None, None, None, None, st_, bad_)  # noqa: E731
    assert host() == 0
    assert host(fmt=FMT_AUTO) == INVALID and host(st_=None) == INVALID and host(bad_=None) == INVALID
    assert host(arrays=(p, None, p)) == INVALID and host(n=1 << 32) == INVALID
    assert host(n=0, arrays=(None, None, None)) == 0


def test_python_faces_are_exported():
    import compu_amd

    for name in ("inflate_index_build", "inflate_index_read", "inflate_index_units_host", "gzip_index_decode", "gzip_index_read", "InflateIndex",
                 "InflateIndexSummary"):
        assert hasattr(compu_amd, name), name
