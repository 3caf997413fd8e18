"""chip_select_units_host against the plain-Python definition (select_ref.py): every array and the summary, on a hand-made layout
with empty units, on the boundary ranges, and on 200 seeded random layouts; broken layouts, max_sel, count-then-fill, and the
argument checks of all three entry points, which need no device.  Without the feature every test here fails at the missing symbol."""
import ctypes as C
import random

import numpy as np
import pytest

import select_ref as R

E_INVALID = -101
POISON32, POISON64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE


def host(layout, ranges, max_sel=None):
    import compu_amd

    lo = np.array([r[0] for r in ranges], dtype=np.uint64)
    ln = np.array([r[1] for r in ranges], dtype=np.uint32)
    return compu_amd.select_units_host(*[np.array(a, dtype=dt) for a, dt in zip(layout, (np.uint64, np.uint32, np.uint64, np.uint32))], lo, ln,
                                       max_sel=max_sel)


def check(layout, ranges, what=""):
    want = R.select(*layout, ranges)
    sel_unit, sel_in_off, sel_in_len, sel_out_off, sel_out_cap, src_off, dst_off, status, summ = host(layout, ranges)
    assert summ.as_tuple() == want.summary(), what
    assert sel_unit.tolist() == want.sel_unit and sel_in_off.tolist() == want.sel_in_off and sel_in_len.tolist() == want.sel_in_len, what
    assert sel_out_off.tolist() == want.sel_out_off and sel_out_cap.tolist() == want.sel_out_cap, what
    assert src_off.tolist() == want.src_off and dst_off.tolist() == want.dst_off and status.tolist() == want.status, what
    return want


# empty units at the start, in the middle, doubled, and at the end
HAND_CAPS = [0, 0, 10, 7, 0, 64, 1, 0, 0, 300, 5, 0]


@pytest.mark.parametrize("begin", [0, 1000], ids=["from0", "from1000"])
def test_hand_made_layout(begin):
    layout = R.layout(HAND_CAPS, begin=begin)
    ranges = R.boundary_ranges(layout[2], layout[3])
    want = check(layout, ranges)
    st = dict(zip(ranges, want.status))
    end = begin + sum(HAND_CAPS)
    assert st[(end, 0)] == R.OK and st[(end, 1)] == R.OUTSIDE and st[(R.U64 - 1, 2)] == R.OUTSIDE
    if begin:
        assert st[(begin - 1, 1)] == R.OUTSIDE and st[(0, 1)] == R.OUTSIDE
    # every range on its own, so that a mistake cannot hide behind another range's selection
    for r in ranges:
        check(layout, [r], r)
    # a range that starts where empty units sit starts in the unit that holds the byte; the empty ones are never selected
    one = R.select(*layout, [(begin + 17, 1)])
    assert one.sel_unit == [5] and one.src_off == [0]
    whole = R.select(*layout, [(begin, end - begin)])
    assert whole.sel_unit == [2, 3, 5, 6, 9, 10] and whole.scratch_bytes == end - begin


def test_no_units_and_no_ranges():
    check(([], [], [], []), [(0, 0), (0, 1), (5, 0)])
    sel = host(R.layout([5, 5]), [])
    assert sel[-1].as_tuple() == (0, 0, 0, 0, 0, R.READ_OK)
    check(R.layout([0, 0, 0]), [(0, 0), (0, 1)])  # units, but no content


def test_random_layouts():
    rng = random.Random(20240607)
    for case in range(200):
        n = rng.randrange(1, 3001) if case % 4 == 0 else rng.randrange(1, 200)
        top = rng.choice((1, 3, 300))
        caps = [rng.randrange(0, top + 1) if rng.random() < 0.8 else 0 for _ in range(n)]
        begin = rng.choice((0, 0, 12345, 1 << 40))
        layout = R.layout(caps, begin=begin, seed=case)
        m = rng.randrange(1, 3001) if case % 4 == 1 else rng.randrange(1, 100)
        ranges = R.random_ranges(rng, begin, begin + sum(caps), m)
        check(layout, ranges, case)


def test_large_layout_sizes_from_the_issue():
    """1..3 000 units with 1..3 000 ranges: the largest of both at once"""
    rng = random.Random(7)
    caps = [rng.randrange(0, 301) for _ in range(3000)]
    layout = R.layout(caps)
    check(layout, R.random_ranges(rng, 0, sum(caps), 3000))


def raw_call(layout, ranges, max_sel):
    """chip_select_units_host with poisoned output arrays of max(n, 4) / m entries; returns (rc, arrays, summary)"""
    import compu_amd
    from compu_amd.api import _SelectSummary

    arrs = [np.array(a, dtype=dt) for a, dt in zip(layout, (np.uint64, np.uint32, np.uint64, np.uint32))]
    lo = np.array([r[0] for r in ranges], dtype=np.uint64)
    ln = np.array([r[1] for r in ranges], dtype=np.uint32)
    n, m = len(layout[0]), len(ranges)
    k = max(n, 4)
    outs = [np.full(k, POISON32, np.uint32), np.full(k, POISON64, np.uint64), np.full(k, POISON32, np.uint32), np.full(k, POISON64, np.uint64),
            np.full(k, POISON32, np.uint32), np.full(m, POISON64, np.uint64), np.full(m, POISON64, np.uint64), np.full(m, 0x6E6E6E6E, np.int32)]
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    raw = _SelectSummary()
    rc = compu_amd.lib().chip_select_units_host(n, *[p(a) for a in arrs], m, p(lo), p(ln), max_sel, *[p(a) for a in outs], C.byref(raw))
    return rc, outs, compu_amd.SelectSummary(raw)


def untouched(a, start=0):
    poison = 0x6E6E6E6E if a.dtype == np.int32 else (POISON32 if a.dtype == np.uint32 else POISON64)
    return bool((a[start:] == poison).all())


def test_bad_layout_writes_nothing():
    caps = [10, 20, 30, 40, 50]
    ranges = [(0, 5), (25, 100), (500, 1)]
    for at in (1, len(caps) - 1):  # a broken chain at index 1 and at the last index
        for delta in (1, -1):
            layout = R.layout(caps)
            layout[2][at] += delta
            rc, outs, summ = raw_call(layout, ranges, len(caps))
            assert rc == 0 and summ.as_tuple() == (0, 0, 0, 0, at, R.READ_BAD_LAYOUT), (at, delta)
            assert all(untouched(a) for a in outs)
            assert R.select(*layout, ranges).summary() == summ.as_tuple()
    # one frame without a size, as chip_zstd_plan leaves it (it adds nothing to the offsets): the link behind it fails
    for at in range(len(caps)):
        layout = R.layout([c if i != at else 0 for i, c in enumerate(caps)])
        layout[3][at] = R.UNSIZED
        rc, outs, summ = raw_call(layout, ranges, len(caps))
        assert rc == 0 and summ.as_tuple() == (0, 0, 0, 0, at + 1, R.READ_BAD_LAYOUT), at
        assert all(untouched(a) for a in outs)
        assert R.select(*layout, ranges).summary() == summ.as_tuple()
    # the lowest failing link wins
    layout = R.layout(caps)
    layout[2][2] += 1
    layout[2][4] += 1
    assert raw_call(layout, ranges, 0)[2].bad_index == 2
    # a chain that wraps 2^64 is no layout
    rc, outs, summ = raw_call(([0, 30], [30, 30], [R.U64 - 25, R.U64 - 15], [10, 20]), ranges, 2)
    assert rc == 0 and summ.status == R.READ_BAD_LAYOUT and summ.bad_index == 2 and all(untouched(a) for a in outs)


def test_max_sel_writes_a_prefix_and_count_then_fill():
    rng = random.Random(3)
    caps = [rng.randrange(0, 50) for _ in range(400)]
    layout = R.layout(caps)
    ranges = R.random_ranges(rng, 0, sum(caps), 60, max_len=200)
    want = R.select(*layout, ranges)
    assert want.n_sel > 20
    # count: null arrays
    import compu_amd
    from compu_amd.api import _SelectSummary

    arrs = [np.array(a, dtype=dt) for a, dt in zip(layout, (np.uint64, np.uint32, np.uint64, np.uint32))]
    lo = np.array([r[0] for r in ranges], dtype=np.uint64)
    ln = np.array([r[1] for r in ranges], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    raw = _SelectSummary()
    rc = compu_amd.lib().chip_select_units_host(len(caps), *[p(a) for a in arrs], len(ranges), p(lo), p(ln), 0, *([None] * 8), C.byref(raw))
    assert rc == 0 and compu_amd.SelectSummary(raw).as_tuple() == want.summary()
    # fill: exactly n_sel, and a prefix with nothing behind it
    for max_sel in (want.n_sel, 7, 1):
        rc, outs, summ = raw_call(layout, ranges, max_sel)
        assert rc == 0 and summ.as_tuple() == want.summary()
        for a, w in zip(outs[:5], (want.sel_unit, want.sel_in_off, want.sel_in_len, want.sel_out_off, want.sel_out_cap)):
            assert a[:max_sel].tolist() == w[:max_sel] and untouched(a, max_sel), max_sel
        assert outs[5].tolist() == want.src_off and outs[6].tolist() == want.dst_off and outs[7].tolist() == want.status


def test_invalid_arguments_need_no_device():
    """Every CHIP_E_INVALID case of the three entry points answers before the device is looked for (this test runs without one)."""
    import compu_amd
    from compu_amd.api import _ReadSummary, _SelectSummary

    L = compu_amd.lib()
    a64, a32 = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    q, d = a64.ctypes.data_as(C.c_void_p), a32.ctypes.data_as(C.c_void_p)  # stand-ins: a refused call looks at no array
    ss, rs = _SelectSummary(), _ReadSummary()
    big = (1 << 32)
    sel_ok = [1, q, d, q, d, 1, q, d, 1, d, q, d, q, d, q, q, d]
    for fn, tail in ((L.chip_select_units_host, [C.byref(ss)]), (L.chip_select_units, [C.byref(ss), None])):
        def bad(i, v, fn=fn, tail=tail):
            args = list(sel_ok)
            args[i] = v
            return fn(*args, *tail)

        assert fn(*sel_ok, None, *tail[1:]) == E_INVALID  # summary NULL
        for i in (1, 2, 3, 4, 6, 7):  # a plan or range array NULL with its count > 0
            assert bad(i, None) == E_INVALID, i
        for i in (9, 10, 11, 12, 13):  # a sel array NULL with max_sel > 0
            assert bad(i, None) == E_INVALID, i
        assert bad(0, big) == E_INVALID and bad(5, big) == E_INVALID
    # no ranges: CHIP_OK and an all-zero summary, host and device entry alike, without a device
    for fn, tail in ((L.chip_select_units_host, [C.byref(ss)]), (L.chip_select_units, [C.byref(ss), None])):
        ss.n_sel = ss.out_len = 77
        assert fn(1, q, d, q, d, 0, None, None, 0, *([None] * 8), *tail) == 0
        assert compu_amd.SelectSummary(ss).as_tuple() == (0, 0, 0, 0, 0, 0)

    read_ok = [31, 1, q, q, d, q, d, 1, q, d, q, 16, q, d, C.byref(rs), None]

    def bad_read(i, v):
        args = list(read_ok)
        args[i] = v
        return L.chip_read_ranges(*args)

    assert bad_read(14, None) == E_INVALID  # summary NULL
    for i in (2, 3, 4, 5, 6, 8, 9):  # in_base, a plan or range array NULL with its count > 0
        assert bad_read(i, None) == E_INVALID, i
    assert bad_read(10, None) == E_INVALID  # dst_base NULL with dst_cap > 0
    assert bad_read(1, big) == E_INVALID and bad_read(7, big) == E_INVALID
    for fmt in (12345, 131, 1, -1):  # formats chip_decode_batch refuses (131: CHIP_FMT_BGZF is an encoder format)
        assert bad_read(0, fmt) == E_INVALID, fmt
    assert bad_read(2, C.c_void_p(a64.ctypes.data + 1)) == E_INVALID  # in_base as chip_decode_batch wants it: 4-byte aligned
    rs.n_units = rs.out_len = 77
    args = list(read_ok)
    args[7], args[8], args[9] = 0, None, None
    assert L.chip_read_ranges(*args) == 0
    assert compu_amd.ReadSummary(rs).as_tuple() == (0, 0, 0, 0, 0, 0, 0, 0)
