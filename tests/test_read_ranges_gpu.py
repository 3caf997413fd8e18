"""Reading ranges on the GPU: chip_select_units equals chip_select_units_host equals the plain-Python definition (select_ref.py)
on the plans of a BGZF file of 2 378 blocks and of a seekable zstd file of 153 frames; chip_read_ranges lands alice[lo:lo + len]
end to end, decodes only the units the ranges touch, writes nothing outside dst[0 .. out_len), reports CHIP_READ_NEED_OUTPUT and
CHIP_READ_BAD_LAYOUT without writing, names a damaged block and the ranges it spoils, never decodes a damaged block no range
touches, and serves two host threads on one stream.  Without the feature every test here fails at the missing symbols."""
import random
import threading

import numpy as np
import pytest

import select_ref as R

pytestmark = pytest.mark.gpu

FMT_GZIP, FMT_ZSTD, FMT_BGZF, W_SEEK_TABLE = 31, 100, 131, 1
POISON, GUARD = 0xEE, 64


def upload(torch, data):
    """`data` in a 16-byte aligned device tensor padded to a multiple of 4 (and never empty)"""
    t = torch.full(((len(data) + 3) // 4 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


class Plan:
    """A file on the device, its plan as device tensors and as lists"""

    def __init__(self, torch, fmt, buf, length, rows):
        self.fmt, self.buf, self.length = fmt, buf, length
        self.dev = rows  # in_off, in_len, out_off, out_cap
        self.host = [t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint32).tolist() for t in rows]


PLANS = {}


def plan_of(torch, alice, kind):
    import compu_amd

    if kind not in PLANS:
        src = upload(torch, alice)
        if kind == "bgzf":
            out, summ = compu_amd.encode_file(FMT_BGZF, 1, src, len(alice), unit_bytes=64)
            buf = upload(torch, out.cpu().numpy().tobytes())
            *rows, ps = compu_amd.bgzf_plan(buf, summ.out_len)
            assert ps.n_blocks == 2377 + 1 and ps.eof == 1 and int(ps.status) == 0 and ps.total_out == len(alice)
            PLANS[kind] = Plan(torch, FMT_GZIP, buf, summ.out_len, rows)
        else:
            out, summ = compu_amd.encode_file(FMT_ZSTD, 3, src, len(alice), unit_bytes=1000, flags=W_SEEK_TABLE)
            buf = upload(torch, out.cpu().numpy().tobytes())
            *rows, ps = compu_amd.zstd_plan(buf, summ.out_len)
            assert (ps.n_frames, ps.n_skippable, ps.n_unsized, int(ps.status), ps.total_out) == (153, 1, 0, 0, len(alice))
            PLANS[kind] = Plan(torch, FMT_ZSTD, buf, summ.out_len, rows)
    return PLANS[kind]


def range_set(plan, name, alice):
    if name == "seeded":  # 3 000: the per-range scan crosses its 1 024-entry workgroup boundary twice
        return R.random_ranges(random.Random(1), 0, len(alice), 3000)
    return R.boundary_ranges(plan.host[2], plan.host[3])


def to_device(torch, ranges):
    from compu_amd.api import _ranges_to_device

    return _ranges_to_device(ranges, torch.device("cuda"))


def lists(torch, tensors):
    return [t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint32 if t.dtype == torch.int32 else np.uint8).tolist() for t in tensors]


def expected_bytes(alice, ranges, status):
    return b"".join(alice[lo:lo + ln] for (lo, ln), st in zip(ranges, status) if st == R.OK)


def read(torch, plan, ranges, mis=0, room=None, rows=None, buf=None):
    """chip_read_ranges into a poisoned tensor with guard bytes on each side; returns (before, dst, behind, dst_off, status, summary):
    the guard in front, the `room` bytes of destination, everything behind them"""
    import compu_amd

    lo, ln = to_device(torch, ranges)
    if room is None:
        room = sum(l for (_, l), st in zip(ranges, R.select(*plan.host, ranges).status) if st == R.OK)
    box = torch.full((GUARD + 16 + room + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert box.data_ptr() % 16 == 0
    dst = box[GUARD + mis:GUARD + mis + room]
    _, dst_off, status, summ = compu_amd.read_ranges(plan.fmt, buf if buf is not None else plan.buf, *(rows or plan.dev), lo, ln, dst=dst)
    torch.cuda.synchronize()
    raw = box.cpu().numpy().tobytes()
    return raw[:GUARD + mis], raw[GUARD + mis:GUARD + mis + room], raw[GUARD + mis + room:], dst_off, status, summ


def all_poison(b):
    return b == bytes([POISON]) * len(b)


@pytest.mark.parametrize("which", ["seeded", "boundary"])
@pytest.mark.parametrize("kind", ["bgzf", "zstd"])
def test_select_units_equals_host_equals_reference(gpu, alice, kind, which):
    import compu_amd

    plan = plan_of(gpu, alice, kind)
    ranges = range_set(plan, which, alice)
    want = R.select(*plan.host, ranges)
    assert want.n_outside > 0 and want.n_sel > 1
    lo, ln = to_device(gpu, ranges)
    *arrays, summ = compu_amd.select_units(*plan.dev, lo, ln)
    got = lists(gpu, arrays)
    np_lo, np_ln = np.array([r[0] for r in ranges], np.uint64), np.array([r[1] for r in ranges], np.uint32)
    *h_arrays, h_summ = compu_amd.select_units_host(*plan.host, np_lo, np_ln)
    assert summ.as_tuple() == h_summ.as_tuple() == want.summary()
    wants = [want.sel_unit, want.sel_in_off, want.sel_in_len, want.sel_out_off, want.sel_out_cap, want.src_off, want.dst_off, want.status]
    for name, g, h, w in zip(("sel_unit", "sel_in_off", "sel_in_len", "sel_out_off", "sel_out_cap", "src_off", "dst_off", "status"), got, h_arrays, wants):
        assert g == h.tolist() == w, name
    # a prefix, and nothing behind it
    k = want.n_sel // 2
    *arrays, summ = compu_amd.select_units(*plan.dev, lo, ln, max_sel=k)
    assert summ.as_tuple() == want.summary() and lists(gpu, arrays[:1])[0] == want.sel_unit[:k]


@pytest.mark.parametrize("mis", [0, 5])
@pytest.mark.parametrize("which", ["seeded", "boundary"])
@pytest.mark.parametrize("kind", ["bgzf", "zstd"])
def test_read_ranges(gpu, alice, kind, which, mis):
    plan = plan_of(gpu, alice, kind)
    ranges = range_set(plan, which, alice)
    want = R.select(*plan.host, ranges)
    before, dst, behind, dst_off, status, summ = read(gpu, plan, ranges, mis=mis)
    assert summ.as_tuple() == (want.n_sel, want.out_len, want.n_outside, 0, 0, 0, R.READ_OK, 0)
    assert lists(gpu, [dst_off, status]) == [want.dst_off, want.status]
    assert len(dst) == want.out_len and dst == expected_bytes(alice, ranges, want.status)
    assert all_poison(before) and all_poison(behind)
    # with room to spare nothing behind out_len is written either
    before, dst, behind, _, _, summ = read(gpu, plan, ranges, mis=mis, room=want.out_len + 100)
    assert summ.out_len == want.out_len and dst[:want.out_len] == expected_bytes(alice, ranges, want.status)
    assert all_poison(before) and all_poison(dst[want.out_len:]) and all_poison(behind)


@pytest.mark.parametrize("kind", ["bgzf", "zstd"])
def test_whole_content_one_byte_and_one_block(gpu, alice, kind):
    import compu_amd

    plan = plan_of(gpu, alice, kind)
    whole = compu_amd.bgzf_decode(plan.buf, plan.length) if kind == "bgzf" else compu_amd.zstd_frames_decode(plan.buf, plan.length)[0]
    _, dst, _, _, status, summ = read(gpu, plan, [(0, len(alice))])
    assert dst == whole.cpu().numpy().tobytes() == alice and summ.n_units == sum(1 for c in plan.host[3] if c)
    # one byte: one unit
    _, dst, _, _, _, summ = read(gpu, plan, [(77777, 1)])
    assert dst == alice[77777:77778] and summ.n_units == 1
    # 3 000 one-byte ranges inside a single unit: it is decoded once
    u = len(plan.host[2]) // 2
    rng = random.Random(5)
    ranges = [(plan.host[2][u] + rng.randrange(plan.host[3][u]), 1) for _ in range(3000)]
    _, dst, _, dst_off, _, summ = read(gpu, plan, ranges)
    assert summ.n_units == 1 and summ.out_len == 3000 and dst == bytes(alice[lo] for lo, _ in ranges)
    assert lists(gpu, [dst_off])[0] == list(range(3000))


@pytest.mark.parametrize("kind", ["bgzf", "zstd"])
def test_need_output_and_nothing_to_read(gpu, alice, kind):
    import compu_amd

    plan = plan_of(gpu, alice, kind)
    ranges = range_set(plan, "boundary", alice)
    want = R.select(*plan.host, ranges)
    for mis in (0, 5):
        before, dst, behind, dst_off, status, summ = read(gpu, plan, ranges, mis=mis, room=want.out_len - 1)
        assert summ.as_tuple() == (0, want.out_len, want.n_outside, 0, 0, 0, R.READ_NEED_OUTPUT, 0)
        assert all_poison(before) and all_poison(dst) and all_poison(behind)
    # no ranges; ranges that are all empty or all outside: no unit is decoded, nothing is written
    lo, ln = to_device(gpu, [(0, 1)])
    out, _, _, summ = compu_amd.read_ranges(plan.fmt, plan.buf, *plan.dev, lo[:0], ln[:0])
    assert summ.as_tuple() == (0, 0, 0, 0, 0, 0, R.READ_OK, 0) and out.numel() == 0
    for ranges, outside in (([(0, 0), (100, 0), (len(alice), 0), (R.U64 - 1, 0)], 0), ([(len(alice), 1), (R.U64 - 1, 2)], 2)):
        before, dst, behind, dst_off, status, summ = read(gpu, plan, ranges, room=32)
        assert summ.as_tuple() == (0, 0, outside, 0, 0, 0, R.READ_OK, 0)
        assert all_poison(before) and all_poison(dst) and all_poison(behind)
        assert lists(gpu, [dst_off, status]) == [[0] * len(ranges), [R.OUTSIDE if outside else R.OK] * len(ranges)]


def test_damaged_block(gpu, alice):
    """One byte of the CRC-32 of BGZF block 1 200 flipped, on a copy of the file: the decoder answers -3 for that block."""
    plan = plan_of(gpu, alice, "bgzf")
    in_off, in_len, out_off, out_cap = plan.host
    bad = 1200
    buf = plan.buf.clone()
    buf[in_off[bad] + in_len[bad] - 8] ^= 0x40
    lo_b, hi_b = out_off[bad], out_off[bad] + out_cap[bad]
    ranges = R.random_ranges(random.Random(2), 0, len(alice), 3000, stray=0.0)
    ranges += [(lo_b, 1), (hi_b - 1, 1), (lo_b - 1, 2), (hi_b - 1, 2), (lo_b - 10, 200), (0, len(alice)), (lo_b - 1, 1), (hi_b, 1)]
    want = R.select(*plan.host, ranges)
    touch = [f is not None and f <= bad <= l for f, l in zip(want.first, want.last)]
    assert 6 <= sum(touch) < len(ranges) // 2
    before, dst, behind, dst_off, status, summ = read(gpu, plan, ranges, mis=5, buf=buf)
    assert summ.as_tuple() == (want.n_sel, want.out_len, 0, 1, bad, 0, R.READ_OK, -3)
    assert lists(gpu, [status])[0] == [R.BAD_UNIT if t else R.OK for t in touch]
    assert all_poison(before) and all_poison(behind) and lists(gpu, [dst_off])[0] == want.dst_off
    for (lo, ln), t, d in zip(ranges, touch, want.dst_off):
        if not t:
            assert dst[d:d + ln] == alice[lo:lo + ln], (lo, ln)
    # ranges that all avoid the block: it is never decoded
    clean = [r for r, t in zip(ranges, touch) if not t]
    want = R.select(*plan.host, clean)
    assert bad not in want.sel_unit and bad - 1 in want.sel_unit and bad + 1 in want.sel_unit
    _, dst, _, _, status, summ = read(gpu, plan, clean, buf=buf)
    assert summ.as_tuple() == (want.n_sel, want.out_len, 0, 0, 0, 0, R.READ_OK, 0)
    assert dst == expected_bytes(alice, clean, want.status) and lists(gpu, [status])[0] == [R.OK] * len(clean)


def test_bad_layout_writes_nothing(gpu, alice):
    import compu_amd
    import zstd_plan_cases as Z

    plan = plan_of(gpu, alice, "bgzf")
    ranges = range_set(plan, "boundary", alice)
    lo, ln = to_device(gpu, ranges)
    for at, delta in ((1, 1), (1700, -1), (len(plan.host[2]) - 1, 1)):
        out_off = plan.dev[2].clone()
        out_off[at] += delta
        rows = [plan.dev[0], plan.dev[1], out_off, plan.dev[3]]
        before, dst, behind, dst_off, status, summ = read(gpu, plan, ranges, room=1000, rows=rows)
        assert summ.as_tuple() == (0, 0, 0, 0, 0, at, R.READ_BAD_LAYOUT, 0)
        assert all_poison(before) and all_poison(dst) and all_poison(behind)
        assert not dst_off.any() and not status.any()  # (as allocated: zeros)
        *arrays, ss = compu_amd.select_units(*rows, lo, ln, max_sel=4)
        assert ss.as_tuple() == (0, 0, 0, 0, at, R.READ_BAD_LAYOUT) and all(a.numel() == 0 for a in arrays)
    # one frame that does not state its size: the plan's out_cap is CHIP_ZPLAN_UNSIZED, which is no layout to read from
    frame = Z.unsized_frame(alice[:5000])
    buf = upload(gpu, frame)
    *rows, ps = compu_amd.zstd_plan(buf, len(frame))
    assert (ps.n_frames, ps.n_unsized, int(ps.status)) == (1, 1, 0)
    out, dst_off, status, summ = compu_amd.read_ranges(FMT_ZSTD, buf, *rows, *to_device(gpu, [(0, 10), (100, 1)]),
                                                       dst=gpu.full((64,), POISON, dtype=gpu.uint8, device="cuda"))
    assert out is None and summ.as_tuple() == (0, 0, 0, 0, 0, 1, R.READ_BAD_LAYOUT, 0)
    with pytest.raises(ValueError):
        compu_amd.zstd_frames_read(buf, len(frame), [(0, 10)])


def test_two_host_threads_on_one_stream_then_trim(gpu, alice):
    """The slot is locked from its lookup to the wait behind the last launch: two threads with range sets of different sizes on
    the same stream get their own bytes every time; chip_trim() releases the slot and the next call allocates again."""
    import compu_amd

    jobs = [("bgzf", R.random_ranges(random.Random(11), 0, len(alice), 2500, stray=0.0)), ("zstd", [(1000, 50000), (3, 7)])]
    plans = [plan_of(gpu, alice, kind) for kind, _ in jobs]
    wants = [expected_bytes(alice, ranges, [R.OK] * len(ranges)) for _, ranges in jobs]
    devs = [to_device(gpu, ranges) for _, ranges in jobs]
    gpu.cuda.synchronize()
    stream = gpu.cuda.current_stream()
    errors = []

    def work(k):
        try:
            with gpu.cuda.stream(stream):
                for _ in range(10):
                    out, _, _, summ = compu_amd.read_ranges(plans[k].fmt, plans[k].buf, *plans[k].dev, *devs[k])
                    assert summ.n_bad == 0 and out.cpu().numpy().tobytes() == wants[k]
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    compu_amd.trim()  # the reader's slot is released with the others
    for k in range(2):
        out, _, _, summ = compu_amd.read_ranges(plans[k].fmt, plans[k].buf, *plans[k].dev, *devs[k])
        assert out.cpu().numpy().tobytes() == wants[k]


def test_conveniences(gpu, alice):
    import compu_amd

    ranges = [(152088, 1), (0, 100), (64, 64), (70000, 3000), (5, 0)]
    want = b"".join(alice[lo:lo + ln] for lo, ln in ranges)
    for kind, fn in (("bgzf", compu_amd.bgzf_read), ("zstd", compu_amd.zstd_frames_read)):
        plan = plan_of(gpu, alice, kind)
        out, dst_off = fn(plan.buf, plan.length, ranges)
        assert out.cpu().numpy().tobytes() == want and dst_off.tolist() == [0, 1, 101, 165, 3165]
        with pytest.raises(ValueError):
            fn(plan.buf, plan.length, [(0, 10), (len(alice), 1)])
