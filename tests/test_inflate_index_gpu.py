"""The checkpoint index on the GPU.  chip_inflate_index_build: the points, checks and windows of built streams equal the values
derived from the writer's block records and the system zlib, at spacing 1 and at larger spacings, counted and truncated; the
build's decode answers equal chip_decode_batch's for the same unit and room, errors included.  chip_inflate_index_read: the window
edges of a chunk; whole files (alice29, 2.5 MiB of bench data; zlib levels 1, 6, 9; raw, zlib, gzip) through the index equal
zlib.decompress; ranges of every kind; damage behind the build names the chunk and spares the others; a truncated index reads
the whole content; too little room, a broken index layout and nothing to read write nothing; null dst_off / range_status change
no byte; a plan read over the same chunks as gzip members answers the same.  Truth is zlib and tests/deflate_writer.py.  Without the
feature every test fails at the missing symbols."""
import ctypes as C
import zlib

import numpy as np
import pytest

import inflate_index_cases as IC
import inflate_index_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD, WINDOW = 0xEE, 64, 32768
POISON64 = int.from_bytes(bytes([POISON]) * 8, "little")
FINISHED, NEED_INPUT, NEED_OUTPUT = 2, 0, 1
RANGE_OK, RANGE_OUTSIDE, RANGE_BAD_UNIT = 0, 1, 2
READ_OK, READ_NEED_OUTPUT, READ_BAD_LAYOUT = 0, 1, 2


def upload(torch, data):
    """`data` in a 16-byte aligned device tensor padded to a multiple of 4 (and never empty)"""
    t = torch.full(((len(data) + 3) // 4 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


def u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def build(torch, fmt, data, out_cap, spacing, max_points, room=None):
    """chip_inflate_index_build into poisoned arrays of `room` entries (default max_points) -> dict of everything it answered"""
    import compu_amd
    from compu_amd.api import _InflateIndexSummary

    room = max_points if room is None else room
    d_in = upload(torch, data)
    out = torch.full((out_cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    pt_bit = torch.full((room,), POISON, dtype=torch.uint8, device="cuda").repeat_interleave(8).view(torch.int64) if room else None
    pt_out = pt_bit.clone() if room else None
    pt_check = torch.full((room * 4,), POISON, dtype=torch.uint8, device="cuda").view(torch.int32) if room else None
    windows = torch.full((room * WINDOW,), POISON, dtype=torch.uint8, device="cuda") if room else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    raw = _InflateIndexSummary()
    rc = compu_amd.lib().chip_inflate_index_build(R.FMT[fmt], p(d_in), len(data), p(out), out_cap, spacing, max_points, p(pt_bit), p(pt_out),
                                                  p(pt_check), p(windows), C.byref(raw), None)
    assert rc == 0
    return dict(d_in=d_in, out=out, pt_bit=pt_bit, pt_out=pt_out, pt_check=pt_check, windows=windows,
                summ=compu_amd.InflateIndexSummary(raw))


def decode_one(torch, fmt, data, out_cap):
    """chip_decode_batch of the same unit into the same poisoned room -> (out tensor, out_len, in_used, status)"""
    import compu_amd

    out = torch.full((out_cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")  # noqa: E731
    out_len, in_used, status = compu_amd.decode_batch(R.FMT[fmt], upload(torch, data), i64(0), i32(len(data)), out, i64(0), i32(out_cap))
    torch.cuda.synchronize()
    return out, u32(out_len)[0], u32(in_used)[0], int(status[0])


def same_as_decode(torch, fmt, data, out_cap, b):
    out, out_len, in_used, status = decode_one(torch, fmt, data, out_cap)
    s = b["summ"]
    assert (s.out_len, s.in_used, s.status) == (out_len, in_used, status)
    assert torch.equal(b["out"], out), "the bytes written are chip_decode_batch's, and nothing behind the room"
    return status


def check_points(b, want, content, wrap, n_all=None):
    """the first len(want) entries equal `want` [(bit, out, check)], the windows hold the content in front of each point and
    their own poison behind it, and nothing is written behind the entries"""
    s = b["summ"]
    assert s.n_points == (len(want) if n_all is None else n_all) and s.wrap == wrap
    n = len(want)
    if b["pt_bit"] is None:
        return
    bits, outs, checks = u64(b["pt_bit"]), u64(b["pt_out"]), u32(b["pt_check"])
    assert list(zip(bits[:n], outs[:n], checks[:n])) == want
    assert all(v == POISON64 for v in bits[n:] + outs[n:]) and all(v == POISON64 & 0xFFFFFFFF for v in checks[n:])
    win = b["windows"].cpu().numpy()
    for k, (_, o, _) in enumerate(want):
        wl = min(WINDOW, o)
        slot = win[k * WINDOW:(k + 1) * WINDOW]
        assert slot[:wl].tobytes() == content[o - wl:o], k
        assert (slot[wl:] == POISON).all(), k
    assert (win[n * WINDOW:] == POISON).all()


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
@pytest.mark.parametrize("case", ["phases", "phases_empty_final", "edges"])
def test_exact_points_on_built_streams(gpu, case, fmt):
    s = IC.edges(fmt) if case == "edges" else IC.phases(fmt, case == "phases")
    wrap, cap = R.WRAP[fmt], len(s.content)
    for spacing in (1, 500):
        want = R.points(s, wrap, spacing)
        b = build(gpu, fmt, s.data, cap, spacing, len(want) + 3)
        assert same_as_decode(gpu, fmt, s.data, cap, b) == FINISHED
        assert b["out"][:cap].cpu().numpy().tobytes() == s.content
        check_points(b, want, s.content, wrap)
        summ = b["summ"]
        assert summ.check == R.check_of(wrap, s.content)
        eob = [r for r in s.layout if r.kind in ("eob", "stored")][-1]
        assert summ.end_bit == eob.bit + eob.nbits
    want = R.points(s, wrap, 1)
    counted = build(gpu, fmt, s.data, cap, 1, 0)
    check_points(counted, [], s.content, wrap, n_all=len(want))
    assert counted["summ"].as_tuple() == build(gpu, fmt, s.data, cap, 1, len(want))["summ"].as_tuple()
    cut = build(gpu, fmt, s.data, cap, 1, 3, room=6)
    check_points(cut, want[:3], s.content, wrap, n_all=len(want))
    if case == "edges":  # the default spacing: 1 MiB, one point
        check_points(build(gpu, fmt, s.data, cap, 0, 2), want[:1], s.content, wrap)


def test_auto_format_names_the_wrapper(gpu):
    import compu_amd

    for fmt in ("zlib", "gzip"):
        s = IC.damage(fmt)
        out = gpu.empty(len(s.content), dtype=gpu.uint8, device="cuda")
        index, summ = compu_amd.inflate_index_build(47, upload(gpu, s.data), len(s.data), out, spacing=1000)
        assert (summ.status, summ.wrap, index.fmt, summ.out_len) == (FINISHED, R.WRAP[fmt], R.FMT[fmt], len(s.content))
        assert u64(index.pt_bit) == [p[0] for p in R.points(s, R.WRAP[fmt], 1000)]


def block_of(s, kind_pred):
    return next(r.block for r in s.layout if kind_pred(r))


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_the_build_is_the_decode_when_it_stops(gpu, fmt):
    import deflate_writer as W

    s = IC.damage(fmt)
    wrap, n = R.WRAP[fmt], len(s.content)
    full = R.points(s, wrap, 1)
    # the room one byte short: every boundary was reached
    b = build(gpu, fmt, s.data, n - 1, 1, len(full) + 2)
    assert same_as_decode(gpu, fmt, s.data, n - 1, b) == NEED_OUTPUT
    check_points(b, full, s.content, wrap)
    assert (b["summ"].check, b["summ"].end_bit) == (0, 0)
    # cut in the middle of block 9: boundaries 0 .. 9 were reached
    mid = next(r for r in s.layout if r.block == 9 and r.kind in ("lit", "stored"))
    data = s.data[:(mid.bit + mid.nbits // 2) // 8 + 1]
    assert s.blocks[9][0] < 8 * len(data) < s.blocks[10][0] - 64
    b = build(gpu, fmt, data, n, 1, len(full))
    assert same_as_decode(gpu, fmt, data, n, b) == NEED_INPUT
    check_points(b, R.points(s, wrap, 1, n_blocks=10), s.content, wrap)
    # a distance too far back in the third block
    d = W.Deflate()
    d.fixed([65, 66, 67]).dynamic(list(b"hello hello")).fixed([68, ("m", 5, 30), 69], final=True)
    bad = W.wrap(d, fmt)
    b = build(gpu, fmt, bad.data, 100, 1, 8)
    assert same_as_decode(gpu, fmt, bad.data, 100, b) == -3
    check_points(b, R.points(bad, wrap, 1), bad.content, wrap)
    # a wrong check value in the trailer: -3, the points still listed
    if fmt != "raw":
        data = s.data[:-8] + bytes([s.data[-8] ^ 1]) + s.data[-7:] if fmt == "gzip" else s.data[:-1] + bytes([s.data[-1] ^ 1])
        b = build(gpu, fmt, data, n, 1, len(full))
        assert same_as_decode(gpu, fmt, data, n, b) == -3
        check_points(b, full, s.content, wrap)
        assert b["summ"].check == 0


def index_of(gpu, fmt, data, content_len, spacing, max_points=None):
    import compu_amd

    d_in = upload(gpu, data)
    out = gpu.empty(max(content_len, 4), dtype=gpu.uint8, device="cuda")
    index, summ = compu_amd.inflate_index_build(R.FMT[fmt], d_in, len(data), out, spacing=spacing, max_points=max_points)
    assert (summ.status, summ.out_len) == (FINISHED, content_len)
    return index, d_in, summ


def read(gpu, index, d_in, ranges, room=None):
    """inflate_index_read into a poisoned destination with guards -> (dst bytes, guard ok, dst_off, status, summary)"""
    import compu_amd
    from compu_amd.api import _ranges_to_device

    lo, ln = _ranges_to_device(ranges, gpu.device("cuda"))
    if room is None:
        room = sum(l for lo_, l in ranges if lo_ + l <= index.total_out)
    box = gpu.full((GUARD + room + GUARD,), POISON, dtype=gpu.uint8, device="cuda")
    dst = box[GUARD:GUARD + room]
    _, dst_off, status, summ = compu_amd.inflate_index_read(index, d_in, lo, ln, dst=dst)
    host = box.cpu().numpy()
    guards = (host[:GUARD] == POISON).all() and (host[GUARD + room:] == POISON).all()
    return host[GUARD:GUARD + room].tobytes(), guards, u64(dst_off), status.cpu().tolist(), summ


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_window_edges_in_the_read(gpu, fmt):
    import compu_amd

    s = IC.edges(fmt)
    index, d_in, _ = index_of(gpu, fmt, s.data, len(s.content), 1)
    assert u64(index.pt_out)[:4] == [0, 1000, 1153, 32768] and 56415 in u64(index.pt_out)
    assert compu_amd.gzip_index_decode(index, d_in).cpu().numpy().tobytes() == s.content
    # each chunk alone: its first token reads the window the index kept, not a neighbour's output
    outs = u64(index.pt_out) + [len(s.content)]
    for k in range(index.n_points):
        got, guards, _, status, summ = read(gpu, index, d_in, [(outs[k], outs[k + 1] - outs[k])])
        assert got == s.content[outs[k]:outs[k + 1]] and guards and status == [RANGE_OK]
        assert (summ.n_units, summ.n_bad, int(summ.status)) == (1, 0, READ_OK)


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_built_streams_through_the_index(gpu, fmt):
    import compu_amd

    for s in (IC.phases(fmt), IC.phases(fmt, False), IC.damage(fmt)):
        for spacing in (1, 500):
            index, d_in, _ = index_of(gpu, fmt, s.data, len(s.content), spacing)
            assert index.n_points == len(R.points(s, R.WRAP[fmt], spacing))
            assert compu_amd.gzip_index_decode(index, d_in).cpu().numpy().tobytes() == s.content


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("name", ["alice", "synth"])
def test_whole_content_through_the_index(gpu, name, level, fmt):
    import compu_amd

    content, data = IC.file_content(name), IC.compressed(name, level, fmt)
    for spacing in (16384, 65536, 0):
        index, d_in, summ = index_of(gpu, fmt, data, len(content), spacing)
        step = spacing or 1 << 20
        outs = u64(index.pt_out)
        assert summ.n_points == index.n_points and outs[0] == 0 and all(b - a >= step for a, b in zip(outs, outs[1:]))
        assert summ.check == R.check_of(R.WRAP[fmt], content)
        lo, ln = compu_amd.api._ranges_to_device([(0, len(content))], gpu.device("cuda"))
        out, _, status, rs = compu_amd.inflate_index_read(index, d_in, lo, ln)
        assert (int(rs.status), rs.n_bad, rs.n_units, rs.out_len) == (READ_OK, 0, index.n_points, len(content))
        assert out.cpu().numpy().tobytes() == content
    if name == "alice" and level == 6:
        assert index.n_points == 1, "152 089 bytes at the default spacing: one chunk"


def file_index(gpu, fmt="gzip", max_points=None):
    """the 2.5 MiB file at zlib level 6, a point every 64 KiB (zlib's blocks there are a few tens of KiB: some forty points)"""
    content, data = IC.file_content("synth"), IC.compressed("synth", 6, fmt)
    index, d_in, _ = index_of(gpu, fmt, data, len(content), 65536, max_points)
    return content, data, index, d_in


def chunks_touched(outs, total, ranges):
    ends = outs[1:] + [total]
    return {k for k, (a, b) in enumerate(zip(outs, ends)) for lo, ln in ranges if ln and lo + ln <= total and lo < b and lo + ln > a and b > a}


def test_ranges(gpu):
    content, _, index, d_in = file_index(gpu)
    total, outs = len(content), u64(index.pt_out)
    assert index.n_points >= 6
    ranges = [(outs[2] + 10, 100), (outs[2] + 50, 20), (outs[2] + 50, 20),  # inside one chunk, nested, repeated
              (outs[3] - 5, 10), (outs[3] - 100, outs[5] - outs[3] + 200),   # across two chunks, across four
              (outs[4], 0), (total, 0), (total - 1, 1),                       # zero lengths, the last byte
              (total - 1, 2), (outs[1], 1)]                                   # past the end; out of order
    got, guards, dst_off, status, summ = read(gpu, index, d_in, ranges)
    want_status = [RANGE_OUTSIDE if lo + ln > total else RANGE_OK for lo, ln in ranges]
    assert status == want_status and guards
    assert got == b"".join(content[lo:lo + ln] for (lo, ln), st in zip(ranges, want_status) if st == RANGE_OK)
    lens = [ln if st == RANGE_OK else 0 for (_, ln), st in zip(ranges, want_status)]
    assert dst_off == [sum(lens[:r]) for r in range(len(ranges))]
    touched = chunks_touched(outs, total, ranges)
    assert touched == {1, 2, 3, 4, 5, index.n_points - 1}
    assert (summ.n_units, summ.n_outside, summ.n_bad, summ.out_len, int(summ.status)) == (len(touched), 1, 0, sum(lens), READ_OK)
    # too little room: the exact size, no byte written, nothing decoded
    got, guards, dst_off2, status2, summ = read(gpu, index, d_in, ranges, room=sum(lens) - 1)
    assert (int(summ.status), summ.out_len, summ.n_units) == (READ_NEED_OUTPUT, sum(lens), 0)
    assert got == bytes([POISON]) * (sum(lens) - 1) and guards and dst_off2 == dst_off and status2 == want_status


@pytest.mark.parametrize("fmt", ["zlib", "gzip"])
def test_damage_after_the_build(gpu, fmt):
    s = IC.damage(fmt)
    total = len(s.content)
    index, _, _ = index_of(gpu, fmt, s.data, total, 1)
    outs = u64(index.pt_out) + [total]
    j, last = IC.DAMAGE_BLOCK, index.n_points - 1
    whole = [(outs[k], outs[k + 1] - outs[k]) for k in range(index.n_points)]
    # one content byte flipped in chunk j: its check chain breaks, the others keep their bytes
    data, at = IC.flipped_stored_byte(s, j)
    assert outs[j] <= at < outs[j + 1]
    got, guards, dst_off, status, summ = read(gpu, index, upload(gpu, data), whole + [(outs[j - 1], outs[j + 2] - outs[j - 1])])
    assert status == [RANGE_BAD_UNIT if k == j else RANGE_OK for k in range(index.n_points)] + [RANGE_BAD_UNIT] and guards
    assert (summ.n_bad, summ.first_bad, summ.n_units, int(summ.status)) == (1, j, index.n_points, READ_OK)
    assert summ.bad_status in (NEED_INPUT, NEED_OUTPUT), "the chunk decoded to its end: it is the check value that differs"
    for k in range(index.n_points):
        if k != j:
            assert got[dst_off[k]:dst_off[k] + whole[k][1]] == s.content[outs[k]:outs[k + 1]], k
    # ranges that do not touch chunk j never decode it
    got, _, _, status, summ = read(gpu, index, upload(gpu, data), whole[:j] + whole[j + 1:])
    assert set(status) == {RANGE_OK} and (summ.n_bad, summ.n_units) == (0, index.n_points - 1)
    # a wrong check value in the trailer: only the last chunk is bad
    data = s.data[:-8] + bytes([s.data[-8] ^ 1]) + s.data[-7:] if fmt == "gzip" else s.data[:-1] + bytes([s.data[-1] ^ 1])
    got, _, dst_off, status, summ = read(gpu, index, upload(gpu, data), whole)
    assert status == [RANGE_OK] * last + [RANGE_BAD_UNIT]
    assert (summ.n_bad, summ.first_bad, summ.bad_status) == (1, last, -3)
    assert got[:dst_off[last]] == s.content[:outs[last]]


def test_raw_deflate_has_no_check_chain(gpu):
    """raw deflate carries no check value: the flipped stored byte of test_damage_after_the_build decodes, as it does under zlib,
    and no chunk is called bad"""
    s = IC.damage("raw")
    index, _, _ = index_of(gpu, "raw", s.data, len(s.content), 1)
    data, at = IC.flipped_stored_byte(s, IC.DAMAGE_BLOCK)
    got, _, _, status, summ = read(gpu, index, upload(gpu, data), [(0, len(s.content))])
    assert summ.n_bad == 0 and got[:at] == s.content[:at] and got[at] == s.content[at] ^ 0x55 and got[at + 1:] == s.content[at + 1:]


@pytest.mark.parametrize("fmt", ["zlib", "gzip"])
def test_a_moved_point_spoils_the_chunk_in_front_of_it(gpu, fmt):
    import compu_amd

    s = IC.damage(fmt)
    total = len(s.content)
    index, d_in, _ = index_of(gpu, fmt, s.data, total, 1)
    outs = u64(index.pt_out) + [total]
    j = 4
    pt_bit = index.pt_bit.clone()
    pt_bit[j + 1] += 1
    moved = compu_amd.InflateIndex(index.fmt, index.length, index.total_out, pt_bit, index.pt_out, index.pt_check, index.windows)
    ranges = [(outs[k], outs[k + 1] - outs[k]) for k in range(j + 1)]
    got, guards, dst_off, status, summ = read(gpu, moved, d_in, ranges)
    assert status == [RANGE_OK] * j + [RANGE_BAD_UNIT] and guards
    assert (summ.n_bad, summ.first_bad, summ.n_units, int(summ.status)) == (1, j, j + 1, READ_OK)
    assert got[:dst_off[j]] == s.content[:outs[j]]


@pytest.mark.parametrize("max_points", [1, 3])
def test_a_truncated_index_reads_the_whole_content(gpu, max_points):
    import compu_amd

    content, _, index, d_in = file_index(gpu, max_points=max_points)
    assert index.n_points == max_points
    assert compu_amd.gzip_index_decode(index, d_in).cpu().numpy().tobytes() == content
    out, dst_off = compu_amd.gzip_index_read(index, d_in, [(100000, 50), (5, 7)])
    assert out.cpu().numpy().tobytes() == content[100000:100050] + content[5:12] and u64(dst_off) == [0, 50]


# ---- what the index read shares with the plan read: the room, the layout, nothing to read, null outputs -------------------------
# One small stream (IC.edges: eight blocks, 57 KiB) at spacing 1, so that every block with content is a chunk.


def edges_index(gpu, fmt):
    """-> (content by the system zlib, the stream, its index at spacing 1, the stream on the device)"""
    s = IC.edges(fmt)
    content = zlib.decompress(s.data, R.FMT[fmt])
    index, d_in, _ = index_of(gpu, fmt, s.data, len(content), 1)
    assert index.n_points >= 3
    return content, s, index, d_in


def host_selection(index, ranges):
    """what the read has to answer, by host arithmetic alone: chip_inflate_index_units_host for the chunks, chip_select_units_host
    over them -> (dst_off, range status, SelectSummary)"""
    import compu_amd

    pt_bit, pt_out, pt_check = u64(index.pt_bit), u64(index.pt_out), u32(index.pt_check)
    in_off, in_len, out_cap, _, _, status, _ = compu_amd.inflate_index_units_host(index.fmt, index.length, pt_bit, pt_out, pt_check, index.total_out)
    assert status == READ_OK
    lo, ln = np.array([r[0] for r in ranges], np.uint64), np.array([r[1] for r in ranges], np.uint32)
    *_, dst_off, range_status, summ = compu_amd.select_units_host(in_off, in_len, pt_out, out_cap, lo, ln)
    return dst_off.tolist(), range_status.tolist(), summ


def raw_read(gpu, index, d_in, ranges, room, outputs=True):
    """chip_inflate_index_read through compu_amd.lib() into a poisoned dst with guards and poisoned dst_off / range_status, both null
    when `outputs` is false -> (all bytes of dst and its guards, dst_off, range_status, the summary as a tuple)"""
    import compu_amd
    from compu_amd.api import _ranges_to_device, _ReadSummary

    m = len(ranges)
    lo, ln = _ranges_to_device(ranges, gpu.device("cuda")) if m else (None, None)
    box = gpu.full((GUARD + room + GUARD,), POISON, dtype=gpu.uint8, device="cuda")
    dst_off = gpu.full((m * 8 + 8,), POISON, dtype=gpu.uint8, device="cuda").view(gpu.int64)
    status = gpu.full((m * 4 + 4,), POISON, dtype=gpu.uint8, device="cuda").view(gpu.int32)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    raw = _ReadSummary(7, 7, 7, 7, 7, 7, 1, 7)  # whatever the caller left there
    gpu.cuda.synchronize()
    rc = compu_amd.lib().chip_inflate_index_read(index.fmt, p(d_in), index.length, index.n_points, p(index.pt_bit), p(index.pt_out),
                                                 p(index.pt_check), p(index.windows), index.total_out, m, p(lo), p(ln),
                                                 C.c_void_p(box.data_ptr() + GUARD), room, p(dst_off) if outputs else None,
                                                 p(status) if outputs else None, C.byref(raw), None)
    assert rc == 0
    gpu.cuda.synchronize()
    return box.cpu().numpy().tobytes(), u64(dst_off), u32(status), compu_amd.ReadSummary(raw).as_tuple()


def edge_ranges(outs, total):
    """ranges across chunk edges, inside one chunk, of length 0, outside the content, out of order"""
    return [(outs[1] - 7, 20), (outs[2] - 1, outs[4] - outs[2] + 2), (outs[3] + 5, 100), (outs[2], 0), (total, 0), (total - 1, 2), (total + 9, 1),
            (total - 1, 1), (3, 40)]


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_need_output_writes_nothing_and_sizes_the_second_call(gpu, fmt):
    content, _, index, d_in = edges_index(gpu, fmt)
    ranges = edge_ranges(u64(index.pt_out), len(content))
    want_off, want_status, want = host_selection(index, ranges)
    assert want.n_outside == 2 and want.n_sel >= 4 and want.out_len == sum(ln for (_, ln), st in zip(ranges, want_status) if st == RANGE_OK)
    got, guards, dst_off, status, summ = read(gpu, index, d_in, ranges, room=want.out_len - 1)
    assert summ.as_tuple() == (0, want.out_len, want.n_outside, 0, 0, 0, READ_NEED_OUTPUT, 0)
    assert got == bytes([POISON]) * (want.out_len - 1) and guards, "no byte of dst, and none of the 64 behind it"
    assert (dst_off, status) == (want_off, want_status)
    got, guards, dst_off, status, summ = read(gpu, index, d_in, ranges, room=summ.out_len)
    assert summ.as_tuple() == (want.n_sel, want.out_len, want.n_outside, 0, 0, 0, READ_OK, 0) and guards
    assert got == b"".join(content[lo:lo + ln] for (lo, ln), st in zip(ranges, want_status) if st == RANGE_OK)
    assert (dst_off, status) == (want_off, want_status)


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_a_broken_index_layout_names_the_chunk_and_writes_nothing(gpu, fmt):
    import compu_amd

    content, _, index, d_in = edges_index(gpu, fmt)
    ranges = edge_ranges(u64(index.pt_out), len(content))
    room = len(content)
    untouched = bytes([POISON]) * (GUARD + room + GUARD)
    # pt_out[k] above pt_out[k + 1] for an inner k; a point that does not move on in the stream; content in front of the first point
    for name, k, value, chunk in (("pt_out", 2, u64(index.pt_out)[3] + 1, 2), ("pt_bit", 2, u64(index.pt_bit)[1], 1), ("pt_out", 0, 1, 0)):
        arrays = dict(pt_bit=index.pt_bit.clone(), pt_out=index.pt_out.clone())
        arrays[name][k] = value
        broken = compu_amd.InflateIndex(index.fmt, index.length, index.total_out, arrays["pt_bit"], arrays["pt_out"], index.pt_check, index.windows)
        pt_bit, pt_out = u64(broken.pt_bit), u64(broken.pt_out)
        *rows, status, bad = compu_amd.inflate_index_units_host(index.fmt, index.length, pt_bit, pt_out, u32(index.pt_check), index.total_out)
        assert (int(status), bad) == (READ_BAD_LAYOUT, chunk)
        assert R.units(R.WRAP[fmt], index.length, pt_bit, pt_out, u32(index.pt_check), index.total_out)[:2] == (READ_BAD_LAYOUT, chunk)
        box, dst_off, range_status, summ = raw_read(gpu, broken, d_in, ranges, room)
        assert summ == (0, 0, 0, 0, 0, bad, READ_BAD_LAYOUT, 0), "the lowest offending chunk, not the link behind it"
        assert box == untouched and set(dst_off) == {POISON64} and set(range_status) == {POISON64 & 0xFFFFFFFF}


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_nothing_to_read(gpu, fmt):
    import compu_amd
    from compu_amd.api import _ranges_to_device

    content, _, index, d_in = edges_index(gpu, fmt)
    outs, total = u64(index.pt_out), len(content)
    untouched = bytes([POISON]) * (GUARD + 32 + GUARD)
    # no ranges: CHIP_OK and the zero summary, whatever the caller left there
    box, dst_off, status, summ = raw_read(gpu, index, d_in, [], 32)
    assert summ == (0, 0, 0, 0, 0, 0, READ_OK, 0) and box == untouched and dst_off == [POISON64] and status == [POISON64 & 0xFFFFFFFF]
    lo, ln = _ranges_to_device([(0, 1)], gpu.device("cuda"))
    out, _, _, rs = compu_amd.inflate_index_read(index, d_in, lo[:0], ln[:0])
    assert rs.as_tuple() == (0, 0, 0, 0, 0, 0, READ_OK, 0) and out.numel() == 0
    # ranges of length 0, inside, on a chunk's edge, at the end and far outside: nothing is decoded
    ranges = [(0, 0), (outs[1], 0), (outs[2] + 3, 0), (total, 0), ((1 << 64) - 1, 0)]
    want_off, want_status, want = host_selection(index, ranges)
    assert (want.n_sel, want.out_len, want.n_outside) == (0, 0, 0) and want_status == [RANGE_OK] * len(ranges)
    box, dst_off, status, summ = raw_read(gpu, index, d_in, ranges, 32)
    assert summ == (0, 0, 0, 0, 0, 0, READ_OK, 0) and box == untouched
    assert (dst_off[:-1], status[:-1]) == (want_off, want_status) == ([0] * len(ranges), [RANGE_OK] * len(ranges))


@pytest.mark.parametrize("damaged", [False, True])
@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_null_dst_off_and_range_status_change_no_byte(gpu, fmt, damaged):
    """without range_status the scan of the bad flags is skipped: dst and the summary are those of the call that has both"""
    content, s, index, d_in = edges_index(gpu, fmt)
    outs, total = u64(index.pt_out), len(content)
    ranges = edge_ranges(outs, total) + [(0, total)]
    want_off, want_status, want = host_selection(index, ranges)
    n_bad, bad_chunk = 0, 0
    if damaged:  # one byte of the 20 000 stored ones flipped behind the build: raw deflate has no check value to miss
        data, at = IC.flipped_stored_byte(s, 5)
        d_in = upload(gpu, data)
        bad_chunk = max(k for k, o in enumerate(outs) if o <= at)
        n_bad = 0 if fmt == "raw" else 1
    with_both = raw_read(gpu, index, d_in, ranges, want.out_len)
    with_none = raw_read(gpu, index, d_in, ranges, want.out_len, outputs=False)
    assert with_none[0] == with_both[0] and with_none[3] == with_both[3]
    assert set(with_none[1]) == {POISON64} and set(with_none[2]) == {POISON64 & 0xFFFFFFFF}
    box, dst_off, status, summ = with_both
    assert summ[:5] == (want.n_sel, want.out_len, want.n_outside, n_bad, bad_chunk if n_bad else 0) and summ[6] == READ_OK
    assert box[:GUARD] == box[GUARD + want.out_len:] == bytes([POISON]) * GUARD and dst_off[:-1] == want_off
    if n_bad:
        touched = [st == RANGE_OK and ln > 0 and lo < outs[bad_chunk + 1] and lo + ln > outs[bad_chunk] for (lo, ln), st in zip(ranges, want_status)]
        assert status[:-1] == [RANGE_BAD_UNIT if t else st for t, st in zip(touched, want_status)] and any(touched) and not all(touched)
    else:
        assert status[:-1] == want_status
        truth = content if not damaged else content[:at] + bytes([content[at] ^ 0x55]) + content[at + 1:]
        assert box[GUARD:GUARD + want.out_len] == b"".join(truth[lo:lo + ln] for (lo, ln), st in zip(ranges, want_status) if st == RANGE_OK)


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_the_plan_read_and_the_index_read_agree(gpu, fmt):
    """The same content as five gzip members (a plan whose units are whole members) and as one stream whose five blocks are the
    members' content (an index at spacing 1 whose chunks are those blocks): the two reads answer the same."""
    import compu_amd
    import deflate_writer as W
    import gzip_plan_cases as GP
    from compu_amd.api import _ranges_to_device

    pieces = [GP.text(3000, 1), GP.noise(1, 2), GP.text(4096, 3), GP.noise(2500, 4), GP.text(777, 5)]
    content = b"".join(pieces)
    cum = [sum(len(p) for p in pieces[:k]) for k in range(len(pieces) + 1)]
    members = b"".join(GP.member(p) for p in pieces)
    assert b"".join(zlib.decompress(GP.member(p), 31) for p in pieces) == content
    d = W.Deflate()
    d.dynamic(list(pieces[0])).stored(pieces[1]).fixed(list(pieces[2])).stored(pieces[3]).dynamic(list(pieces[4]), final=True)
    one = W.wrap(d, fmt)
    assert zlib.decompress(one.data, R.FMT[fmt]) == content
    buf = upload(gpu, members)
    *rows, ps = compu_amd.gzip_plan(buf, len(members))
    index, d_in, _ = index_of(gpu, fmt, one.data, len(content), 1)
    assert (ps.n_members, int(ps.status)) == (5, 0) and u64(rows[2]) == u64(index.pt_out) == cum[:-1] and u32(rows[3]) == [len(p) for p in pieces]
    total = len(content)
    ranges = [(cum[1] - 5, 10), (cum[3] - 1, 2), (cum[2], 0), (total, 0), (0, total), (total - 1, 2), (total + 5, 1), (cum[4], 1), (10, 20),
              (cum[2] + 1, cum[3] - cum[2] - 2)]
    want_off, want_status, want = host_selection(index, ranges)
    assert want.n_outside == 2 and want.n_sel == 5
    lo, ln = _ranges_to_device(ranges, gpu.device("cuda"))
    by_plan = compu_amd.read_ranges(31, buf, *rows, lo, ln)
    by_index = compu_amd.inflate_index_read(index, d_in, lo, ln)
    for out, dst_off, status, summ in (by_plan, by_index):
        assert summ.as_tuple() == (want.n_sel, want.out_len, want.n_outside, 0, 0, 0, READ_OK, 0)
        assert (u64(dst_off), status.cpu().tolist()) == (want_off, want_status)
        assert out.cpu().numpy().tobytes() == b"".join(content[lo:lo + ln] for (lo, ln), st in zip(ranges, want_status) if st == RANGE_OK)
    assert gpu.equal(by_plan[0], by_index[0]) and gpu.equal(by_plan[1], by_index[1]) and gpu.equal(by_plan[2], by_index[2])
