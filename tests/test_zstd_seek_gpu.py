"""Seekable zstd files on the device: chip_xxh64_batch against the Python XXH64, chip_zstd_seek_plan against the host walk at every
alignment, chip_zstd_seek_table_write against the host form and against the table chip_encode_file writes, seekable_write and
SeekableZstd end to end, chip_zstd_seek_read on ranges of every kind, damage that only the table's checksum catches, a reader that
fetches only the frames it needs, and the life cycle of the plan's launch slot."""
import ctypes as C
import functools

import numpy as np
import pytest

import seek_cases as S
import seek_ref as R
from conftest import golden
from test_zstd_seek_cpu import _host_plan, _LoggingFile

pytestmark = pytest.mark.gpu
FMT_ZSTD = 100
RANGE_OK, RANGE_OUTSIDE, RANGE_BAD_UNIT = 0, 1, 2
CANARY32, CANARY64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _up(torch, a, dt=None):
    a = np.array(a)  # (a writable, contiguous copy)
    return torch.from_numpy(a.view(dt) if dt is not None else a).to("cuda:0")


def _at_alignment(torch, data, a, fill=0xC3):
    """a device buffer with `data` at byte a (0..7) of a fresh allocation, `fill` around it: (buffer, the view of the data)"""
    buf = torch.full((len(data) + 16,), fill, dtype=torch.uint8, device="cuda:0")
    if len(data):
        buf[a:a + len(data)] = _up(torch, np.frombuffer(bytes(data), np.uint8))
    return buf, buf[a:a + len(data)]


@functools.lru_cache(maxsize=None)
def _content():
    return golden("alice29.txt")[:100003]


def test_xxh64_batch_equals_the_python_xxh64(gpu):
    """every edge length at every start alignment 0..7 in one call; the buffer and the entry behind `digest` stay as they were"""
    import compu_amd

    torch = gpu
    rng = np.random.default_rng(11)
    offs, lens, at = [], [], 5
    for n in S.XXH_LENGTHS:
        for a in range(8):
            at = (at + 15) // 8 * 8 + a  # a gap of at least 8 bytes, then the alignment
            offs.append(at)
            lens.append(n)
            at += n
    data = rng.integers(0, 256, at + 64, dtype=np.uint8)
    want = [R.xxh64(data[o:o + n].tobytes()) for o, n in zip(offs, lens)]
    d = _up(torch, data)
    d_off, d_len = _up(torch, np.array(offs, np.uint64), np.int64), _up(torch, np.array(lens, np.uint32), np.int32)
    digest = torch.full((len(offs) + 1,), CANARY64, dtype=torch.int64, device="cuda:0")
    rc = compu_amd.lib().chip_xxh64_batch(len(offs), C.c_void_p(d.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_len.data_ptr()),
                                          C.c_void_p(digest.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    got = digest.cpu().numpy().view(np.uint64)
    bad = [(o % 8, n) for o, n, g, w in zip(offs, lens, got[:-1].tolist(), want) if g != w]
    assert not bad, bad[:10]
    assert int(got[-1]) == CANARY64 and np.array_equal(d.cpu().numpy(), data)
    assert int(got[0]) == R.XXH64_EMPTY
    # the Python face: the same digests, and an empty batch
    face = compu_amd.xxh64_batch(d, d_off, d_len)
    assert face.cpu().numpy().view(np.uint64).tolist() == want
    assert compu_amd.xxh64_batch(d, d_off[:0], d_len[:0]).numel() == 0
    lib, q = compu_amd.lib(), C.c_void_p(d.data_ptr())
    assert lib.chip_xxh64_batch(0, None, None, None, None, None) == 0
    assert lib.chip_xxh64_batch(1, None, q, q, q, None) == -101 and lib.chip_xxh64_batch(1, q, q, q, None, None) == -101
    assert lib.chip_xxh64_batch(1 << 31, q, q, q, q, None) == -101


def _dev_plan(torch, view, file_len, max_frames, want_checksum=True, canary=3):
    """chip_zstd_seek_plan through ctypes into canaried device arrays: (rows, summary tuple), as _host_plan"""
    import compu_amd
    from compu_amd.api import _ZstdSeekSummary

    lib, raw = compu_amd.lib(), _ZstdSeekSummary()
    m = max_frames + canary
    in_off, out_off = (torch.full((m,), CANARY64, dtype=torch.int64, device="cuda:0") for _ in range(2))
    in_len, out_cap, cs = (torch.full((m,), CANARY32, dtype=torch.int32, device="cuda:0") for _ in range(3))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.chip_zstd_seek_plan(p(view) if view.numel() else None, view.numel(), file_len, max_frames, p(in_off), p(in_len), p(out_off), p(out_cap),
                                 p(cs) if want_checksum else None, C.byref(raw), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    summ = tuple(getattr(raw, f) for f, _ in raw._fields_)
    k = min(max_frames, summ[0]) if summ[5] == R.OK else 0
    host = [t.cpu().numpy() for t in (in_off, in_len, out_off, out_cap, cs)]
    if summ[5] == R.OK:
        for a in host[:4] + (host[4:] if want_checksum else []):
            assert (a[k:] == (CANARY64 if a.dtype == np.int64 else CANARY32)).all()
    if not want_checksum:
        assert (host[4] == CANARY32).all()
    cols = [a[:k].view(np.uint64 if a.dtype == np.int64 else np.uint32) for a in host]
    if not want_checksum:
        cols[4] = np.zeros(k, np.uint32)
    return cols, summ


def _columns(rows):
    """the rows of _host_plan as the five arrays _dev_plan returns"""
    return [np.array([r[j] for r in rows], dtype=dt) for j, dt in enumerate((np.uint64, np.uint32, np.uint64, np.uint32, np.uint32))]


def _same(cols, want, upto=None, checksum=True):
    return all(np.array_equal(c, w[:upto]) for c, w in list(zip(cols, want))[:5 if checksum else 4])


def test_seek_plan_equals_the_host_walk_at_every_alignment(gpu):
    """every case of the CPU list, OK or not, with the table at each alignment mod 4 of the device buffer (4..7 once more for the
    small ones); counting, filling, a partial fill and no checksum array"""
    torch = gpu
    for case in S.tables():
        want_rows, want = _host_plan(case.tail, case.file_len)
        want_cols = _columns(want_rows)
        n = want[0] if want[5] == R.OK else 0
        for a in (range(8) if len(case.tail) < 100 else range(4)):
            buf, view = _at_alignment(torch, case.tail, a)
            assert _dev_plan(torch, view, case.file_len, 0)[1] == want, (case.name, a)
            cols, summ = _dev_plan(torch, view, case.file_len, n)
            assert summ == want and _same(cols, want_cols), (case.name, a)
            if a == 1 and n > 1:
                cols, summ = _dev_plan(torch, view, case.file_len, n // 2)
                assert summ == want and _same(cols, want_cols, upto=n // 2), case.name
                cols, summ = _dev_plan(torch, view, case.file_len, n, want_checksum=False)
                assert summ == want and _same(cols, want_cols, checksum=False), case.name
            assert (buf[:a] == 0xC3).all() and (buf[a + len(case.tail):] == 0xC3).all()


def test_seek_plan_python_face(gpu):
    import compu_amd

    torch = gpu
    case = S.by_name("n257_cs1_extra3_cut0")
    _, view = _at_alignment(torch, case.tail, 3)
    got = compu_amd.zstd_seek_plan(view, case.file_len)
    want = compu_amd.zstd_seek_plan_host(case.tail, case.file_len)
    assert got[5].as_tuple() == want[5].as_tuple() and got[5].status == compu_amd.ZstdSeekStatus.Ok
    for g, w in zip(got[:5], want[:5]):
        assert g.cpu().numpy().view(w.dtype).tolist() == w.tolist()
    bad = compu_amd.zstd_seek_plan(_at_alignment(torch, S.by_name("unsized_middle").tail, 1)[1], S.by_name("unsized_middle").file_len)
    assert bad[5].status == compu_amd.ZstdSeekStatus.TooLarge and bad[5].bad_index == 2 and bad[0].numel() == 0


def test_table_write_equals_the_host_form_at_every_alignment(gpu):
    import compu_amd

    torch = gpu
    for n in S.NS:
        c, d, x = S.entries(n)
        d_c, d_d, d_x = (_up(torch, v, np.int32) for v in (c, d, x))
        for cs, d_cs in ((None, None), (x, d_x)):
            want = compu_amd.zstd_seek_table_write_host(c, d, cs)
            for a in range(4):
                buf, view = _at_alignment(torch, bytes(len(want)), a)
                out, size = compu_amd.zstd_seek_table_write(d_c, d_d, d_cs, out=view)
                torch.cuda.synchronize()
                assert size == len(want) and bytes(out.cpu().numpy()) == want, (n, cs is not None, a)
                assert (buf[:a] == 0xC3).all() and (buf[a + len(want):] == 0xC3).all()
            # one byte short: the size, and nothing written
            buf, view = _at_alignment(torch, bytes(len(want) - 1), 1)
            out, size = compu_amd.zstd_seek_table_write(d_c, d_d, d_cs, out=view)
            torch.cuda.synchronize()
            assert out is None and size == len(want) and (buf[:1] == 0xC3).all() and (buf[1:len(want)] == 0).all() and (buf[len(want):] == 0xC3).all()


def test_table_without_checksums_is_the_one_encode_file_writes(gpu):
    import compu_amd

    torch = gpu
    data = _content()
    d_in = _up(torch, np.frombuffer(data + bytes(1), np.uint8))
    out, summ = compu_amd.encode_file(FMT_ZSTD, 3, d_in, len(data), unit_bytes=4096, flags=compu_amd.W_SEEK_TABLE)
    table = out[summ.table_off:]
    _, c_len, _, d_len, cs, plan = compu_amd.zstd_seek_plan(table, summ.out_len)
    assert plan.status == compu_amd.ZstdSeekStatus.Ok and plan.n_frames == summ.n_units == 25 and plan.checksums == 0
    assert plan.frames_bytes == summ.table_off and plan.total_out == len(data)
    again, size = compu_amd.zstd_seek_table_write(c_len, d_len, None)
    torch.cuda.synchronize()
    assert size == table.numel() and torch.equal(again, table)


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("unit", [1000, 4096, 65536])
def test_seekable_write_then_open(gpu, unit, level):
    """the table's checksums are the frames' own content checksums (the encoder's, old code) and the Python XXH64 of the chunks; the
    frame walk of chip_zstd_plan agrees with the table on all four arrays; the reader gives the content back"""
    import compu_amd

    torch = gpu
    data = _content()
    d_in = _up(torch, np.frombuffer(data + bytes(1), np.uint8))
    out, summ = compu_amd.seekable_write(d_in, len(data), level=level, unit_bytes=unit)
    n = -(-len(data) // unit)
    assert summ.status == compu_amd.FileStatus.Ok and summ.n_units == n and summ.out_len == out.numel() == summ.table_off + 17 + 12 * n
    z = compu_amd.SeekableZstd.open(out)
    assert (z.n_frames, z.size, z.has_checksums) == (n, len(data), True)
    file = bytes(out.cpu().numpy())
    for i in range(n):
        end = int(z.in_off[i]) + int(z.in_len[i])
        assert int(z.checksum[i]) == int.from_bytes(file[end - 4:end], "little"), i
        assert int(z.checksum[i]) == R.xxh64(data[i * unit:(i + 1) * unit]) & 0xFFFFFFFF, i
    in_off, in_len, out_off, out_cap, plan = compu_amd.zstd_plan(out, out.numel())
    assert plan.status == compu_amd.ZstdPlanStatus.Ok and (plan.n_frames, plan.n_skippable, plan.n_unsized) == (n, 1, 0)
    for got, want in zip((in_off, in_len, out_off, out_cap), (z.in_off, z.in_len, z.out_off, z.out_cap)):
        assert got.cpu().numpy().view(want.dtype).tolist() == want.tolist()
    got, dst_off = z.read([(0, len(data))])
    assert bytes(got.cpu().numpy()) == data and dst_off.tolist() == [0]
    assert z.read_bytes(len(data) - 5, 5) == data[-5:] and z.bytes_fetched == 0
    # no checksums: 8-byte entries, the same frames
    plain, s2 = compu_amd.seekable_write(d_in, len(data), level=level, unit_bytes=unit, checksums=False)
    assert s2.out_len == s2.table_off + 17 + 8 * n and s2.table_off == summ.table_off and torch.equal(plain[:s2.table_off], out[:summ.table_off])
    # an `out` that is too small by one byte
    small = torch.zeros(summ.out_len - 1, dtype=torch.uint8, device="cuda:0")
    none, s3 = compu_amd.seekable_write(d_in, len(data), level=level, unit_bytes=unit, out=small)
    assert none is None and s3.status == compu_amd.FileStatus.NeedOutput and s3.out_len == summ.out_len


@functools.lru_cache(maxsize=None)
def _seekable_1000():
    """the content in frames of 1000 bytes: (file tensor, plan tensors with checksums)"""
    import torch

    import compu_amd

    data = _content()
    out, _ = compu_amd.seekable_write(_up(torch, np.frombuffer(data + bytes(1), np.uint8)), len(data), level=3, unit_bytes=1000)
    file = torch.zeros((out.numel() + 3) // 4 * 4, dtype=torch.uint8, device="cuda:0")
    file[:out.numel()] = out
    return file, compu_amd.zstd_seek_plan(file[:out.numel()])


def test_seek_read_ranges_of_every_kind(gpu):
    import compu_amd

    torch = gpu
    data = _content()
    file, (in_off, in_len, out_off, out_cap, cs, plan) = _seekable_1000()
    assert plan.n_frames == 101 and plan.checksums == 1
    ranges = [(2100, 300), (2990, 20), (4500, 4100), (0, len(data)), (777, 0), (2100, 300), (2200, 900), (len(data) - 3, 4), (99999, 4)]
    lo, ln = _up(torch, np.array([r[0] for r in ranges], np.int64)), _up(torch, np.array([r[1] for r in ranges], np.int32))
    out, dst_off, status, summ = compu_amd.zstd_seek_read(file, in_off, in_len, out_off, out_cap, cs, lo, ln)
    assert status.tolist() == [RANGE_OK] * 7 + [RANGE_OUTSIDE, RANGE_OK]
    assert (summ.n_units, summ.n_outside, summ.n_bad, int(summ.status)) == (101, 1, 0, 0)
    got, at = bytes(out.cpu().numpy()), 0
    for (a, n), o, st in zip(ranges, dst_off.tolist(), status.tolist()):
        assert o == at
        if st == RANGE_OK:
            assert got[o:o + n] == data[a:a + n], (a, n)
            at += n
    assert len(got) == at == summ.out_len
    # without the whole-content range only the touched frames are decoded
    few = [0, 1, 2, 4, 5, 6, 8]
    out2, _, status2, summ2 = compu_amd.zstd_seek_read(file, in_off, in_len, out_off, out_cap, cs, lo[few], ln[few])
    assert summ2.n_units == len({2, 3, 4, 5, 6, 7, 8, 99, 100}) and summ2.n_bad == 0 and status2.tolist() == [0] * 7
    # checksum None is read_ranges, to the byte and to the summary
    a = compu_amd.zstd_seek_read(file, in_off, in_len, out_off, out_cap, None, lo, ln)
    b = compu_amd.read_ranges(FMT_ZSTD, file, in_off, in_len, out_off, out_cap, lo, ln)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3].as_tuple() == b[3].as_tuple()
    assert torch.equal(a[0], out) and a[3].as_tuple() == summ.as_tuple()


def test_damage_that_only_the_table_catches(gpu):
    """raw-block frames without a content checksum: a flipped content byte decodes Finished at full length, and only the table's
    XXH64 knows"""
    import compu_amd

    torch = gpu
    file, contents, frames = S.raw_frames_file(20)
    content = b"".join(contents)
    starts = np.cumsum([0] + [len(c) for c in contents]).tolist()
    fstarts = np.cumsum([0] + [len(f) for f in frames]).tolist()
    hurt = bytearray(file)
    hurt[fstarts[8] - 1] ^= 0x20  # the last content byte of frame 7
    wrong_table = bytearray(file)
    wrong_table[fstarts[20] + 8 + 12 * 7 + 8] ^= 1  # the checksum of entry 7, the data intact
    ranges = [(starts[7] + 5, 10), (starts[6] + 1, len(contents[6]) + len(contents[7]) + 3), (starts[3], 50), (0, len(content)), (starts[9], 7),
              (starts[6], len(contents[6]))]
    touch7 = [True, True, False, True, False, False]
    lo, ln = _up(torch, np.array([r[0] for r in ranges], np.int64)), _up(torch, np.array([r[1] for r in ranges], np.int32))

    def read(image, verify, pick=slice(None)):
        d = _up(torch, np.frombuffer(bytes(image) + bytes(-len(image) % 4), np.uint8))
        in_off, in_len, out_off, out_cap, cs, plan = compu_amd.zstd_seek_plan(d[:len(image)])
        assert plan.status == compu_amd.ZstdSeekStatus.Ok and plan.n_frames == 20 and plan.checksums == 1
        return compu_amd.zstd_seek_read(d, in_off, in_len, out_off, out_cap, cs if verify else None, lo[pick], ln[pick])

    for image in (hurt, wrong_table):
        out, dst_off, status, summ = read(image, True)
        assert (summ.n_units, summ.n_bad, summ.first_bad, summ.bad_status, int(summ.status)) == (20, 1, 7, -22, 0)
        assert status.tolist() == [RANGE_BAD_UNIT if t else RANGE_OK for t in touch7]
        got = bytes(out.cpu().numpy())
        for (a, n), o, t in zip(ranges, dst_off.tolist(), touch7):
            assert t or got[o:o + n] == content[a:a + n]
    # the intact file verifies
    out, _, status, summ = read(file, True)
    assert summ.n_bad == 0 and status.tolist() == [0] * 6 and bytes(out.cpu().numpy()) == b"".join(content[a:a + n] for a, n in ranges)
    # verify off: the damaged bytes, without complaint
    out, dst_off, status, summ = read(hurt, False)
    assert (summ.n_bad, summ.first_bad, summ.bad_status) == (0, 0, 0) and status.tolist() == [0] * 6
    damaged = bytearray(content)
    damaged[starts[8] - 1] ^= 0x20
    assert bytes(out.cpu().numpy()) == b"".join(bytes(damaged[a:a + n]) for a, n in ranges)
    # a read that does not touch frame 7 reports nothing
    out, _, status, summ = read(hurt, True, pick=[2, 4, 5])
    assert (summ.n_units, summ.n_bad) == (3, 0) and status.tolist() == [0, 0, 0]
    assert bytes(out.cpu().numpy()) == b"".join(content[a:a + n] for a, n in (ranges[2], ranges[4], ranges[5]))
    # the reader raises with the frame and the status, and reads on request without the check
    z = compu_amd.SeekableZstd.open(bytes(hurt))
    with pytest.raises(RuntimeError, match="unit 7 did not decode: status -22"):
        z.read([(starts[7], 4)])
    assert z.read_bytes(starts[8] - 2, 2, verify=False) == bytes(damaged[starts[8] - 2:starts[8]])
    assert z.read_bytes(starts[8], 9) == content[starts[8]:starts[8] + 9]
    with pytest.raises(ValueError, match="outside"):
        z.read([(len(content), 1)])


def test_reader_fetches_the_table_and_the_touched_frames_only(gpu):
    import compu_amd

    torch = gpu
    file, contents, frames = S.raw_frames_file(64, size=200)
    content = b"".join(contents)
    starts = np.cumsum([0] + [len(c) for c in contents]).tolist()
    fstarts = np.cumsum([0] + [len(f) for f in frames]).tolist()
    T = 17 + 12 * 64
    f = _LoggingFile(file)
    z = compu_amd.SeekableZstd.open(f, tail_bytes=T)
    assert f.reads == [(len(file) - T, T)] and z.bytes_fetched == T
    ranges = [(starts[40] + 3, 20), (starts[3], len(contents[3])), (starts[11] - 2, 10)]
    del f.reads[:]
    out, dst_off = z.read(ranges)
    assert bytes(out.cpu().numpy()) == b"".join(content[a:a + n] for a, n in ranges) and dst_off.tolist() == [0, 20, 20 + len(contents[3])]
    want = [(fstarts[3], len(frames[3])), (fstarts[10], len(frames[10]) + len(frames[11])), (fstarts[40], len(frames[40]))]
    assert f.reads == want  # frames 10 and 11 in one read
    # the union of everything read from the file: the table's span and those four frames' spans, and bytes_fetched is its size
    assert z.bytes_fetched == T + sum(len(frames[k]) for k in (3, 10, 11, 40))
    # the same ranges from the file in device memory
    d = _up(torch, np.frombuffer(file + bytes(-len(file) % 4), np.uint8))
    zd = compu_amd.SeekableZstd.open(d, length=len(file), tail_bytes=17)
    out_d, dst_off_d = zd.read(ranges)
    assert torch.equal(out_d, out) and torch.equal(dst_off_d, dst_off) and zd.bytes_fetched == 0
    assert zd.in_off.tolist() == z.in_off.tolist() and zd.checksum.tolist() == z.checksum.tolist()


def test_trim_plan_trim_plan(gpu):
    """chip_trim() releases the plan's slot of a non-default stream; the next plan there allocates it again: the same answer"""
    import compu_amd

    torch = gpu
    case = S.by_name("n1025_cs1_whole")
    _, view = _at_alignment(torch, case.tail, 2)
    stream = torch.cuda.Stream()
    results = []
    for _ in range(2):
        compu_amd.trim()
        with torch.cuda.stream(stream):
            got = compu_amd.zstd_seek_plan(view, case.file_len, stream=stream)
            results.append(([t.cpu().numpy().tolist() for t in got[:5]], got[5].as_tuple()))
    compu_amd.trim()
    assert results[0] == results[1] and results[0][1][5] == R.OK and results[0][1][0] == 1025
