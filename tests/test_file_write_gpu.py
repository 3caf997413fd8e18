"""chip_encode_file on the GPU: the file equals the units of chip_encode_batch laid end to end (plus the EOF block for BGZF) --
the contract "the same bytes as the batch encoder" --, is read back by gzip, by libzstd, by chip_bgzf_plan / bgzf_decode, by a
CHIP_F_MEMBERS unit and by chip_zstd_plan / zstd_frames_decode, carries a seek table that says what the plan says, reports
CHIP_FILE_NEED_OUTPUT without writing, and serves two host threads on one stream.  Without the feature every test here fails at
the missing symbols."""
import ctypes as C
import gzip
import threading

import numpy as np
import pytest

import file_cases as F
import zstd_ref
from file_cases import FMT_BGZF, FMT_GZIP, FMT_ZSTD, W_SEEK_TABLE

pytestmark = pytest.mark.gpu

LIBZSTD = zstd_ref.load()
POISON, ENC_FINISHED, FINISHED, F_MEMBERS = 0xEE, 2, 2, 2
UNITS = [F.BGZF_PAYLOAD, 1000]  # the BGZF default (BGZF: passed as 0), and about 150 units with a short last one


def upload(torch, data):
    """`data` in a 16-byte aligned device tensor padded to a multiple of 4 (and never empty)"""
    t = torch.full(((len(data) + 3) // 4 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


def variants(alice, unit):
    return [("alice", alice), ("empty", b""), ("one_byte", alice[:1]), ("one_unit", alice[:unit]), ("two_units", alice[:2 * unit])]


def batch_file(torch, fmt, level, data, unit_bytes):
    """what chip_encode_batch writes for the same cuts, each unit in a slot of its own chip_encode_bound, end to end (bytes)"""
    import compu_amd

    cuts = F.cuts(fmt, len(data), unit_bytes)
    if not cuts:
        return b"", []
    caps = [compu_amd.encode_bound(fmt, ln) for _, ln in cuts]
    out_off = np.concatenate(([0], np.cumsum([(c + 15) // 16 * 16 for c in caps]))).astype(np.int64)
    d_out = torch.zeros(int(out_off[-1]) + 16, dtype=torch.uint8, device="cuda")
    i64 = lambda v: torch.from_numpy(np.asarray(v, np.int64)).cuda()  # noqa: E731
    i32 = lambda v: torch.from_numpy(np.asarray(v, np.int32)).cuda()  # noqa: E731
    out_len, status = compu_amd.encode_batch(fmt, level, upload(torch, data), i64([o for o, _ in cuts]), i32([ln for _, ln in cuts]), d_out,
                                             i64(out_off[:-1]), i32(caps))
    torch.cuda.synchronize()
    assert status.tolist() == [ENC_FINISHED] * len(cuts)
    host, lens = d_out.cpu().numpy(), out_len.tolist()
    return b"".join(host[o:o + n].tobytes() for o, n in zip(out_off[:-1].tolist(), lens)), lens


def write_file(torch, fmt, level, data, unit_bytes, flags=0):
    """chip_encode_file into a poisoned tensor of chip_encode_file_bound + 64 bytes: (the device tensor, the file's bytes, summary);
    nothing behind out_len has been written"""
    import compu_amd

    bound = compu_amd.encode_file_bound(fmt, len(data), unit_bytes, flags)
    assert bound > 0
    d_file = torch.full((bound + 64,), POISON, dtype=torch.uint8, device="cuda")
    out, summ = compu_amd.encode_file(fmt, level, upload(torch, data), len(data), unit_bytes, flags, out=d_file[:bound])
    assert summ.status == compu_amd.FileStatus.Ok and summ.out_len <= bound and out.numel() == summ.out_len
    host = d_file.cpu().numpy()
    assert (host[summ.out_len:] == POISON).all(), "bytes behind the file were written"
    return d_file, host[:summ.out_len].tobytes(), summ


def cases(alice, fmt):
    for unit in UNITS:
        unit_bytes = 0 if (fmt == FMT_BGZF and unit == F.BGZF_PAYLOAD) else unit
        for name, data in variants(alice, unit):
            yield f"{name}/{unit}", data, unit_bytes
    if fmt != FMT_BGZF:
        yield "alice/default", alice, 0  # 262 144: one unit


@pytest.mark.parametrize("level", [1, 6])
def test_bgzf_file(gpu, alice, level):
    import compu_amd

    eof = compu_amd.bgzf_eof_block()
    for name, data, unit_bytes in cases(alice, FMT_BGZF):
        want, lens = batch_file(gpu, FMT_BGZF, level, data, unit_bytes)
        d_file, got, summ = write_file(gpu, FMT_BGZF, level, data, unit_bytes)
        n = len(F.cuts(FMT_BGZF, len(data), unit_bytes))
        assert summ.as_tuple() == (n, len(want) + 28, len(want) + 28, 0), name
        assert got == want + eof, name
        assert gzip.decompress(got) == data, name
        *_, plan = compu_amd.bgzf_plan(d_file, summ.out_len)
        assert plan.as_tuple() == (n + 1, len(data), summ.out_len, 0, 1), name
        assert compu_amd.bgzf_decode(d_file, summ.out_len).cpu().numpy().tobytes() == data, name
    out, summ = compu_amd.bgzf_write(upload(gpu, alice), len(alice), level=level)
    assert out.cpu().numpy().tobytes() == write_file(gpu, FMT_BGZF, level, alice, 0)[1] and summ.n_units == 3  # alice in blocks of 65 280


@pytest.mark.parametrize("level", [1, 6])
def test_gzip_file(gpu, alice, level):
    import compu_amd

    i64 = lambda v: gpu.tensor([v], dtype=gpu.int64, device="cuda")  # noqa: E731
    i32 = lambda v: gpu.tensor([v], dtype=gpu.int32, device="cuda")  # noqa: E731
    for name, data, unit_bytes in cases(alice, FMT_GZIP):
        want, lens = batch_file(gpu, FMT_GZIP, level, data, unit_bytes)
        d_file, got, summ = write_file(gpu, FMT_GZIP, level, data, unit_bytes)
        assert summ.as_tuple() == (len(lens), len(want), len(want), 0), name
        assert got == want, name
        assert gzip.decompress(got) == data, name
        back = gpu.zeros(len(data) + 16, dtype=gpu.uint8, device="cuda")
        out_len, in_used, status = compu_amd.decode_batch(FMT_GZIP, d_file, i64(0), i32(summ.out_len), back, i64(0), i32(len(data)), flags=F_MEMBERS)
        gpu.cuda.synchronize()
        assert (int(status[0]), int(out_len[0]), int(in_used[0])) == (FINISHED, len(data), summ.out_len), name
        assert back.cpu().numpy()[:len(data)].tobytes() == data, name


def libzstd_decompress(data, room):
    z = LIBZSTD
    z.ZSTD_decompress.restype = C.c_size_t
    z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    dst = C.create_string_buffer(room + 1)
    n = z.ZSTD_decompress(dst, room + 1, data, len(data))
    assert not z.ZSTD_isError(n), z.ZSTD_getErrorCode(n)
    return dst.raw[:n]


@pytest.mark.parametrize("flags", [0, W_SEEK_TABLE], ids=["frames", "seek_table"])
@pytest.mark.parametrize("level", [1, 3])
def test_zstd_file(gpu, alice, level, flags):
    import compu_amd

    for name, data, unit_bytes in cases(alice, FMT_ZSTD):
        want, lens = batch_file(gpu, FMT_ZSTD, level, data, unit_bytes)
        d_file, got, summ = write_file(gpu, FMT_ZSTD, level, data, unit_bytes, flags)
        n = len(lens)
        table = 17 + 8 * n if flags else 0
        assert summ.as_tuple() == (n, len(want) + table, len(want), 0), name
        assert got[:summ.table_off] == want, name
        in_off, in_len, out_off, out_cap, plan = compu_amd.zstd_plan(d_file, summ.out_len)
        assert (plan.n_frames, plan.n_unsized, plan.n_skippable, plan.in_used, int(plan.status)) == (n, 0, 1 if flags else 0, summ.out_len, 0), name
        assert plan.total_out == len(data) and in_len.tolist() == lens, name
        assert compu_amd.zstd_frames_decode(d_file, summ.out_len)[0].cpu().numpy().tobytes() == data, name
        if LIBZSTD is not None:  # (libzstd steps over the skippable frame)
            assert libzstd_decompress(got, len(data)) == data, name
        if flags:
            assert summ.table_off + 17 + 8 * n == summ.out_len, name
            assert F.parse_seek_table(got, summ.table_off) == list(zip(in_len.tolist(), out_cap.tolist())), name
            assert got[summ.table_off:] == F.seek_table([(c, ln) for c, (_, ln) in zip(lens, F.cuts(FMT_ZSTD, len(data), unit_bytes))]), name


@pytest.mark.parametrize("fmt,flags", [(FMT_BGZF, 0), (FMT_GZIP, 0), (FMT_ZSTD, 0), (FMT_ZSTD, W_SEEK_TABLE)], ids=["bgzf", "gzip", "zstd", "zstd_table"])
def test_need_output_writes_nothing(gpu, alice, fmt, flags):
    import compu_amd

    for data, unit_bytes in ((alice, 1000), (b"", 0), (alice[:70000], 0)):
        for level in (1, 6) if fmt != FMT_ZSTD else (1, 3):
            _, want, summ = write_file(gpu, fmt, level, data, unit_bytes, flags)
            exact = summ.out_len
            assert compu_amd.encode_file_bound(fmt, len(data), unit_bytes, flags) >= exact
            d_in = upload(gpu, data)
            for dst_mis in (0, 7):
                room = gpu.full((exact + 64,), POISON, dtype=gpu.uint8, device="cuda")
                out, short = compu_amd.encode_file(fmt, level, d_in, len(data), unit_bytes, flags, out=room[dst_mis:dst_mis + exact - 1])
                assert out is None and short.as_tuple() == (summ.n_units, exact, summ.table_off, F.FILE_NEED_OUTPUT)
                assert (room.cpu().numpy() == POISON).all(), "the output was written although the file does not fit"
                out, fits = compu_amd.encode_file(fmt, level, d_in, len(data), unit_bytes, flags, out=room[dst_mis:dst_mis + exact])
                assert fits.as_tuple() == summ.as_tuple() and out.numel() == exact
                host = room.cpu().numpy()
                assert host[dst_mis:dst_mis + exact].tobytes() == want
                assert (host[:dst_mis] == POISON).all() and (host[dst_mis + exact:] == POISON).all(), "bytes around the file were written"
    # no room at all, and no output pointer
    from compu_amd.api import _FileSummary

    s = _FileSummary()
    d_in = upload(gpu, alice)
    rc = compu_amd.lib().chip_encode_file(fmt, 1, 1000, flags, C.c_void_p(d_in.data_ptr()), len(alice), None, 0, C.byref(s),
                                          C.c_void_p(gpu.cuda.current_stream().cuda_stream))
    assert rc == 0 and s.status == F.FILE_NEED_OUTPUT and s.out_len > 0


def test_two_host_threads_write_on_one_stream(gpu, alice):
    """The slot is locked from its lookup to the wait behind the last launch: two threads with inputs of different sizes (the
    scratch of one would not do for the other) on the same stream get their own files every time; chip_trim() releases the slot
    and the next call allocates again."""
    import compu_amd

    jobs = [(FMT_ZSTD, 3, alice, 1000, W_SEEK_TABLE), (FMT_BGZF, 6, alice[:40000], 0, 0)]
    wants = [write_file(gpu, *job)[1] for job in jobs]
    ins = [upload(gpu, job[2]) for job in jobs]
    gpu.cuda.synchronize()
    stream = gpu.cuda.current_stream()
    errors = []

    def work(k):
        fmt, level, data, unit_bytes, flags = jobs[k]
        try:
            with gpu.cuda.stream(stream):
                for _ in range(10):
                    out, summ = compu_amd.encode_file(fmt, level, ins[k], len(data), unit_bytes, flags)
                    assert out.cpu().numpy().tobytes() == wants[k]
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    compu_amd.trim()  # the writer's slot is released with the others
    for k, job in enumerate(jobs):
        assert write_file(gpu, *job)[1] == wants[k]
    src = gpu.arange(64, dtype=gpu.uint8, device="cuda")
    dst, _, total = compu_amd.pack_units(src, gpu.tensor([8, 0], dtype=gpu.int64, device="cuda"), gpu.tensor([3, 2], dtype=gpu.int32, device="cuda"))
    assert total == 5 and dst.tolist() == [8, 9, 10, 0, 1]
