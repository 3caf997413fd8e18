"""Writing ZIP archives on the GPU: chip_zip_assemble against chip_zip_assemble_host on every case of tests/zip_write_cases.py (bytes,
entries, summary, poison around a shifted `out`); chip_zip_write at levels 0, 1 and 6 over contents around the copy tile and the CRC
piece against the reference fed with zlib.crc32 and the streams of a separate chip_encode_batch call, read back by zipfile,
chip_zip_plan and chip_zip_decode; too little room and every bad source on the device; 70 000 entries, which cross the 65 535 count
and make the scans take more than one partial block; an .npz round trip through zip_write_items; the slot reused and trimmed.  The
host assembly is pinned to the rules of include/compu_hip.h and to zipfile by tests/test_zip_write_cpu.py.  Without the feature every
test here fails at the missing symbol."""
import ctypes as C
import io
import zipfile
import zlib

import numpy as np
import pytest

import zip_ref as R
import zip_write_cases as ZC
import zip_write_ref as WR
from test_zip_write_cpu import arrays, run_host
from zip_cases import noise, text

pytestmark = pytest.mark.gpu

CASES = ZC.all_cases()
IDS = [c.name for c in CASES]
POISON = 0xA7
FRONT = 16  # poisoned bytes in front of `out`
FINISHED = 2


def stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(torch, a, dtype=None):
    """a numpy array on the device, reinterpreted as the signed dtype of its width where torch has no unsigned one"""
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    t = torch.from_numpy(np.ascontiguousarray(a.view(signed) if signed else a).copy()).cuda()
    return t


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class Uploaded:
    """a case's arrays in device memory, made once per case"""

    def __init__(self, torch, case):
        import compu_amd

        src, names, content, comp, crc = arrays(case)
        self.case, self.n = case, len(case.sources)
        self.src = dev(torch, src.view(np.uint8).reshape(-1, 32)) if self.n else None
        self.names, self.content, self.crc = dev(torch, names), dev(torch, content), dev(torch, crc) if self.n else None
        self.comp = None
        if comp is not None:
            self.comp = (dev(torch, comp[0]), comp[1], dev(torch, comp[2]) if self.n else torch.zeros(1, dtype=torch.int64, device="cuda"),
                         dev(torch, comp[3]) if self.n else torch.zeros(1, dtype=torch.int32, device="cuda"))
        self.lib = compu_amd.lib()


def run_device(torch, up, out_cap, shift=0, want_entries=True):
    """chip_zip_assemble into a poisoned device buffer, `out` FRONT + shift bytes behind its start and 16 poisoned bytes behind
    out_cap: (the whole buffer as bytes, the entries array as bytes with one poisoned row behind it, summary tuple)"""
    from compu_amd.api import ZipWriteSummary, _ZipWriteSummary

    case, n, comp = up.case, up.n, up.comp
    buf = torch.full((FRONT + shift + out_cap + 16,), POISON, dtype=torch.uint8, device="cuda")
    entries = torch.full((n + 1, 56), POISON, dtype=torch.uint8, device="cuda")
    raw = _ZipWriteSummary()
    rc = up.lib.chip_zip_assemble(
        n, ptr(up.src), ptr(up.names) if len(case.names) else None, len(case.names), ptr(up.content) if case.content_len else None, case.content_len,
        C.c_void_p(comp[0].data_ptr()) if comp else None, comp[1] if comp else 0, C.c_void_p(comp[2].data_ptr()) if comp else None,
        C.c_void_p(comp[3].data_ptr()) if comp else None, ptr(up.crc), case.flags, C.c_void_p(buf.data_ptr() + FRONT + shift) if out_cap else None, out_cap,
        C.c_void_p(entries.data_ptr()) if want_entries else None, C.byref(raw), stream_ptr(torch))
    assert rc == 0
    return buf.cpu().numpy().tobytes(), entries.cpu().numpy().tobytes(), ZipWriteSummary(raw).as_tuple()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_assembly_equals_the_host_assembly(gpu, case):
    host_buf, rows, summ, host_rows = run_host(case)
    assert summ == case.want()[2]
    up = Uploaded(gpu, case)
    n = len(case.sources)
    row_poison = bytes([POISON]) * 56
    if summ[7] != WR.OK:  # a bad source, or an arithmetic case run without room
        buf, ent, got = run_device(gpu, up, 0)
        assert got == summ and buf == bytes([POISON]) * len(buf)
        assert ent == (row_poison * (n + 1) if summ[7] == WR.BAD_SOURCE else host_rows.tobytes() + row_poison)
        if summ[7] == WR.BAD_SOURCE:  # with room as well: nothing but the summary
            buf, ent, got = run_device(gpu, up, 4096)
            assert got == summ and buf == bytes([POISON]) * len(buf) and ent == row_poison * (n + 1)
        return
    want = host_buf[:summ[2]]
    for shift in (0, 1, 7, 15, 16):
        buf, ent, got = run_device(gpu, up, summ[2], shift)
        assert got == summ and ent == host_rows.tobytes() + row_poison
        assert buf == bytes([POISON]) * (FRONT + shift) + want + bytes([POISON]) * 16, shift
    # more room than needed, and no entries array
    buf, ent, got = run_device(gpu, up, summ[2] + 5, 3, want_entries=False)
    assert got == summ and ent == row_poison * (n + 1) and buf == bytes([POISON]) * (FRONT + 3) + want + bytes([POISON]) * 21
    # too little room: the exact length, the entries, nothing written
    for cap in (summ[2] - 1, 0):
        buf, ent, got = run_device(gpu, up, cap)
        assert got == summ[:7] + (WR.NEED_OUTPUT, summ[8]) and ent == host_rows.tobytes() + row_poison and buf == bytes([POISON]) * len(buf)


@pytest.mark.parametrize("name", ["mixed_force_utf8", "sizes_around_a_tile", "name_of_65535_bytes", "no_comp_arrays", "count_65535"])
def test_one_launch_per_source_buffer_gives_the_same_archive(gpu, name, monkeypatch):
    """the copy's other shape (CHIP_ZIPW_COPY=launches, what tools/time_zip_write.py measures against the default)"""
    case = ZC.by_name(name)
    host_buf, rows, summ, host_rows = run_host(case)
    monkeypatch.setenv("CHIP_ZIPW_COPY", "launches")
    up = Uploaded(gpu, case)
    for shift in (0, 7):
        buf, ent, got = run_device(gpu, up, summ[2], shift)
        assert got == summ and buf == bytes([POISON]) * (FRONT + shift) + host_buf[:summ[2]] + bytes([POISON]) * 16


SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 65535, 65536, 65537]


@pytest.fixture(scope="module")
def boundary_contents():
    """every size once as text and once as random bytes, the data offsets at alignments 0..3: (sources, names, content, payloads)"""
    names, content, sources, payloads = bytearray(), bytearray(), [], []
    for k, (size, kind) in enumerate((s, kind) for s in SIZES for kind in ("t", "r")):
        pay = text(size, 100 + k) if kind == "t" else noise(size, 100 + k)
        while len(content) % 4 != k % 4:
            content += b"\xEE"
        nm = b"%s%d" % (kind.encode(), size)
        sources.append((len(content), size, len(names), len(nm), WR.DEFLATE, 0x6000 + k, 0x5A21))
        names += nm
        content += pay
        payloads.append(pay)
    content += bytes(-len(content) % 4)
    return sources, bytes(names), bytes(content), payloads


def device_streams(torch, sources, d_content, level):
    """the streams a separate chip_encode_batch(CHIP_FMT_DEFLATE, level) call gives for the deflate-eligible entries: the comp triple"""
    import compu_amd

    units = [(i, s) for i, s in enumerate(sources) if s[4] == WR.DEFLATE and 0 < s[1] <= (1 << 30)]
    caps = [(compu_amd.encode_bound(-15, s[1]) + 15) // 16 * 16 for _, s in units]
    offs = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.int64) if units else np.zeros(0, np.int64)
    area = torch.zeros(int(sum(caps)) + 16, dtype=torch.uint8, device="cuda")
    i64 = lambda a: torch.tensor(np.asarray(a, np.int64), dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda a: torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device="cuda")  # noqa: E731
    streams = [None] * len(sources)
    if units:
        out_len, status = compu_amd.encode_batch(-15, level, d_content, i64([s[0] for _, s in units]), i32([s[1] for _, s in units]), area, i64(offs), i32(caps))
        torch.cuda.synchronize()
        assert (status == FINISHED).all()
        host = area.cpu().numpy().tobytes()
        for (i, _), o, ln in zip(units, offs.tolist(), out_len.tolist()):
            streams[i] = host[o:o + ln]
    return WR.pack_streams(streams)


def write_on_device(torch, sources, names, d_content, content_len, level, flags, out_cap, shift=0):
    """chip_zip_write into poisoned buffers: (buffer bytes, entries bytes, summary tuple, the archive's tensor, the entries' tensor)"""
    import compu_amd
    from compu_amd.api import ZipWriteSummary, _ZipWriteSummary

    n = len(sources)
    src = np.array(sources, dtype=compu_amd.zip_source_dtype()) if n else np.zeros(0, compu_amd.zip_source_dtype())
    d_src = dev(torch, src.view(np.uint8).reshape(-1, 32)) if n else None
    d_names = dev(torch, np.frombuffer(names, np.uint8)) if names else None
    buf = torch.full((FRONT + shift + out_cap + 16,), POISON, dtype=torch.uint8, device="cuda")
    entries = torch.full((n + 1, 56), POISON, dtype=torch.uint8, device="cuda")
    raw = _ZipWriteSummary()
    rc = compu_amd.lib().chip_zip_write(level, flags, n, ptr(d_src), ptr(d_names), len(names), ptr(d_content) if content_len else None, content_len,
                                        C.c_void_p(buf.data_ptr() + FRONT + shift) if out_cap else None, out_cap, C.c_void_p(entries.data_ptr()),
                                        C.byref(raw), stream_ptr(torch))
    assert rc == 0
    return buf.cpu().numpy().tobytes(), entries.cpu().numpy().tobytes(), ZipWriteSummary(raw).as_tuple(), buf[FRONT + shift:], entries[:n]


@pytest.mark.parametrize("level", [0, 1, 6])
def test_write_around_every_boundary(gpu, level, boundary_contents):
    import compu_amd

    sources, names, content, payloads = boundary_contents
    n = len(sources)
    d_content = dev(gpu, np.frombuffer(content, np.uint8))
    comp = device_streams(gpu, sources, d_content, level)
    crcs = [zlib.crc32(p) for p in payloads]
    for flags, shift in ((0, 0), (WR.ZW_UTF8, 5), (WR.ZW_ZIP64, 16)):
        want, rows, summ = WR.assemble(sources, names, content, comp, crcs, flags)
        room = compu_amd.zip_write_bound(n, len(names), sum(len(p) for p in payloads))
        assert room >= summ[2]
        buf, ent, got, d_arch, d_ent = write_on_device(gpu, sources, names, d_content, len(content), level, flags, room, shift)
        assert got == summ
        assert buf == bytes([POISON]) * (FRONT + shift) + want + bytes([POISON]) * (room - summ[2] + 16)
        dt = compu_amd.zip_entry_dtype()
        assert [tuple(int(v) for v in e) for e in np.frombuffer(ent[:56 * n], dt).tolist()] == rows and ent[56 * n:] == bytes([POISON]) * 56
        if level == 0:
            assert summ[1] == 0 and all(r[7] == 0 for r in rows)  # stored blocks never shrink
        else:
            assert summ[1] == sum(1 for s, r in zip(sources, rows) if r[2] < s[1]) >= 6  # at least the text entries of 4 095 bytes and more
    # read back: zipfile, the device plan, the device decode (of the last archive, the ZIP64 form, and of the plain one)
    for flags in (WR.ZW_ZIP64, 0):
        want, rows, summ = WR.assemble(sources, names, content, comp, crcs, flags)
        buf, ent, got, d_arch, d_ent = write_on_device(gpu, sources, names, d_content, len(content), level, flags, (summ[2] + 3) // 4 * 4)
        zf = zipfile.ZipFile(io.BytesIO(want))
        assert zf.testzip() is None and [zf.open(zi).read() for zi in zf.infolist()] == payloads
        assert [zi.orig_filename.encode() for zi in zf.infolist()] == [names[s[2]:s[2] + s[3]] for s in sources]
        archive = gpu.zeros((summ[2] + 3) // 4 * 4 + 4, dtype=gpu.uint8, device="cuda")  # (4-byte aligned and padded for the plan)
        archive[:summ[2]] = d_arch[:summ[2]]
        planned, psumm = compu_amd.zip_plan(archive, summ[2])
        assert psumm.as_tuple() == (n, n, sum(len(p) for p in payloads), summ[3], summ[4], summ[5], 0, R.OK, summ[8])
        assert planned.cpu().numpy().tobytes() == ent[:56 * n]
        out, out_off, sizes, status, dsumm = compu_amd.zip_decode(archive, summ[2])
        assert status.tolist() == [FINISHED] * n and out.cpu().numpy().tobytes() == b"".join(payloads)


def test_too_little_room_and_bad_sources_write_nothing(gpu, boundary_contents):
    """NEED_OUTPUT and each BAD_SOURCE rule through chip_zip_write leave out and entries poisoned; the lowest bad index wins with the
    bad records 3 000 entries apart, in different workgroups"""
    sources, names, content, payloads = boundary_contents
    n = len(sources)
    d_content = dev(gpu, np.frombuffer(content, np.uint8))
    comp = device_streams(gpu, sources, d_content, 6)
    want, rows, summ = WR.assemble(sources, names, content, comp, [zlib.crc32(p) for p in payloads], 0)
    for cap in (summ[2] - 1, 0):
        buf, ent, got, _, _ = write_on_device(gpu, sources, names, d_content, len(content), 6, 0, cap)
        assert got == summ[:7] + (WR.NEED_OUTPUT, 0) and buf == bytes([POISON]) * len(buf)
        assert ent[56 * n:] == bytes([POISON]) * 56 and ent[:56 * n] != bytes([POISON]) * 56 * n  # (answered: compared in the test above)
    edits = [(4, 3), (4, 0xFFFF), (0, len(content) - 2), (0, len(content) + 1), (0, 2**64 - 1), (1, 2**64 - 1), (2, len(names) - 1), (2, 2**64 - 1)]
    for field, value in edits:
        for at in (0, 7, n - 1):
            s = list(sources)
            row = list(s[at])
            row[field] = value
            if field == 0:
                row[1] = max(row[1], 3)
            s[at] = tuple(row)
            buf, ent, got, _, _ = write_on_device(gpu, s, names, d_content, len(content), 6, 0, summ[2] + 100)
            assert got == (n, 0, 0, 0, 0, 0, at, WR.BAD_SOURCE, 0), (field, value, at)
            assert buf == bytes([POISON]) * len(buf) and ent == bytes([POISON]) * 56 * (n + 1)
    # 7 000 small entries, bad records at 4 500 and 1 500: different workgroups of every kernel, the lower one wins
    many = 7000
    names = b"".join(b"f%04d" % k for k in range(many))
    blob = text(4096, 9)
    d_blob = dev(gpu, np.frombuffer(blob, np.uint8))
    s = [(k % 100, k % 50, 5 * k, 5, WR.DEFLATE if k % 2 else WR.STORE, 0, 0x21) for k in range(many)]
    s[4500] = s[4500][:4] + (5,) + s[4500][5:]
    for lower in (1500, 4499):
        t = list(s)
        t[lower] = (4000, 97) + t[lower][2:]
        buf, ent, got, _, _ = write_on_device(gpu, t, names, d_blob, len(blob), 1, 0, 1 << 20)
        assert got == (many, 0, 0, 0, 0, 0, lower, WR.BAD_SOURCE, 0) and buf == bytes([POISON]) * len(buf) and ent == bytes([POISON]) * 56 * (many + 1)
    # the same through chip_zip_assemble, the stream rule included
    case = ZC.by_name("bad_stream_one_past_the_end")
    assert run_device(gpu, Uploaded(gpu, case), 4096)[2] == (4, 0, 0, 0, 0, 0, 3, WR.BAD_SOURCE, 0)


def test_seventy_thousand_entries(gpu):
    """the one archive above toy size: it crosses the 65 535 count, so it has ZIP64 end records, and the scans take more than one
    partial block"""
    sources, names, content, crcs = ZC.seventy_thousand()
    n = len(sources)
    want, rows, summ = WR.assemble(sources, names, content, None, crcs, 0)  # (an entry of 0 or 1 bytes never shrinks: all stored)
    assert summ[8] == 1 and summ[1] == 0 and want[-98:-94] == b"PK\x06\x06"
    d_content = dev(gpu, np.frombuffer(content, np.uint8))
    buf, ent, got, d_arch, _ = write_on_device(gpu, sources, names, d_content, len(content), 6, 0, summ[2], shift=9)
    assert got == summ
    assert buf == bytes([POISON]) * (FRONT + 9) + want + bytes([POISON]) * 16
    import compu_amd

    assert [tuple(int(v) for v in e) for e in np.frombuffer(ent[:56 * n], compu_amd.zip_entry_dtype()).tolist()] == rows
    infos = zipfile.ZipFile(io.BytesIO(buf[FRONT + 9:FRONT + 9 + summ[2]])).infolist()
    assert len(infos) == 70000 and infos[0].filename == "e00000" and infos[-1].filename == "e69999"
    assert [zi.file_size for zi in infos[:6]] == [0, 1, 0, 1, 0, 1]


def test_npz_round_trip(gpu):
    import compu_amd

    arrays_ = {"weights": np.arange(6000, dtype=np.float32).reshape(60, 100) / 7, "ids": np.arange(-50, 50, dtype=np.int64),
               "mask": (np.arange(777) % 3 == 0)}
    items = []
    for k, (name, a) in enumerate(arrays_.items()):
        f = io.BytesIO()
        np.lib.format.write_array(f, a, allow_pickle=False)
        blob = f.getvalue()
        # one content as host bytes, the others as device tensors
        items.append((name + ".npy", blob if k == 0 else gpu.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()))
    archive, entries, summ = compu_amd.zip_write_items(items, level=6)
    assert summ.status == compu_amd.ZipWriteStatus.Ok and summ.n_entries == 3 and summ.n_deflated >= 2 and archive.numel() == summ.out_len
    data = archive.cpu().numpy().tobytes()
    loaded = np.load(io.BytesIO(data))
    assert sorted(loaded.files) == sorted(arrays_)
    for name, a in arrays_.items():
        assert loaded[name].dtype == a.dtype and np.array_equal(loaded[name], a)
    zf = zipfile.ZipFile(io.BytesIO(data))
    assert all(zi.flag_bits & 0x800 for zi in zf.infolist()) and zf.testzip() is None
    # bytes names: no UTF-8 flag; an empty list: the end record alone
    archive, _, summ = compu_amd.zip_write_items([(b"raw", b"abc" * 100)], level=1)
    zf = zipfile.ZipFile(io.BytesIO(archive.cpu().numpy().tobytes()))
    assert zf.infolist()[0].flag_bits == 0 and zf.read("raw") == b"abc" * 100
    archive, entries, summ = compu_amd.zip_write_items([])
    assert archive.cpu().numpy().tobytes() == b"PK\x05\x06" + bytes(18) and entries.shape[0] == 0


def test_the_slot_is_reused_and_trimmed(gpu, boundary_contents):
    """two calls on one stream reuse the slot (a smaller batch behind a larger one, and back); chip_trim() releases it and the next
    call allocates again; a chip_zip_decode still works afterwards"""
    import compu_amd

    sources, names, content, payloads = boundary_contents
    d_content = dev(gpu, np.frombuffer(content, np.uint8))
    d_src = dev(gpu, np.array(sources, dtype=compu_amd.zip_source_dtype()).view(np.uint8).reshape(-1, 32))
    d_names = dev(gpu, np.frombuffer(names, np.uint8))
    first, _, s1 = compu_amd.zip_write(d_src, d_names, d_content, level=6)
    small, _, s2 = compu_amd.zip_write(d_src[:5].contiguous(), d_names, d_content, level=6)
    again, _, s3 = compu_amd.zip_write(d_src, d_names, d_content, level=6)
    assert s1.as_tuple() == s3.as_tuple() and s2.n_entries == 5 and first.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    compu_amd.trim()
    after, entries, s4 = compu_amd.zip_write(d_src, d_names, d_content, level=6)
    assert s4.as_tuple() == s1.as_tuple() and after.cpu().numpy().tobytes() == first.cpu().numpy().tobytes()
    # the assemble face: every entry stored from the same tensors, the CRC-32 from crc32_batch
    off = gpu.tensor([s[0] for s in sources], dtype=gpu.int64, device="cuda")
    ln = gpu.tensor([s[1] for s in sources], dtype=gpu.int64, device="cuda")
    stored, _, s5 = compu_amd.zip_assemble(d_src, d_names, d_content, compu_amd.crc32_batch(d_content, off, ln))
    zf = zipfile.ZipFile(io.BytesIO(stored.cpu().numpy().tobytes()))
    assert s5.n_deflated == 0 and zf.testzip() is None and [zf.open(zi).read() for zi in zf.infolist()] == payloads
    compu_amd.trim()
    archive = gpu.zeros((s4.out_len + 3) // 4 * 4 + 4, dtype=gpu.uint8, device="cuda")
    archive[:s4.out_len] = after
    out, out_off, sizes, status, dsumm = compu_amd.zip_decode(archive, s4.out_len, ["t4097", "r65537"])
    assert status.tolist() == [FINISHED] * 2
    assert out.cpu().numpy().tobytes() == payloads[SIZES.index(4097) * 2] + payloads[SIZES.index(65537) * 2 + 1]
