"""ZIP archives on the GPU: chip_zip_plan against chip_zip_plan_host on every case of tests/zip_cases.py (records bytewise, poisoned
arrays, rows behind max_entries untouched, count-then-fill, the input shifted by 4, 8 and 12 bytes); chip_crc32_batch against
zlib.crc32 around every piece and tile size; chip_zip_decode of every entry against the payloads, selections, too little room,
damage that stays with its entry, entries the plan refuses; two host threads on one stream, chip_trim, a gzip decode on the shared
inflate slot; the one archive above toy size, 70 000 empty entries, whose ZIP64 end record zipfile writes itself.  The host plan is
pinned to the walk of include/compu_hip.h and to zipfile by tests/test_zip_cpu.py.  Without the feature every test here fails at
the missing symbol."""
import ctypes as C
import struct
import threading
import zlib

import numpy as np
import pytest

import zip_cases as Z
import zip_ref as R

pytestmark = pytest.mark.gpu

CASES = Z.all_cases()
IDS = [c.name for c in CASES]
POISON = 0xA7
NEED_INPUT, NEED_OUTPUT, FINISHED = 0, 1, 2
READ_OK, READ_NEED_OUTPUT = 0, 1


def upload(torch, data, shift=0, fill=0xA5):
    """`data` in a device tensor at a 4-byte aligned start `shift` bytes behind a 16-byte aligned one, padded to a multiple of 4;
    the bytes around it hold `fill`."""
    room = shift + (len(data) + 3) // 4 * 4 + 4
    t = torch.full((room,), fill, dtype=torch.uint8, device="cuda")
    if len(data):
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    return t[shift:]


def stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def host_plans():
    """the host plan of every case, made once: (record array, summary tuple)"""
    import compu_amd

    plans = {}
    for c in CASES:
        entries, summ = compu_amd.zip_plan_host(c.data)
        plans[c.name] = (entries, summ.as_tuple())
    return plans


def gpu_plan(torch, lib, d_buf, length, max_entries, room):
    """chip_zip_plan into a poisoned device array of `room` records: (the records as host bytes, summary tuple, the tensor)"""
    from compu_amd.api import ZipPlanSummary, _ZipPlanSummary

    rows = torch.full((room, 56), POISON, dtype=torch.uint8, device="cuda")
    s = _ZipPlanSummary()
    rc = lib.chip_zip_plan(C.c_void_p(d_buf.data_ptr()) if length else None, length, max_entries, C.c_void_p(rows.data_ptr()) if max_entries else None,
                           C.byref(s), stream_ptr(torch))
    assert rc == 0
    return rows.cpu().numpy(), ZipPlanSummary(s).as_tuple(), rows


def assert_plan(torch, lib, data, want, shift=0, max_entries=None, fill=0xA5):
    """the device plan of `data` equals the host plan `want`, bytewise, and nothing behind the rows it owes is written"""
    entries, summ = want
    n = summ[0]
    m = n + 2 if max_entries is None else max_entries
    got, got_summ, rows = gpu_plan(torch, lib, upload(torch, data, shift, fill), len(data), m, max(n, m) + 3)
    assert got_summ == summ
    k = min(n, m)
    assert got[:k].tobytes() == entries[:k].tobytes()
    assert (got[k:] == POISON).all()
    return rows


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_plan_equals_the_host_plan(gpu, case, host_plans):
    import compu_amd

    lib, want = compu_amd.lib(), host_plans[case.name]
    assert want[1] == R.plan(case.data)[1]
    assert_plan(gpu, lib, case.data, want)
    assert_plan(gpu, lib, case.data, want, shift=4, fill=0x00)
    assert_plan(gpu, lib, case.data, want, shift=8, fill=0x50)  # ('P': what lies around the buffer completes no signature)
    assert_plan(gpu, lib, case.data, want, shift=12, fill=0xFF)


def test_plan_counts_then_fills_then_fills_a_part(gpu, host_plans):
    import compu_amd

    lib = compu_amd.lib()
    for name in ("zipfile_mixed", "entry_data_at_every_alignment", "stored_sizes_around_every_power_of_two", "refused_bad_signature_at_entry_last",
                 "accepted_count_smaller_than_the_chain"):
        case, want = Z.by_name(name), host_plans[name]
        n = want[1][0]
        for m in sorted({0, 1, n // 2, max(n - 1, 0), n, n + 1}):
            assert_plan(gpu, lib, case.data, want, max_entries=m)
    case, want = Z.by_name("entry_data_at_every_alignment"), host_plans["entry_data_at_every_alignment"]
    entries, summ = compu_amd.zip_plan(upload(gpu, case.data), len(case.data))
    assert summ.as_tuple() == want[1] and entries.cpu().numpy().tobytes() == want[0].tobytes()
    assert compu_amd.zip_plan(upload(gpu, case.data), len(case.data), max_entries=5)[0].cpu().numpy().tobytes() == want[0][:5].tobytes()
    names = compu_amd.zip_names(entries, summ, case.data[summ.cd_off:summ.cd_off + summ.cd_size])
    assert names[:4] == [b"s00", b"d00", b"s01", b"d01"]
    assert compu_amd.zip_plan(upload(gpu, b""), 0)[1].as_tuple() == (0, 0, 0, 0, 0, 0, 0, R.NO_EOCD, 0)


def test_crc32_batch_equals_zlib(gpu):
    """every size of the list at every offset 0..15, a zero-length range and one of 1 MiB + 1, in one batch; then ranges of many
    pieces, which the fold combines across lanes"""
    import compu_amd

    blob = Z.noise((1 << 20) + 64, 70)
    d = gpu.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    ranges = [((7 * k) % 16 + 16 * (k % 3), n) for k, n in enumerate(Z.SIZES)]
    ranges += [(o, n) for o in range(16) for n in (0, 1, 17, 4097, 65535, 65536, 65537)]
    ranges += [(5, 0), (3, (1 << 20) + 1), (0, 1 << 20), (16, (1 << 20) - 1)]
    off = gpu.tensor([r[0] for r in ranges], dtype=gpu.int64, device="cuda")
    ln = gpu.tensor([r[1] for r in ranges], dtype=gpu.int64, device="cuda")
    got = compu_amd.crc32_batch(d, off, ln)
    gpu.cuda.synchronize()
    want = [zlib.crc32(blob[o:o + n]) for o, n in ranges]
    assert (got.cpu().numpy().view(np.uint32)).tolist() == want
    # 70 pieces and 129 pieces plus a short head: more pieces than lanes, runs of two and three pieces per lane
    big = Z.noise(129 * 65536 + 777, 71)
    d = gpu.from_numpy(np.frombuffer(big, np.uint8).copy()).cuda()
    ranges = [(0, len(big)), (1, 70 * 65536), (13, 64 * 65536 + 1), (2, 65 * 65536), (9, 63 * 65536 + 5), (0, 0)]
    off = gpu.tensor([r[0] for r in ranges], dtype=gpu.int64, device="cuda")
    ln = gpu.tensor([r[1] for r in ranges], dtype=gpu.int64, device="cuda")
    got = compu_amd.crc32_batch(d, off, ln)
    gpu.cuda.synchronize()
    assert (got.cpu().numpy().view(np.uint32)).tolist() == [zlib.crc32(big[o:o + n]) for o, n in ranges]
    assert compu_amd.crc32_batch(d, off[:0], ln[:0]).numel() == 0


def decode(torch, lib, d_buf, length, rows, n_entries, sel, out, out_cap=None):
    """chip_zip_decode into `out` (a device tensor, poisoned by the caller): (out_off list, status list, summary tuple)"""
    from compu_amd.api import ZipDecodeSummary, _ZipDecodeSummary

    n_sel = n_entries if sel is None else len(sel)
    d_sel = None if sel is None else torch.tensor(np.asarray(sel, np.int64).astype(np.uint32).view(np.int32), dtype=torch.int32, device="cuda")
    out_off = torch.full((n_sel + 1,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((n_sel + 1,), -7, dtype=torch.int32, device="cuda")
    s = _ZipDecodeSummary()
    cap = out.numel() if out_cap is None else out_cap
    rc = lib.chip_zip_decode(C.c_void_p(d_buf.data_ptr()), length, C.c_void_p(rows.data_ptr()) if n_entries else None, n_entries, n_sel,
                             C.c_void_p(d_sel.data_ptr()) if d_sel is not None and n_sel else None, C.c_void_p(out.data_ptr()) if cap else None, cap,
                             C.c_void_p(out_off.data_ptr()), C.c_void_p(status.data_ptr()), C.byref(s), stream_ptr(torch))
    assert rc == 0
    assert int(out_off[n_sel]) == -7 and int(status[n_sel]) == -7  # nothing behind the rows
    return out_off[:n_sel].tolist(), status[:n_sel].tolist(), ZipDecodeSummary(s).as_tuple()


def planned(torch, lib, data, want, shift=0):
    d_buf = upload(torch, data, shift)
    n = want[1][0]
    got, summ, rows = gpu_plan(torch, lib, d_buf, len(data), n, n + 1)
    assert summ == want[1]
    return d_buf, rows, n


DECODABLE = [c for c in CASES if c.payloads is not None and R.plan(c.data)[1][7] == R.OK and R.plan(c.data)[1][0] == len(c.payloads)
             and not c.name.startswith("entry_size_2_pow_32")]


@pytest.mark.parametrize("case", DECODABLE, ids=[c.name for c in DECODABLE])
def test_decode_of_every_entry(gpu, case, host_plans):
    """every entry the plan calls OK decodes to its payload with CHIP_FINISHED, the others are skipped with their plan status and
    take no room; the bytes behind total_out stay poisoned"""
    import compu_amd

    lib, want = compu_amd.lib(), host_plans[case.name]
    entries = want[0]
    d_buf, rows, n = planned(gpu, lib, case.data, want, shift=4)
    ok = [int(e["status"]) == R.ENT_OK for e in entries]
    sizes = [len(p) if o else 0 for p, o in zip(case.payloads, ok)]
    total = sum(sizes)
    out = gpu.full((total + 40,), POISON, dtype=gpu.uint8, device="cuda")
    out_off, status, summ = decode(gpu, lib, d_buf, len(case.data), rows, n, None, out[3:], out_cap=total)  # (an odd destination address)
    assert out_off == [sum(sizes[:k]) for k in range(n)]
    assert status == [FINISHED if o else int(e["status"]) for o, e in zip(ok, entries)]
    assert summ == (n, sum(ok), n - sum(ok), ok.index(False) if False in ok else 0, total, READ_OK)
    host = out.cpu().numpy().tobytes()
    assert host[3:3 + total] == b"".join(p for p, o in zip(case.payloads, ok) if o)
    assert host[:3] == bytes([POISON]) * 3 and host[3 + total:] == bytes([POISON]) * 37


def test_selection_in_reverse_with_a_repeat_and_a_bad_index(gpu, host_plans):
    import compu_amd

    lib, case = compu_amd.lib(), Z.by_name("zipfile_mixed")
    d_buf, rows, n = planned(gpu, lib, case.data, host_plans[case.name])
    sel = [4, 3, 2, 99, 2, 1, 0, n, 0xFFFFFFFF, 3]
    pay = [case.payloads[k] if k < n else b"" for k in sel]
    total = sum(len(p) for p in pay)
    out = gpu.full((total + 16,), POISON, dtype=gpu.uint8, device="cuda")
    out_off, status, summ = decode(gpu, lib, d_buf, len(case.data), rows, n, sel, out, out_cap=total)
    assert out_off == [sum(len(p) for p in pay[:k]) for k in range(len(sel))]
    assert status == [FINISHED if k < n else R.ENT_BAD_INDEX for k in sel]
    assert summ == (len(sel), 7, 3, 3, total, READ_OK)
    assert out.cpu().numpy().tobytes() == b"".join(pay) + bytes([POISON]) * 16
    # names and indices through the Python face
    d_out, off, sizes, st, s = compu_amd.zip_decode(d_buf, len(case.data), ["d.txt", 0, b"c.bin"])
    assert d_out.cpu().numpy().tobytes() == case.payloads[3] + case.payloads[0] + case.payloads[2]
    assert sizes.tolist() == [len(case.payloads[3]), len(case.payloads[0]), len(case.payloads[2])] and st.tolist() == [FINISHED] * 3
    assert s.as_tuple() == (3, 3, 0, 0, int(sizes.sum()), READ_OK)
    with pytest.raises(KeyError):
        compu_amd.zip_decode(d_buf, len(case.data), ["nobody"])
    with pytest.raises(ValueError, match="NoEocd"):
        compu_amd.zip_decode(upload(gpu, case.data + b"\0"), len(case.data) + 1)


def test_too_little_room_writes_nothing(gpu, host_plans):
    import compu_amd

    lib, case = compu_amd.lib(), Z.by_name("zipfile_mixed")
    d_buf, rows, n = planned(gpu, lib, case.data, host_plans[case.name])
    total = sum(len(p) for p in case.payloads)
    out = gpu.full((total + 16,), POISON, dtype=gpu.uint8, device="cuda")
    out_off, status, summ = decode(gpu, lib, d_buf, len(case.data), rows, n, None, out, out_cap=total - 1)
    assert summ == (n, 0, 0, 0, total, READ_NEED_OUTPUT)
    assert out_off == [sum(len(p) for p in case.payloads[:k]) for k in range(n)] and status == [NEED_OUTPUT] * n
    assert (out == POISON).all()
    out_off, status, summ = decode(gpu, lib, d_buf, len(case.data), rows, n, None, out, out_cap=0)
    assert summ == (n, 0, 0, 0, total, READ_NEED_OUTPUT) and (out == POISON).all()
    # an entry that would not take part keeps its verdict
    case = Z.by_name("entry_method_12")
    d_buf, rows, n = planned(gpu, lib, case.data, host_plans[case.name])
    total = len(case.payloads[0]) + len(case.payloads[2])
    out_off, status, summ = decode(gpu, lib, d_buf, len(case.data), rows, n, None, out, out_cap=total - 1)
    assert status == [NEED_OUTPUT, R.ENT_UNSUPPORTED, NEED_OUTPUT] and out_off == [0, len(case.payloads[0]), len(case.payloads[0])]
    assert summ == (n, 0, 0, 0, total, READ_NEED_OUTPUT) and (out == POISON).all()


def edited(torch, rows, k, **fields):
    """the plan's records with fields of entry k changed, as a caller may do"""
    import compu_amd

    host = rows.cpu().numpy().reshape(-1).view(compu_amd.zip_entry_dtype()).copy()
    for f, v in fields.items():
        host[k][f] = v
    return torch.from_numpy(host.view(np.uint8).reshape(-1, 56)).cuda()


def test_damage_stays_with_its_entry(gpu, host_plans):
    """a directory CRC flipped; one bit flipped inside a deflated entry's data; a directory size one too small and one too large:
    only that entry's status changes, the neighbours' bytes and statuses stay"""
    import compu_amd

    lib, case = compu_amd.lib(), Z.by_name("zipfile_mixed")
    want = host_plans[case.name]
    n, pay = want[1][0], case.payloads
    total = sum(len(p) for p in pay)
    offs = [sum(len(p) for p in pay[:k]) for k in range(n)]

    def run(data, rows=None, sizes=None):
        d_buf = upload(gpu, data)
        if rows is None:
            rows = gpu_plan(gpu, lib, d_buf, len(data), n, n)[2]
        sizes = sizes or [len(p) for p in pay]
        out = gpu.full((sum(sizes) + 16,), POISON, dtype=gpu.uint8, device="cuda")
        out_off, status, summ = decode(gpu, lib, d_buf, len(data), rows, n, None, out, out_cap=sum(sizes))
        assert out_off == [sum(sizes[:k]) for k in range(n)]
        return out.cpu().numpy().tobytes(), status, summ, rows

    def neighbours_intact(host, sizes, bad):
        at = 0
        for k in range(n):
            if k != bad:
                assert host[at:at + sizes[k]] == pay[k], k
            at += sizes[k]
        assert host[at:] == bytes([POISON]) * 16

    for bad in (0, 3):  # a stored and a deflated entry: the directory's CRC-32 flipped
        host, status, summ, _ = run(Z.flip_directory_crc(case.data, want[1], bad))
        assert status == [R.ENT_BAD_CRC if k == bad else FINISHED for k in range(n)] and summ == (n, n - 1, 1, bad, total, READ_OK)
        assert host[:total] == b"".join(pay)  # (the bytes are all there: only the verdict changed)
    # one bit inside the deflated data of entry 3 (70 000 bytes of text): -3, or BAD_CRC / BAD_SIZE where the flip still decodes
    e3 = want[0][3]
    flipped = bytearray(case.data)
    flipped[int(e3["data_off"]) + int(e3["comp_size"]) // 2] ^= 0x10
    host, status, summ, _ = run(bytes(flipped))
    assert status[3] in (-3, R.ENT_BAD_CRC, R.ENT_BAD_SIZE, NEED_INPUT, NEED_OUTPUT) and status[3] != FINISHED
    assert [s for k, s in enumerate(status) if k != 3] == [FINISHED] * (n - 1) and summ == (n, n - 1, 1, 3, total, READ_OK)
    neighbours_intact(host, [len(p) for p in pay], 3)
    # a stored entry's data changed: BAD_CRC, the bytes are the archive's
    flipped = bytearray(case.data)
    flipped[int(want[0][4]["data_off"]) + 100] ^= 0xFF
    host, status, summ, _ = run(bytes(flipped))
    assert status == [FINISHED] * 4 + [R.ENT_BAD_CRC] and summ[1:4] == (n - 1, 1, 4)
    neighbours_intact(host, [len(p) for p in pay], 4)
    # the directory's size of entry 1 (deflated) one too small: the stream holds more than `size`, CHIP_NEED_OUTPUT
    d_buf = upload(gpu, case.data)
    rows = gpu_plan(gpu, lib, d_buf, len(case.data), n, n)[2]
    sizes = [len(p) for p in pay]
    sizes[1] -= 1
    host, status, summ, _ = run(case.data, edited(gpu, rows, 1, size=sizes[1]), sizes)
    assert status == [FINISHED, NEED_OUTPUT, FINISHED, FINISHED, FINISHED] and summ == (n, n - 1, 1, 1, total - 1, READ_OK)
    neighbours_intact(host, sizes, 1)
    # one too large: the stream finishes one byte short of `size`, which the decode contract answers CHIP_FINISHED with
    # out_len = size - 1: CHIP_ZIPENT_BAD_SIZE
    sizes[1] += 2
    host, status, summ, _ = run(case.data, edited(gpu, rows, 1, size=sizes[1]), sizes)
    assert status == [FINISHED, R.ENT_BAD_SIZE, FINISHED, FINISHED, FINISHED] and summ == (n, n - 1, 1, 1, total + 1, READ_OK)
    neighbours_intact(host, sizes, 1)
    # a stored entry whose edited record no longer satisfies comp_size == size, and one whose data would lie behind the archive:
    # refused before any load, CHIP_ZIPENT_BAD_LOCAL, no room taken
    for fields in (dict(size=len(pay[0]) + 1), dict(data_off=len(case.data) - 10), dict(data_off=2**64 - 1), dict(comp_size=2**64 - 1, size=2**64 - 1)):
        sizes = [0] + [len(p) for p in pay[1:]]
        host, status, summ, _ = run(case.data, edited(gpu, rows, 0, **fields), sizes)
        assert status == [R.ENT_BAD_LOCAL] + [FINISHED] * 4 and summ == (n, n - 1, 1, 0, total - len(pay[0]), READ_OK)
        assert host[:sum(sizes)] == b"".join(pay[1:])


def test_entries_the_plan_refuses_are_skipped(gpu, host_plans):
    import compu_amd

    lib = compu_amd.lib()
    for name in ("entry_method_12", "entry_encrypted_bit_6", "entry_wrong_local_signature", "entry_size_2_pow_32_minus_1_is_too_large",
                 "entry_disk_1", "entry_stored_with_another_size"):
        case, want = Z.by_name(name), host_plans[name]
        d_buf, rows, n = planned(gpu, lib, case.data, want)
        st = [int(e["status"]) for e in want[0]]
        bad = next(k for k, v in enumerate(st) if v != R.ENT_OK)
        pay = [p if v == R.ENT_OK else b"" for p, v in zip(case.payloads, st)]
        total = sum(len(p) for p in pay)
        out = gpu.full((total + 16,), POISON, dtype=gpu.uint8, device="cuda")
        out_off, status, summ = decode(gpu, lib, d_buf, len(case.data), rows, n, None, out, out_cap=total)
        assert status == [FINISHED if v == R.ENT_OK else v for v in st] and summ == (n, n - 1, 1, bad, total, READ_OK), name
        assert out.cpu().numpy().tobytes() == b"".join(pay) + bytes([POISON]) * 16, name


def test_two_host_threads_on_one_stream_trim_and_a_gzip_decode_behind(gpu, host_plans):
    """The slots are locked from their lookup to the last launch: two threads with archives of different sizes on one stream get
    their own answers every time.  chip_trim() releases the slots and the next call allocates again.  A plain
    chip_decode_batch(CHIP_FMT_GZIP) right behind a chip_zip_decode on the same stream shares the inflate slot."""
    import compu_amd

    lib = compu_amd.lib()
    names = ["deflated_sizes", "entry_data_at_every_alignment"]
    cases = [Z.by_name(k) for k in names]
    wants = [host_plans[k] for k in names]
    bufs = [upload(gpu, c.data) for c in cases]
    contents = [b"".join(c.payloads) for c in cases]
    gpu.cuda.synchronize()
    stream = gpu.cuda.current_stream()
    errors = []

    def once(k):
        n = wants[k][1][0]
        got, summ, rows = gpu_plan(gpu, lib, bufs[k], len(cases[k].data), n, n + 1)
        assert summ == wants[k][1] and got[:n].tobytes() == wants[k][0].tobytes()
        out = gpu.full((len(contents[k]) + 8,), POISON, dtype=gpu.uint8, device="cuda")
        out_off, status, s = decode(gpu, lib, bufs[k], len(cases[k].data), rows, n, None, out, out_cap=len(contents[k]))
        assert status == [FINISHED] * n and out.cpu().numpy().tobytes() == contents[k] + bytes([POISON]) * 8

    def work(k):
        try:
            with gpu.cuda.stream(stream):
                for _ in range(6):
                    once(k)
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    compu_amd.trim()
    once(1)
    once(0)
    # gzip members on the inflate slot the zip decode just used, more units than it had
    import gzip

    pays = [Z.text(3000 + k, 80 + k) for k in range(40)]
    members = [gzip.compress(p, 6) for p in pays]
    blob = b"".join(m + bytes(-len(m) % 4) for m in members)
    in_off = np.cumsum([0] + [len(m) + (-len(m) % 4) for m in members[:-1]])
    out_off = np.cumsum([0] + [len(p) for p in pays[:-1]])
    d_in = upload(gpu, blob)
    i64 = lambda a: gpu.tensor(np.asarray(a, np.int64), dtype=gpu.int64, device="cuda")  # noqa: E731
    i32 = lambda a: gpu.tensor(np.asarray(a, np.int32), dtype=gpu.int32, device="cuda")  # noqa: E731
    for _ in range(2):
        once(0)
        out = gpu.zeros(sum(len(p) for p in pays), dtype=gpu.uint8, device="cuda")
        out_len, in_used, status = compu_amd.decode_batch(31, d_in, i64(in_off), i32([len(m) for m in members]), out, i64(out_off),
                                                          i32([len(p) for p in pays]))
        gpu.cuda.synchronize()
        assert (status == FINISHED).all() and out.cpu().numpy().tobytes() == b"".join(pays)


def test_seventy_thousand_empty_entries(gpu):
    """more than 65 535 entries: zipfile writes the ZIP64 end record and the locator itself.  The device plan equals the host plan,
    and the host plan is what zipfile lists."""
    import io
    import zipfile

    import compu_amd

    data = Z.seventy_thousand_empty()
    entries, summ = compu_amd.zip_plan_host(data)
    assert summ.as_tuple()[:3] == (70000, 70000, 0) and summ.status == compu_amd.ZipStatus.Ok and summ.zip64 == 1
    infos = zipfile.ZipFile(io.BytesIO(data)).infolist()
    assert [zi.header_offset for zi in infos] == entries["header_off"].tolist() and len(infos) == 70000
    names = compu_amd.zip_names(entries, summ, data[summ.cd_off:summ.cd_off + summ.cd_size])
    assert names[0] == b"e00000" and names[-1] == b"e69999"
    want = (entries, summ.as_tuple())
    rows = assert_plan(gpu, compu_amd.lib(), data, want, shift=8)
    assert_plan(gpu, compu_amd.lib(), data, want, max_entries=65536)
    # all of them decode to nothing, verified: the CRC-32 of no bytes is 0
    d_buf = upload(gpu, data, 8)
    out = gpu.full((16,), POISON, dtype=gpu.uint8, device="cuda")
    out_off, status, s = decode(gpu, compu_amd.lib(), d_buf, len(data), rows, 70000, None, out, out_cap=0)
    assert s == (70000, 70000, 0, 0, 0, READ_OK) and set(status) == {FINISHED} and set(out_off) == {0} and (out == POISON).all()
