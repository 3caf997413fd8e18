"""Writing tar images without a GPU: chip_tar_write_host against the Python restatement of the rules (tests/tar_write_ref.py) on every
case of tests/tar_write_cases.py -- bytes, entries, summary, the bytes around the image, sixteen alignments of `out`, one byte too
little room and none; tarfile, chip_tar_plan_host and the reference walk (tests/tar_ref.py) as readers of what it wrote;
chip_tar_write_bound; the layouts and the header's numbers; the argument refusals of both calls, which answer before a device is
looked for; and the assembly (compu_amd/csrc/tar_write_core.h) in a stand-alone program under the address and undefined-behaviour
sanitizers.  Without the feature every test here fails at the missing symbol."""
import ctypes as C
import io
import os
import struct
import subprocess
import tarfile

import numpy as np
import pytest

import tar_ref as R
import tar_write_cases as TC
import tar_write_ref as WR

CASES = TC.all_cases()
IDS = [c.name for c in CASES]
READABLE = [c for c in CASES if c.members is not None and not c.arith]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA7
INVALID = -101


def arrays(case):
    """the case as the numpy arrays the C call takes"""
    import compu_amd

    src = np.array(case.sources, dtype=compu_amd.tar_source_dtype()) if case.sources else np.zeros(0, compu_amd.tar_source_dtype())
    u8 = lambda b: np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(1, np.uint8)  # noqa: E731
    return src, u8(case.names), u8(case.content)


def run_host(case, out_cap=None, shift=0, want_entries=True):
    """chip_tar_write_host into a poisoned buffer, `out` `shift` bytes behind its start and 16 poisoned bytes behind out_cap: (the
    whole buffer as bytes, rows, summary tuple, the rows' bytes).  out_cap None: the room the reference states (0 for an arithmetic
    case or a bad one)."""
    import compu_amd
    from compu_amd.api import TarWriteSummary, _TarWriteSummary

    src, names, content = arrays(case)
    if out_cap is None:
        out_cap = 0 if case.arith else case.want()[2][2]
    n = len(case.sources)
    buf = np.full(shift + out_cap + 16, POISON, np.uint8)
    entries = np.full(n + 1, POISON, np.uint8).repeat(72).view(compu_amd.tar_entry_dtype())
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    raw = _TarWriteSummary()
    rc = compu_amd.lib().chip_tar_write_host(
        n, p(src) if n else None, p(names) if len(case.names) else None, len(case.names), p(content) if case.content_len else None, case.content_len,
        case.flags, case.record_bytes, C.c_void_p(buf.ctypes.data + shift) if out_cap else None, out_cap, p(entries) if want_entries else None, C.byref(raw))
    assert rc == 0
    assert entries[n:].tobytes() == bytes([POISON]) * 72  # nothing behind the rows
    return buf.tobytes(), [tuple(int(v) for v in e) for e in entries[:n].tolist()], TarWriteSummary(raw).as_tuple(), entries[:n].tobytes()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_image_equals_the_reference(case):
    """bytes, entries and summary; the bytes behind out_len intact; `out` at 16 alignments; one byte too little room and none; the
    bound"""
    import compu_amd

    want_bytes, want_rows, want_summ = case.want()
    buf, rows, summ, raw_rows = run_host(case)
    assert summ == want_summ
    n = len(case.sources)
    if case.bad or case.arith:
        assert buf == bytes([POISON]) * len(buf)
        if case.bad:  # nothing but the summary is written
            assert raw_rows == bytes([POISON]) * 72 * n
            assert summ == (n, 0, 0, 0, 0, summ[5], WR.BAD_SOURCE)
        else:
            assert rows == want_rows and summ[6] == WR.NEED_OUTPUT
            assert compu_amd.tar_write_bound(n, sum(s[5] + s[6] for s in case.sources), sum(s[1] for s in case.sources), case.record_bytes) >= summ[2]
        return
    assert rows == want_rows and summ[6] == WR.OK
    assert buf == want_bytes + bytes([POISON]) * 16
    assert compu_amd.tar_write_bound(n, sum(s[5] + s[6] for s in case.sources), sum(s[1] for s in case.sources), case.record_bytes) >= summ[2]
    if len(want_bytes) <= (1 << 18):
        for shift in range(1, 16):
            buf, rows2, summ2, _ = run_host(case, shift=shift)
            assert buf == bytes([POISON]) * shift + want_bytes + bytes([POISON]) * 16 and rows2 == rows and summ2 == summ
    # one byte too little, and no room at all: NEED_OUTPUT, the exact length, the entries, nothing written
    for cap in (summ[2] - 1, 0):
        buf, rows2, summ2, _ = run_host(case, out_cap=cap)
        assert summ2 == summ[:6] + (WR.NEED_OUTPUT,) and rows2 == rows and buf == bytes([POISON]) * len(buf)
    assert run_host(case, want_entries=False)[0] == want_bytes + bytes([POISON]) * 16


@pytest.mark.parametrize("case", READABLE, ids=[c.name for c in READABLE])
def test_tarfile_and_the_plan_read_what_was_written(case):
    """tarfile: names, link names, types, sizes, mode, mtime, uid, gid, contents; chip_tar_plan_host of the image gives the answered
    entries bytewise with zero_blocks 2, and the reference walk agrees"""
    import compu_amd

    buf, rows, summ, raw_rows = run_host(case)
    data = buf[:summ[2]]
    assert len(data) % (case.record_bytes or 10240) == 0 and data[summ[3]:] == bytes(summ[2] - summ[3]) and summ[2] - summ[3] >= 1024
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:", encoding="utf-8", errors="surrogateescape") as tf:
        infos = tf.getmembers()
        assert len(infos) == len(case.members)
        raw = lambda s: s.encode("utf-8", "surrogateescape")  # noqa: E731
        for ti, m, row in zip(infos, case.members, rows):
            assert raw(ti.name) == (m.name.rstrip(b"/") if ti.isdir() else m.name), (ti.name, m.name)  # (tarfile strips a directory's '/')
            assert raw(ti.linkname) == m.link
            assert ti.type == bytes([m.typeflag]) and ti.size == len(m.data) and ti.mode == m.mode and ti.mtime == m.mtime
            assert (ti.uid, ti.gid, ti.offset, ti.offset_data) == (m.uid, m.gid, row[0], row[2])
            if ti.isreg() or m.typeflag == ord("7"):
                assert tf.extractfile(ti).read() == m.data
    planned, psumm = compu_amd.tar_plan_host(data)
    assert planned.tobytes() == raw_rows
    n = len(case.members)
    assert psumm.as_tuple() == (n, 0, sum(len(m.data) for m in case.members), summ[3], summ[3], R.OK, 2)
    ref_rows, ref_summ = R.plan(data)
    assert ref_rows == rows and ref_summ == psumm.as_tuple()
    assert R.names(ref_rows, data) == [m.name for m in case.members]
    assert compu_amd.tar_names(planned, data) == [m.name for m in case.members]


def test_what_the_cases_pin():
    """the reference's answers the cases are named for"""
    w = lambda name: TC.by_name(name).want()  # noqa: E731
    rows = w("split_pax")[1]
    # (prefix_len, name_len, flags) of the eight members of the split set
    assert [(r[10], r[7], r[12]) for r in rows] == [(155, 100, 0), (0, 207, 2), (0, 152, 2), (0, 121, 2), (101, 50, 0), (119, 1, 0), (0, 101, 2), (1, 100, 0)]
    assert all(r[10] == 0 for r in w("split_gnu")[1]) and [r[12] for r in w("split_gnu")[1]] == [1] * 8
    assert [r[12] for r in w("links_pax")[1]] == [0, 0, 8, 8, 2 | 8] and [r[12] for r in w("links_gnu")[1]] == [0, 0, 4, 4, 1 | 4]
    assert [r[12] for r in w("sizes_pax_force")[1]] == [16] * 9 and [r[12] for r in w("sizes_gnu_force")[1]] == [32] * 9
    assert [r[12] for r in w("name_lengths_pax")[1]] == [0, 0, 0, 0, 2, 2, 2, 2]  # (255, 256: no '/' in the window of the split)
    assert [r[12] for r in w("name_lengths_no_slash_pax")[1]] == [0, 2, 2, 2, 2]
    assert w("empty")[0] == bytes(10240) and w("empty_record_512")[0] == bytes(1024) and len(w("empty_record_1048576")[0]) == 1 << 20
    assert w("one_pax")[2] == (1, 0, 10240, 1024, 6, 0, WR.OK) and w("one_empty_gnu_force")[2][:4] == (1, 0, 10240, 512)
    # a record's length never has ten bytes: 9 for a one-digit size, 11 for a two-digit one; 999 -> 1001 and 9999 -> 10001 for a path
    assert WR.record(b"size", b"5") == b"9 size=5\n" and WR.record(b"size", b"50") == b"11 size=50\n"
    assert [len(WR.record(b"path", b"n" * n)) for n in (989, 990, 991, 9988, 9989)] == [999, 1001, 1002, 9999, 10001]
    assert [len(WR.record(b"linkpath", b"n" * n)) for n in (985, 986, 9984, 9985)] == [999, 1001, 9999, 10001]
    for tag in ("pax", "gnu"):
        big, below = w(f"arith_size_8_pow_11_{tag}"), w(f"arith_size_8_pow_11_minus_1_{tag}")
        assert big[1][0][12] == (16 if tag == "pax" else 32) and below[1][0][12] == 0 and big[2][6] == WR.NEED_OUTPUT
        assert big[1][0][1] == (1024 if tag == "pax" else 0) and below[1][0][1] == 0
        assert w(f"arith_2_pow_40_{tag}")[2][4] == (1 << 40) + 513
    assert w("bad_second_mode")[2][5:] == (1, WR.BAD_SOURCE) and w("bad_mode")[2][5] == 1 and w("bad_first_and_last")[2][5] == 0


def test_layouts_and_the_header():
    import compu_amd
    from compu_amd.api import _TarSource, _TarWriteSummary

    assert C.sizeof(_TarSource) == 64 == compu_amd.tar_source_dtype().itemsize and C.sizeof(_TarWriteSummary) == 56
    text = open(os.path.join(ROOT, "include", "compu_hip.h")).read()
    assert "CHIP_TW_GNU = 1, CHIP_TW_FORCE_EXT = 2" in text and "CHIP_TARW_OK = 0, CHIP_TARW_NEED_OUTPUT = 1, CHIP_TARW_BAD_SOURCE = 2" in text
    assert "#define CHIP_TARW_NAME_MAX 65535u" in text
    assert (compu_amd.TW_GNU, compu_amd.TW_FORCE_EXT, compu_amd.TARW_NAME_MAX) == (1, 2, 65535) and [int(v) for v in compu_amd.TarWriteStatus] == [0, 1, 2]
    b = compu_amd.tar_write_bound
    assert b(0, 0, 0) == 10240 and b(0, 0, 0, 512) == 1024 and b(3, 10, 1000, 512) == 1000 + 20 + 9216 + 1024 + 512 - (1000 + 20 + 9216 + 1024) % 512
    assert b(1, 0, 0, 100) == 0 and b(1, 0, 0, (1 << 20) + 512) == 0 and b(1, 0, 0, 1 << 20) == 1 << 20
    assert b(1, 2**63, 0) == 0 and b(2**62, 0, 0) == 0 and b(1, 0, 2**64 - 4096) == 0
    for args in ((2**31 - 1, 2**40, 2**40, 0), (5, 7, 9, 512), (1, 0, 2**63, 1 << 20)):
        assert b(*args) == WR.bound(*args)
    # the worst group the constant has to cover: two names of 101 bytes under GNU and a size that is 1 above a block.  A constant of
    # 2560 would not be enough for it.
    c = TC.lay_out("worst", [TC.Member(b"n" * 101, b"x" * 513, link=b"l" * 101, typeflag="0")] * 40, WR.TW_GNU, 512)
    assert 40 * (513 + 404 + 2560) + 1024 + 511 < c.want()[2][2] == 40 * (5 * 512 + 1024) + 1024 <= b(40, 40 * 202, 40 * 513, 512)
    assert run_host(c)[2] == c.want()[2]


def test_the_python_face_on_the_host():
    import compu_amd

    case = TC.by_name("split_pax")
    src, _, _ = arrays(case)
    data, entries, summ = compu_amd.tar_write_host(src, case.names, case.content, flags=case.flags)
    want = case.want()
    assert data == want[0] and summ.as_tuple() == want[2] and [tuple(int(v) for v in e) for e in entries.tolist()] == want[1]
    data, entries, summ = compu_amd.tar_write_host(src, case.names, case.content, out_cap=10)
    assert data == b"" and summ.status == compu_amd.TarWriteStatus.NeedOutput and summ.out_len == want[2][2]
    case = TC.by_name("arith_2_pow_40_gnu")
    src, _, _ = arrays(case)
    data, entries, summ = compu_amd.tar_write_host(src, case.names, b"", flags=case.flags, out_cap=0, content_len=case.content_len)
    assert summ.as_tuple() == case.want()[2] and int(entries[0]["size"]) == 1 << 40 and int(entries[0]["flags"]) == 32


def test_argument_refusals_need_no_device():
    import compu_amd
    from compu_amd.api import _TarWriteSummary

    lib = compu_amd.lib()
    ws = _TarWriteSummary()
    p = C.c_void_p(4096)  # never read: every call below is refused at its arguments
    S = C.byref(ws)
    # n, src, names, names_len, content, content_len, flags, record_bytes, out, out_cap, entries, summary
    good = [3, p, p, 10, p, 100, 0, 0, p, 1000, p, S]

    def refused(call, base, k, v, *more):
        a = list(base)
        a[k] = v
        for kk, vv in zip(more[::2], more[1::2]):
            a[kk] = vv
        return call(*a) == INVALID

    for call, args in ((lib.chip_tar_write_host, good), (lib.chip_tar_write, good + [None])):
        assert refused(call, args, 11, None) and refused(call, args, 1, None) and refused(call, args, 2, None) and refused(call, args, 4, None)
        assert refused(call, args, 8, None)
        assert refused(call, args, 0, 1 << 31) and refused(call, args, 6, 4) and refused(call, args, 6, 0x80000000)
        assert refused(call, args, 7, 511) and refused(call, args, 7, 513) and refused(call, args, 7, (1 << 20) + 512) and refused(call, args, 7, 1)
        assert refused(call, args, 5, 1 << 62) and refused(call, args, 5, (1 << 64) - 1) and refused(call, args, 0, (1 << 31) - 1, 5, 1 << 40)
    # n == 0 needs no pointer, and with too little room no device: the host answers
    for call, tail in ((lib.chip_tar_write_host, []), (lib.chip_tar_write, [None])):
        for flags, rb, want in ((0, 0, 10240), (3, 512, 1024), (1, 1 << 20, 1 << 20)):
            ws.status = 77
            assert call(0, None, None, 0, None, 0, flags, rb, None, 0, None, S, *tail) == 0
            assert (ws.n_entries, ws.n_ext, ws.out_len, ws.end_off, ws.total_size, ws.bad_index, ws.status) == (0, 0, want, 0, 0, 0, WR.NEED_OUTPUT)
            assert call(0, None, None, 0, None, 0, flags, rb, p, want - 1, None, S, *tail) == 0 and ws.status == WR.NEED_OUTPUT


SRC_DT = np.dtype([("data_off", "<u8"), ("size", "<u8"), ("name_off", "<u8"), ("link_off", "<u8"), ("mtime", "<i8"), ("name_len", "<u4"), ("link_len", "<u4"),
                   ("mode", "<u4"), ("uid", "<u4"), ("gid", "<u4"), ("typeflag", "u1"), ("pad", "u1", (3,))])
ENT_DT = np.dtype([("group_off", "<u8"), ("header_off", "<u8"), ("data_off", "<u8"), ("size", "<u8"), ("name_off", "<u8"), ("link_off", "<u8"),
                   ("mtime", "<i8"), ("name_len", "<u4"), ("link_len", "<u4"), ("mode", "<u4"), ("prefix_len", "<u2"), ("typeflag", "u1"), ("flags", "u1")])


def test_assembly_under_the_sanitizers(tmp_path):
    """compu_amd/csrc/tar_write_core.h in a stand-alone program built with the address and undefined-behaviour sanitizers: every case
    from exact-size heap buffers against the reference's files, the plan of what it wrote, one byte too little room"""
    exe = str(tmp_path / "test_tar_write")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_tar_write.cpp")])
    for k, c in enumerate(CASES):
        data, rows, summ = c.want()
        n = len(c.sources)
        head = struct.pack("<8Q", n, len(c.names), len(c.content), c.content_len, c.flags, c.record_bytes, int(c.arith), 0)
        body = np.array(c.sources, dtype=SRC_DT).tobytes() if n else b""
        (tmp_path / f"{k}.in").write_bytes(head + body + c.names + c.content)
        (tmp_path / f"{k}.want").write_bytes(struct.pack("<6Q2i", *summ, 0) + struct.pack("<Q", len(rows)) + (np.array(rows, dtype=ENT_DT).tobytes() if rows else b"")
                                             + (data or b""))
    out = subprocess.run([exe, str(tmp_path), str(len(CASES))], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test result: ok" in out.stdout, out.stdout + out.stderr
    print(out.stdout.strip())
