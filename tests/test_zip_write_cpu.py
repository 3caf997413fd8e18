"""Writing ZIP archives without a GPU: chip_zip_assemble_host against the Python restatement of the rules (tests/zip_write_ref.py) on
every case of tests/zip_write_cases.py -- bytes, entries, summary, the bytes around the archive, sixteen alignments of `out`, one byte
too little room; zipfile, chip_zip_plan_host and the reference walk as readers of what it wrote; chip_zip_write_bound; the layouts
and the header's numbers; the argument refusals of the three calls, which answer before a device is looked for; and the assembly
(compu_amd/csrc/zip_write_core.h) in a stand-alone program under the address and undefined-behaviour sanitizers.  Without the feature
every test here fails at the missing symbol."""
import ctypes as C
import io
import os
import struct
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

import zip_ref as R
import zip_write_cases as ZC
import zip_write_ref as WR

CASES = ZC.all_cases()
IDS = [c.name for c in CASES]
READABLE = [c for c in CASES if c.real and not c.arith and not c.name.startswith("bad_")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA7
INVALID = -101


def arrays(case):
    """the case as the numpy arrays the C call takes"""
    import compu_amd

    src = np.array(case.sources, dtype=compu_amd.zip_source_dtype()) if case.sources else np.zeros(0, compu_amd.zip_source_dtype())
    u8 = lambda b: np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(1, np.uint8)  # noqa: E731
    comp = None
    if case.comp is not None:
        comp = (u8(case.comp[0]), len(case.comp[0]), np.array(case.comp[1], np.uint64), np.array(case.comp[2], np.uint32))
    return src, u8(case.names), u8(case.content), comp, np.array(case.crcs, np.uint32)


def run_host(case, out_cap=None, shift=0, want_entries=True):
    """chip_zip_assemble_host into a poisoned buffer, `out` `shift` bytes behind its start and 16 poisoned bytes behind out_cap:
    (the whole buffer as bytes, rows, summary tuple).  out_cap None: the room the reference states (0 for an arithmetic case)."""
    import compu_amd
    from compu_amd.api import ZipWriteSummary, _ZipWriteSummary

    src, names, content, comp, crc = arrays(case)
    if out_cap is None:
        out_cap = 0 if case.arith else case.want()[2][2]
    n = len(case.sources)
    buf = np.full(shift + out_cap + 16, POISON, np.uint8)
    entries = np.full(n + 1, POISON, np.uint8).repeat(56).view(compu_amd.zip_entry_dtype())
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    raw = _ZipWriteSummary()
    rc = compu_amd.lib().chip_zip_assemble_host(
        n, p(src) if n else None, p(names) if len(case.names) else None, len(case.names), p(content) if case.content_len else None, case.content_len,
        p(comp[0]) if comp else None, comp[1] if comp else 0, p(comp[2]) if comp else None, p(comp[3]) if comp else None, p(crc) if n else None,
        case.flags, C.c_void_p(buf.ctypes.data + shift) if out_cap else None, out_cap, p(entries) if want_entries else None, C.byref(raw))
    assert rc == 0
    assert entries[n:].tobytes() == bytes([POISON]) * 56  # nothing behind the rows
    return buf.tobytes(), [tuple(int(v) for v in e) for e in entries[:n].tolist()], ZipWriteSummary(raw).as_tuple(), entries[:n]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_assembly_equals_the_reference(case):
    """bytes, entries and summary; the bytes behind out_len intact; `out` at 16 alignments; one byte too little room"""
    want_bytes, want_rows, want_summ = case.want()
    buf, rows, summ, raw_rows = run_host(case)
    assert summ == want_summ
    bad = want_summ[7] == WR.BAD_SOURCE
    if bad or case.arith:
        assert buf == bytes([POISON]) * len(buf)
        if bad:  # nothing but the summary is written
            assert raw_rows.tobytes() == bytes([POISON]) * 56 * len(case.sources)
            assert summ == (len(case.sources), 0, 0, 0, 0, 0, summ[6], WR.BAD_SOURCE, 0)
        else:
            assert rows == want_rows and summ[7] == WR.NEED_OUTPUT
        return
    assert rows == want_rows and summ[7] == WR.OK
    assert buf == want_bytes + bytes([POISON]) * 16
    import compu_amd

    assert compu_amd.zip_write_bound(len(case.sources), sum(s[3] for s in case.sources), sum(s[1] for s in case.sources)) >= summ[2]
    if len(want_bytes) < (1 << 20):
        for shift in range(1, 16):
            buf, rows2, summ2, _ = run_host(case, shift=shift)
            assert buf == bytes([POISON]) * shift + want_bytes + bytes([POISON]) * 16 and rows2 == rows and summ2 == summ
    # one byte too little, and no room at all: NEED_OUTPUT, the exact length, the entries, nothing written
    for cap in (summ[2] - 1, 0):
        buf, rows2, summ2, _ = run_host(case, out_cap=cap)
        assert summ2 == summ[:7] + (WR.NEED_OUTPUT, summ[8]) and rows2 == rows and buf == bytes([POISON]) * len(buf)
    assert run_host(case, want_entries=False)[0] == want_bytes + bytes([POISON]) * 16


@pytest.mark.parametrize("case", READABLE, ids=[c.name for c in READABLE])
def test_zipfile_and_the_plan_read_what_was_written(case):
    """zipfile: names, methods, sizes, CRC, contents, testzip(); chip_zip_plan_host of the output gives the answered entries bytewise,
    and the reference walk agrees"""
    import compu_amd

    buf, rows, summ, entries = run_host(case)
    data = buf[:summ[2]]
    zf = zipfile.ZipFile(io.BytesIO(data))
    assert zf.testzip() is None
    infos = zf.infolist()
    assert len(infos) == len(case.sources)
    for zi, row, src, pay in zip(infos, rows, case.sources, case.payloads):
        name = case.names[src[2]:src[2] + src[3]]
        assert zi.orig_filename.encode("utf-8" if case.flags & WR.ZW_UTF8 else "cp437") == name
        assert (zi.compress_type, zi.file_size, zi.compress_size, zi.CRC, zi.header_offset) == (row[7], len(pay), row[2], zlib.crc32(pay), row[0])
        assert zf.open(zi).read() == pay
    planned, psumm = compu_amd.zip_plan_host(data)
    assert planned.tobytes() == entries.tobytes()
    n = len(case.sources)
    assert psumm.as_tuple() == (n, n, sum(len(p) for p in case.payloads), summ[3], summ[4], summ[5], 0, R.OK, summ[8])
    assert R.plan(data) == (rows, psumm.as_tuple())
    names = compu_amd.zip_names(planned, psumm, data[summ[3]:summ[3] + summ[4]])
    assert names == [case.names[s[2]:s[2] + s[3]] for s in case.sources]


def test_what_the_cases_pin():
    """the reference's answers the cases are named for, checked on the reference itself and on zipfile: the forms the writer's rules
    distinguish are the ones an independent reader accepts"""
    w = lambda name: ZC.by_name(name).want()  # noqa: E731
    assert w("empty")[0] == b"PK\x05\x06" + bytes(18) and len(w("empty_force")[0]) == 98 and w("empty_force")[2][8] == 1
    assert w("comp_len_size_minus_1_is_deflated")[1][0][7] == 8 and w("comp_len_1_is_deflated")[1][0][7] == 8
    for name in ("comp_len_size_is_stored", "comp_len_size_plus_1_is_stored", "comp_len_0_is_stored"):
        assert w(name)[1][0][7] == 0 and w(name)[1][0][2] == 40
    assert [r[7] for r in w("mixed")[1]] == [0, 0, 8, 0, 0] and w("mixed")[2][1] == 1 and w("no_comp_arrays")[2][1] == 0
    assert w("method_0_asked_for_text")[2][1] == 0 and w("text_deflates")[2][1] == 1 and w("noise_does_not")[2][1] == 0
    # the thresholds, as lengths: the ZIP64 sizes make the local part 20 bytes longer and the record 20; lho alone 12
    plain, big = w("arith_stored_m32_minus_1_is_plain")[2], w("arith_stored_m32_takes_the_zip64_sizes")[2]
    assert (plain[3], plain[4], plain[8]) == (31 + WR.M32 - 1, 47, 1) and (big[3], big[4]) == (31 + 20 + WR.M32, 47 + 20)
    a, b = w("arith_header_off_m32_minus_1_is_plain"), w("arith_header_off_m32_goes_into_the_subfield_alone")
    assert a[1][1][0] == WR.M32 - 1 and a[2][4] == 2 * 47 and b[1][1][0] == WR.M32 and b[2][4] == 2 * 47 + 12
    a, b = w("arith_cd_off_m32_minus_1_is_plain")[2], w("arith_cd_off_m32_alone_takes_the_zip64_end")[2]
    assert (a[3], a[8], a[2] - a[3] - a[4]) == (WR.M32 - 1, 0, 22) and (b[3], b[8], b[2] - b[3] - b[4], b[4]) == (WR.M32, 1, 98, 47)
    c = w("arith_cd_off_crosses_with_the_last_header_below")
    assert c[1][1][0] < WR.M32 <= c[2][3] and c[2][4] == 2 * 47 and c[2][8] == 1
    assert w("count_65534")[2][8] == 0 and w("count_65535")[2][8] == 1
    assert w("bad_two_bad_records_the_lower_wins")[2][6:8] == (1, WR.BAD_SOURCE) and w("bad_first_and_last")[2][6] == 0
    assert w("unused_stream_out_of_range_is_ignored")[2][7] == WR.OK
    # the FORCE form field by field, read by zipfile
    data = w("mixed_force")[0]
    zf = zipfile.ZipFile(io.BytesIO(data))
    assert zf.testzip() is None and [zi.extract_version for zi in zf.infolist()] == [45] * 5
    assert data[4:6] == b"\x2d\x00" and data[18:26] == b"\xff" * 8 and data[28:30] == b"\x14\x00"
    for n in (65534, 65535):
        zf = zipfile.ZipFile(io.BytesIO(w(f"count_{n}")[0]))
        assert len(zf.infolist()) == n and zf.infolist()[-1].filename == "e%05d" % (n - 1)


def test_layouts_and_the_header():
    import compu_amd
    from compu_amd.api import _ZipSource, _ZipWriteSummary

    assert C.sizeof(_ZipSource) == 32 == compu_amd.zip_source_dtype().itemsize and C.sizeof(_ZipWriteSummary) == 64
    text = open(os.path.join(ROOT, "include", "compu_hip.h")).read()
    assert "CHIP_ZIP_STORE = 0, CHIP_ZIP_DEFLATE = 8" in text and "CHIP_ZW_ZIP64 = 1, CHIP_ZW_UTF8 = 2" in text
    assert "CHIP_ZIPW_OK = 0, CHIP_ZIPW_NEED_OUTPUT = 1, CHIP_ZIPW_BAD_SOURCE = 2" in text and "#define CHIP_ZIPW_DEFLATE_MAX (1u << 30)" in text
    assert (compu_amd.ZIP_STORE, compu_amd.ZIP_DEFLATE, compu_amd.ZW_ZIP64, compu_amd.ZW_UTF8, compu_amd.ZIPW_DEFLATE_MAX) == (0, 8, 1, 2, 1 << 30)
    assert [int(v) for v in compu_amd.ZipWriteStatus] == [0, 1, 2]
    b = compu_amd.zip_write_bound
    assert b(0, 0, 0) == 98 and b(3, 10, 1000) == 1000 + 20 + 372 + 98 and b(1, 0, 2**64 - 223) == 2**64 - 1 and b(1, 0, 2**64 - 222) == 0
    assert b(1, 2**63, 0) == 0 and b(2**62, 0, 0) == 0 and b(2**31 - 1, 2**40, 2**40) == WR.bound(2**31 - 1, 2**40, 2**40)


def test_the_python_face_on_the_host():
    import compu_amd

    case = ZC.by_name("mixed_utf8")
    src, names, content, comp, crc = arrays(case)
    data, entries, summ = compu_amd.zip_assemble_host(src, case.names, case.content, crc, case.comp[0], case.comp[1], case.comp[2], flags=case.flags)
    want = case.want()
    assert data == want[0] and summ.as_tuple() == want[2] and [tuple(int(v) for v in e) for e in entries.tolist()] == want[1]
    data, entries, summ = compu_amd.zip_assemble_host(src, case.names, case.content, crc, flags=case.flags, out_cap=10)
    assert data == b"" and summ.status == compu_amd.ZipWriteStatus.NeedOutput and summ.n_deflated == 0
    case = ZC.by_name("arith_stored_2_pow_40")
    src, names, content, comp, crc = arrays(case)
    data, entries, summ = compu_amd.zip_assemble_host(src, case.names, case.content, crc, out_cap=0, content_len=case.content_len)
    assert summ.as_tuple() == case.want()[2] and int(entries[0]["size"]) == 1 << 40


def test_argument_refusals_need_no_device():
    import compu_amd
    from compu_amd.api import _ZipWriteSummary

    lib = compu_amd.lib()
    ws = _ZipWriteSummary()
    p = C.c_void_p(4096)  # never read: every call below is refused at its arguments
    S = C.byref(ws)
    # n, src, names, names_len, content, content_len, comp, comp_all, comp_off, comp_len, crc, flags, out, out_cap, entries, summary
    good = [3, p, p, 10, p, 100, p, 50, p, p, p, 0, p, 1000, p, S]

    def refused(call, base, k, v, *more):
        a = list(base)
        a[k] = v
        for kk, vv in zip(more[::2], more[1::2]):
            a[kk] = vv
        return call(*a) == INVALID

    for call, args in ((lib.chip_zip_assemble_host, good), (lib.chip_zip_assemble, good + [None])):
        assert refused(call, args, 15, None) and refused(call, args, 1, None) and refused(call, args, 2, None) and refused(call, args, 4, None)
        assert refused(call, args, 10, None) and refused(call, args, 12, None)
        for gone in ((6,), (8,), (9,), (6, 8), (6, 9), (8, 9)):  # exactly one or two of the three comp arrays
            a = list(args)
            for k in gone:
                a[k] = None
            assert call(*a) == INVALID
        assert refused(call, args, 0, 1 << 31) and refused(call, args, 11, 4) and refused(call, args, 11, 0x80000000)
        assert refused(call, args, 5, 1 << 62) and refused(call, args, 0, (1 << 31) - 1, 5, 1 << 40)
    # n, names_len or content_len of 0 need no pointer; entries may be NULL; with too little room for no entries the host answers
    for call, tail in ((lib.chip_zip_assemble_host, []), (lib.chip_zip_assemble, [None])):
        for flags, want in ((0, 22), (1, 98)):
            ws.status = 77
            assert call(0, None, None, 0, None, 0, None, 0, None, None, None, flags, None, 0, None, S, *tail) == 0
            assert (ws.n_entries, ws.n_deflated, ws.out_len, ws.cd_off, ws.cd_size, ws.eocd_off, ws.bad_index, ws.status, ws.zip64) == (
                0, 0, want, 0, 0, want - 22, 0, WR.NEED_OUTPUT, flags)
            assert call(0, None, None, 0, None, 0, None, 0, None, None, None, flags, p, want - 1, None, S, *tail) == 0 and ws.status == WR.NEED_OUTPUT
    # level, flags, n, src, names, names_len, in_base, in_len, out_base, out_cap, entries, summary, stream
    good = [6, 0, 3, p, p, 10, p, 100, p, 1000, p, S, None]
    call = lib.chip_zip_write
    assert refused(call, good, 11, None) and refused(call, good, 3, None) and refused(call, good, 4, None) and refused(call, good, 6, None)
    assert refused(call, good, 8, None) and refused(call, good, 2, 1 << 31) and refused(call, good, 1, 4) and refused(call, good, 0, 10)
    assert refused(call, good, 0, -2) and refused(call, good, 6, C.c_void_p(4098)) and refused(call, good, 7, 1 << 62)
    for flags, want in ((2, 22), (3, 98)):
        assert call(-1, flags, 0, None, None, 0, None, 0, None, 0, None, S, None) == 0
        assert (ws.out_len, ws.eocd_off, ws.status, ws.zip64) == (want, want - 22, WR.NEED_OUTPUT, flags & 1)


def test_assembly_under_the_sanitizers(tmp_path):
    """compu_amd/csrc/zip_write_core.h in a stand-alone program built with the address and undefined-behaviour sanitizers: every case
    from exact-size heap buffers against the reference's files, and the record formatters at the 2^32 and 65 535 thresholds against
    the reference's bytes"""
    exe = str(tmp_path / "test_zip_write")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_zip_write.cpp")])
    src_dt = np.dtype([("data_off", "<u8"), ("size", "<u8"), ("name_off", "<u8"), ("name_len", "<u2"), ("method", "<u2"), ("dos_time", "<u2"),
                       ("dos_date", "<u2")])
    ent_dt = np.dtype([("header_off", "<u8"), ("data_off", "<u8"), ("comp_size", "<u8"), ("size", "<u8"), ("name_off", "<u8"), ("crc32", "<u4"),
                       ("name_len", "<u2"), ("method", "<u2"), ("flags", "<u2"), ("pad", "<u2"), ("status", "<i4")])
    for k, c in enumerate(CASES):
        data, rows, summ = c.want()
        n = len(c.sources)
        have = c.comp is not None
        head = struct.pack("<8Q", n, len(c.names), len(c.content), c.content_len, int(have), len(c.comp[0]) if have else 0, c.flags, int(c.arith))
        body = np.array(c.sources, dtype=src_dt).tobytes() if n else b""
        body += np.array(c.crcs, "<u4").tobytes()
        if have:
            body += np.array(c.comp[1], "<u8").tobytes() + np.array(c.comp[2], "<u4").tobytes() + c.comp[0]
        (tmp_path / f"{k}.in").write_bytes(head + body + c.names + c.content)
        (tmp_path / f"{k}.want").write_bytes(struct.pack("<7Q2i", *summ) + struct.pack("<Q", len(rows)) + (np.array(rows, dtype=ent_dt).tobytes() if rows else b"")
                                             + data)
    # the formatters at the thresholds: the central record and the local header of the second entry, and the end records, as the
    # reference writes them for the arithmetic cases
    probes = []
    for name in ("arith_stored_m32_minus_1_is_plain", "arith_stored_m32_takes_the_zip64_sizes", "arith_header_off_m32_minus_1_is_plain",
                 "arith_header_off_m32_goes_into_the_subfield_alone", "arith_cd_off_m32_minus_1_is_plain", "arith_cd_off_m32_alone_takes_the_zip64_end",
                 "arith_both_forms_in_one_entry", "arith_forced_small", "count_65534", "count_65535"):
        probes.append(str(IDS.index(name)))
        c = ZC.by_name(name)
        k = IDS.index(name)
        (tmp_path / f"{k}.records").write_bytes(record_bytes(c))
    out = subprocess.run([exe, str(tmp_path), str(len(CASES))] + probes, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test result: ok" in out.stdout, out.stdout + out.stderr
    print(out.stdout.strip())


def record_bytes(case):
    """the generated bytes of a case's LAST entry and its end records as the reference's record functions write them, without the
    data: local header (30) | local extra | central record (46) | central extra | end records"""
    import zip_writer as W

    _, rows, summ = case.want()
    header_off, data_off, c, size, name_off, crc, name_len, method, gp, _, _ = rows[-1]
    src = case.sources[-1]
    force = bool(case.flags & WR.ZW_ZIP64)
    zs, zl = force or size >= WR.M32 or c >= WR.M32, force or header_off >= WR.M32
    vals = ([size, c] if zs else []) + ([header_off] if zl else [])
    version = 45 if vals else 20 if method == 8 else 10
    lextra = W.zip64_extra([size, c]) if zs else b""
    local = W.local_header(b"", method, gp, crc, WR.M32 if zs else c, WR.M32 if zs else size, version=version, dos_time=src[5], dos_date=src[6])
    local = local[:26] + struct.pack("<HH", name_len, len(lextra))
    cextra = W.zip64_extra(vals) if vals else b""
    rec = W.central_record(b"", method, gp, crc, WR.M32 if zs else c, WR.M32 if zs else size, WR.M32 if zl else header_off, made_by=version,
                           version=version, dos_time=src[5], dos_date=src[6], nlen=name_len, xlen=len(cextra))
    n, cd_off, cd_size = summ[0], summ[3], summ[4]
    end = (W.end_record64(n, n, cd_size, cd_off) + W.locator64(cd_off + cd_size) if summ[8] else b"") + W.end_record(
        min(n, 0xFFFF), min(n, 0xFFFF), min(cd_size, WR.M32), min(cd_off, WR.M32))
    return local + lextra + rec + cextra + end
