"""ZIP archives without a GPU: chip_zip_plan_host against the Python restatement of the walk (tests/zip_ref.py) on every case of
tests/zip_cases.py, records and summary; both against zipfile as the independent reader wherever zipfile reads the archive; what
the cases pin by name; the argument refusals of the four entry points, which answer before a device is looked for; and the walk
(compu_amd/csrc/zip_plan_core.h) in a stand-alone program under the address and undefined-behaviour sanitizers, over every case,
every prefix and every single-byte corruption of two small ones.  Without the feature every test here fails at the missing symbol."""
import ctypes as C
import io
import os
import struct
import subprocess
import zipfile

import numpy as np
import pytest

import zip_cases as Z
import zip_ref as R

CASES = Z.all_cases()
IDS = [c.name for c in CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_plan(data, max_entries=None):
    import compu_amd

    entries, summ = compu_amd.zip_plan_host(data, max_entries)
    return [tuple(int(v) for v in e) for e in entries.tolist()], summ.as_tuple()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_plan_equals_the_reference_walk(case):
    want = R.plan(case.data)
    assert host_plan(case.data) == want
    n = want[1][0]
    for m in {0, 1, n // 2, n + 3}:
        rows, summ = host_plan(case.data, m)
        assert summ == want[1] and rows == want[0][:m]


@pytest.mark.parametrize("case", [c for c in CASES if c.independent], ids=[c.name for c in CASES if c.independent])
def test_host_plan_agrees_with_zipfile(case):
    """name, method, flags, sizes, CRC-32 and header offset of every entry as zipfile's infolist() has them, and the bytes zipfile
    reads are the payload: both the plan and the case are pinned to an independent reader"""
    import compu_amd

    rows, summ = host_plan(case.data)
    assert summ[7] == R.OK and summ[0] == len(case.payloads)
    zf = zipfile.ZipFile(io.BytesIO(case.data))
    infos = zf.infolist()
    assert len(infos) == len(rows)
    entries, s = compu_amd.zip_plan_host(case.data)
    names = compu_amd.zip_names(entries, s, case.data[s.cd_off:s.cd_off + s.cd_size])
    for zi, row, name, payload in zip(infos, rows, names, case.payloads):
        header_off, data_off, comp_size, size, name_off, crc, name_len, method, flags, pad, status = row
        assert name == zi.orig_filename.encode("utf-8" if flags & 0x800 else "cp437")
        assert (method, flags, size, comp_size, crc, header_off) == (zi.compress_type, zi.flag_bits, zi.file_size, zi.compress_size, zi.CRC,
                                                                     zi.header_offset)
        assert status == R.ENT_OK and size == len(payload) and crc == Z.crc32(payload)
        assert zf.open(zi).read() == payload
        raw = case.data[data_off:data_off + comp_size]  # the plan's own data range holds the payload
        assert (raw if method == 0 else __import__("zlib").decompress(raw, -15)) == payload


def test_what_the_cases_pin():
    """the verdict each case is named for"""
    s = lambda name: R.plan(Z.by_name(name).data)  # noqa: E731
    for c in CASES:
        rows, summ = R.plan(c.data)
        if c.name.startswith("refused_"):
            assert summ[7] != R.OK, c.name
        elif not c.name.startswith("entry_") and c.name not in ("decoy_end_record_in_the_comment_wins", "accepted_count_smaller_than_the_chain"):
            assert summ[7] == R.OK and summ[1] == summ[0] == len(c.payloads), c.name
    for name in ("refused_21_bytes", "refused_22_zero_bytes", "refused_no_end_record", "refused_empty", "refused_trailing_bytes", "refused_trailing_64k",
                 "refused_end_record_cut"):
        assert s(name) == ([], (0, 0, 0, 0, 0, 0, 0, R.NO_EOCD, 0)), name
    for name in ("refused_locator_without_a_record", "refused_locator_points_behind_itself", "refused_locator_offset_2_pow_64_minus_1",
                 "refused_directory_overlaps_the_end_record", "refused_directory_behind_the_end_record", "refused_zip64_directory_overlaps_its_record",
                 "refused_directory_sum_wraps", "refused_directory_size_wraps", "refused_count_2_pow_32"):
        rows, summ = s(name)
        assert rows == [] and summ[7] == R.BAD_DIRECTORY and summ[0] == 0, name
    for name, at in (("refused_bad_signature_at_entry_0", 0), ("refused_bad_signature_at_entry_1", 1), ("refused_bad_signature_at_entry_last", 2),
                     ("refused_record_cut_by_the_directory_end", 2), ("refused_header_cut_by_the_directory_end", 2),
                     ("refused_count_larger_than_the_chain", 3), ("refused_empty_directory_with_a_count", 0), ("refused_missing_zip64_value_usize", 1),
                     ("refused_missing_zip64_value_csize", 1), ("refused_missing_zip64_value_lho", 1), ("refused_zip64_extra_one_value_short", 1),
                     ("refused_zip64_value_cut_by_the_extra_field", 1)):
        rows, summ = s(name)
        assert (len(rows), summ[0], summ[6], summ[7]) == (at, at, at, R.BAD_DIRECTORY), name
    for c in CASES:
        if c.name.startswith("refused_spanning_"):
            assert R.plan(c.data)[1][7] == R.UNSUPPORTED and R.plan(c.data)[0] == [], c.name
    assert s("accepted_count_smaller_than_the_chain")[1][0] == 2
    # the end record inside the comment that reaches the end wins: an archive of no entries whose end record is not the last one
    rows, summ = s("decoy_end_record_in_the_comment_wins")
    data = Z.by_name("decoy_end_record_in_the_comment_wins").data
    assert rows == [] and summ[7] == R.OK and summ[0] == 0 and summ[5] == data.rindex(b"PK\x05\x06") > data.index(b"PK\x05\x06")
    rows, summ = s("decoy_end_record_in_the_comment_ignored")
    data = Z.by_name("decoy_end_record_in_the_comment_ignored").data
    assert summ[0] == 3 and summ[5] == data.index(b"PK\x05\x06") < data.rindex(b"PK\x05\x06")
    status_of = {"entry_method_12": R.ENT_UNSUPPORTED, "entry_method_14": R.ENT_UNSUPPORTED, "entry_method_93": R.ENT_UNSUPPORTED,
                 "entry_encrypted_bit_0": R.ENT_ENCRYPTED, "entry_encrypted_bit_6": R.ENT_ENCRYPTED, "entry_encrypted_bit_13": R.ENT_ENCRYPTED,
                 "entry_method_12_and_encrypted": R.ENT_UNSUPPORTED, "entry_local_header_behind_the_directory_start": R.ENT_BAD_LOCAL,
                 "entry_local_header_in_the_directory": R.ENT_BAD_LOCAL, "entry_local_header_offset_2_pow_64_minus_1": R.ENT_BAD_LOCAL,
                 "entry_wrong_local_signature": R.ENT_BAD_LOCAL, "entry_data_reaches_into_the_directory": R.ENT_BAD_LOCAL,
                 "entry_comp_size_2_pow_64_minus_1": R.ENT_BAD_LOCAL, "entry_stored_with_another_size": R.ENT_BAD_LOCAL,
                 "entry_local_name_length_reaches_out": R.ENT_BAD_LOCAL, "entry_size_2_pow_32_minus_1_is_too_large": R.ENT_TOO_LARGE,
                 "entry_size_2_pow_32_minus_2_is_a_unit": R.ENT_OK, "entry_comp_size_2_pow_29_minus_63_in_a_tiny_file": R.ENT_BAD_LOCAL,
                 "entry_stored_size_2_pow_32_in_a_tiny_file": R.ENT_BAD_LOCAL, "entry_disk_1": R.ENT_UNSUPPORTED,
                 "entry_disk_ffff_without_zip64_extra": R.ENT_UNSUPPORTED, "entry_local_header_differs_from_the_directory": R.ENT_OK,
                 "zip64_extra_and_disk_ffff": R.ENT_OK}
    assert set(status_of) == {c.name for c in CASES if c.name.startswith("entry_") and c.name != "entry_data_at_every_alignment"} | {"zip64_extra_and_disk_ffff"}
    for name, want in status_of.items():
        rows, summ = s(name)
        statuses = [r[10] for r in rows]
        assert summ[7] == R.OK and summ[0] == 3 and want in statuses and all(v in (R.ENT_OK, want) for v in statuses), name
        assert summ[1] == statuses.count(R.ENT_OK) and summ[2] == sum(r[3] for r in rows if r[10] == R.ENT_OK), name
        for r in rows:
            assert (r[1] == 0) == (r[10] == R.ENT_BAD_LOCAL) or r[10] in (R.ENT_UNSUPPORTED, R.ENT_ENCRYPTED), name


def test_the_limits_of_a_unit_are_the_records_limits():
    """comp_size 2^29 - 63 cannot be stated in front of a small directory without being BAD_LOCAL first, so the TOO_LARGE rule's
    comp_size side is pinned on the record alone: the same entry in an archive whose directory lies behind 2^29 bytes of zeros"""
    import compu_amd

    limit = (1 << 29) - 64
    pay = Z.text(100, 50)
    for csize, want in ((limit, R.ENT_OK), (limit + 1, R.ENT_TOO_LARGE)):
        spec = Z.Spec("big", pay, Z.DEFLATED, cd=dict(csize=csize))
        a = Z.build([spec], gap=b"")
        # the gap is not materialised as Python bytes twice: one bytearray, handed over as a numpy view
        buf = np.zeros(len(a.data) + limit + 64, np.uint8)
        head = a.cd_off
        buf[:head] = np.frombuffer(a.data[:head], np.uint8)
        shift = limit + 64
        tail = bytearray(a.data[head:])
        struct.pack_into("<I", tail, len(tail) - 22 + 16, head + shift)  # the end record's directory offset
        buf[head + shift:] = np.frombuffer(bytes(tail), np.uint8)
        entries, summ = compu_amd.zip_plan_host(buf)
        assert summ.status == compu_amd.ZipStatus.Ok and summ.n_entries == 1
        assert int(entries[0]["status"]) == want and int(entries[0]["comp_size"]) == csize and int(entries[0]["data_off"]) == a.data_off[0]


def test_layouts_and_the_header():
    from compu_amd.api import _ZipDecodeSummary, _ZipEntry, _ZipPlanSummary, zip_entry_dtype

    assert C.sizeof(_ZipEntry) == 56 == zip_entry_dtype().itemsize and C.sizeof(_ZipPlanSummary) == 64 and C.sizeof(_ZipDecodeSummary) == 48
    text = open(os.path.join(ROOT, "include", "compu_hip.h")).read()
    assert "CHIP_ZIP_OK = 0, CHIP_ZIP_NO_EOCD = 1, CHIP_ZIP_BAD_DIRECTORY = 2, CHIP_ZIP_UNSUPPORTED = 3" in text
    for name, v in (("UNSUPPORTED", 16), ("ENCRYPTED", 17), ("BAD_LOCAL", 18), ("TOO_LARGE", 19), ("BAD_SIZE", 20), ("BAD_CRC", 21), ("BAD_INDEX", 22)):
        assert f"CHIP_ZIPENT_{name} = {v}" in text
    assert "#define CHIP_CRC_PIECE 65536u" in text


def test_argument_refusals_need_no_device():
    import compu_amd
    from compu_amd.api import _ZipDecodeSummary, _ZipPlanSummary

    lib = compu_amd.lib()
    ps, ds = _ZipPlanSummary(), _ZipDecodeSummary()
    p = C.c_void_p(4096)  # never read: every call below is refused at its arguments
    INVALID = -101
    assert lib.chip_zip_plan_host(p, 100, 0, None, None) == INVALID
    assert lib.chip_zip_plan_host(None, 100, 0, None, C.byref(ps)) == INVALID
    assert lib.chip_zip_plan_host(p, 100, 1, None, C.byref(ps)) == INVALID
    assert lib.chip_zip_plan_host(p, (1 << 40) + 1, 0, None, C.byref(ps)) == INVALID
    assert lib.chip_zip_plan_host(None, 0, 0, None, C.byref(ps)) == 0 and ps.status == R.NO_EOCD and ps.n_entries == 0
    assert lib.chip_zip_plan(p, 100, 0, None, None, None) == INVALID
    assert lib.chip_zip_plan(None, 100, 0, None, C.byref(ps), None) == INVALID
    assert lib.chip_zip_plan(p, 100, 1, None, C.byref(ps), None) == INVALID
    assert lib.chip_zip_plan(C.c_void_p(4098), 100, 0, None, C.byref(ps), None) == INVALID
    assert lib.chip_zip_plan(p, (1 << 40) + 1, 0, None, C.byref(ps), None) == INVALID
    ps.status = 77
    assert lib.chip_zip_plan(None, 0, 0, None, C.byref(ps), None) == 0  # an empty buffer: no device either
    assert (ps.status, ps.n_entries, ps.n_ok, ps.total_size, ps.cd_off, ps.cd_size, ps.eocd_off, ps.bad_index, ps.zip64) == (R.NO_EOCD, 0, 0, 0, 0, 0, 0, 0, 0)
    assert lib.chip_zip_plan(p, 21, 0, None, C.byref(ps), None) == 0 and ps.status == R.NO_EOCD  # too short for an end record
    assert lib.chip_crc32_batch(1, None, p, p, p, None) == INVALID and lib.chip_crc32_batch(1, p, None, p, p, None) == INVALID
    assert lib.chip_crc32_batch(1, p, p, None, p, None) == INVALID and lib.chip_crc32_batch(1, p, p, p, None, None) == INVALID
    assert lib.chip_crc32_batch(1 << 32, p, p, p, p, None) == INVALID
    assert lib.chip_crc32_batch(0, None, None, None, None, None) == 0
    good = [p, 1000, p, 3, 3, None, p, 1000, p, p, C.byref(ds), None]

    def refused(k, v):
        a = list(good)
        a[k] = v
        return lib.chip_zip_decode(*a)

    assert refused(10, None) == INVALID and refused(0, None) == INVALID and refused(0, C.c_void_p(4097)) == INVALID
    assert refused(1, (1 << 40) + 1) == INVALID and refused(2, None) == INVALID and refused(8, None) == INVALID and refused(9, None) == INVALID
    assert refused(6, None) == INVALID and refused(3, 1 << 31) == INVALID and refused(4, 1 << 31) == INVALID
    ds.status = 77
    assert refused(4, 0) == 0 and (ds.n_sel, ds.n_ok, ds.n_bad, ds.first_bad, ds.total_out, ds.status) == (0, 0, 0, 0, 0, 0)


def test_host_walk_under_the_sanitizers(tmp_path):
    """compu_amd/csrc/zip_plan_core.h in a stand-alone program built with the address and undefined-behaviour sanitizers: every case
    against the reference walk from exact-size heap buffers, every prefix and every single-byte corruption of two small cases"""
    exe = str(tmp_path / "test_zip_plan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_zip_plan.cpp")])
    dt = np.dtype([("header_off", "<u8"), ("data_off", "<u8"), ("comp_size", "<u8"), ("size", "<u8"), ("name_off", "<u8"), ("crc32", "<u4"),
                   ("name_len", "<u2"), ("method", "<u2"), ("flags", "<u2"), ("pad", "<u2"), ("status", "<i4")])
    small = []
    for k, c in enumerate(CASES):
        rows, summ = R.plan(c.data)
        (tmp_path / f"{k}.zip").write_bytes(c.data)
        (tmp_path / f"{k}.want").write_bytes(struct.pack("<7Q2i", *summ) + np.array(rows, dtype=dt).tobytes())
    # two small archives (ZIP64 records and extra; a file comment, a foreign subfield, an archive comment): every prefix and
    # every corruption of the whole file stays quick
    for j, specs in enumerate(([Z.Spec("a", b"abcdefgh", Z.STORED), Z.Spec("b", Z.text(60, 60), Z.DEFLATED, z64=("usize", "csize", "lho"))],
                               [Z.Spec("a", b"abc", Z.STORED, comment=b"c", extra_front=Z.W.subfield(7, b"xy")), Z.Spec("dir/", b"", Z.DEFLATED)])):
        k = len(CASES) + j
        data = Z.build(specs, zip64=(j == 0), comment=b"hi" * j).data
        rows, summ = R.plan(data)
        assert summ[7] == R.OK and summ[1] == 2
        (tmp_path / f"{k}.zip").write_bytes(data)
        (tmp_path / f"{k}.want").write_bytes(struct.pack("<7Q2i", *summ) + np.array(rows, dtype=dt).tobytes())
        small.append(str(k))
    out = subprocess.run([exe, str(tmp_path), str(len(CASES) + 2)] + small, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test result: ok" in out.stdout, out.stdout + out.stderr
    print(out.stdout.strip())
