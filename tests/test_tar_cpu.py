"""tar archives without a GPU: chip_tar_plan_host against the Python restatement of the walk (tests/tar_ref.py) on every case of
tests/tar_cases.py and on every cut of it -- records, summary, max_entries of 0, 1 and exact, the bytes behind the written records
untouched; against tarfile as the independent reader on every well-formed case; what the cases pin by name; tar_names on host
bytes; the argument refusals, which answer before a device is looked for.  Cuts: every multiple of 512 and 1, 100, 511, 513,
len - 1 of every image, the 3 000-member image (6 001 blocks) included: the reference keeps between the prefixes of one image what
does not depend on the length (tar_ref.Memo), and is compared with the plain walk of the cut bytes on every cut of the small images
and on sampled cuts of the long one.  Every test here calls the library, so without the feature each fails at the missing symbol."""
import ctypes as C
import io
import os
import struct
import subprocess
import tarfile

import numpy as np
import pytest

import tar_cases as T
import tar_ref as R

CASES = T.all_cases()
IDS = [c.name for c in CASES]
POISON = 0xA7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_plan_bytes(data, max_entries=None, room=None):
    """chip_tar_plan_host into a poisoned array of `room` records: (the records' bytes, summary tuple); what lies behind the records
    the call owes must still hold the poison"""
    import compu_amd
    from compu_amd.api import TarPlanSummary, _TarPlanSummary

    lib, dt = compu_amd.lib(), compu_amd.tar_entry_dtype()
    buf = np.frombuffer(data, np.uint8)
    s = _TarPlanSummary()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    if max_entries is None:
        assert lib.chip_tar_plan_host(p(buf), len(data), 0, None, C.byref(s)) == 0
        max_entries = int(s.n_entries)
    room = max_entries + 2 if room is None else room
    rows = np.full(room * dt.itemsize, POISON, np.uint8)
    assert lib.chip_tar_plan_host(p(buf), len(data), max_entries, p(rows) if max_entries else None, C.byref(s)) == 0
    k = min(max_entries, int(s.n_entries))
    assert (rows[k * dt.itemsize:] == POISON).all()
    return rows[:k * dt.itemsize].tobytes(), TarPlanSummary(s).as_tuple()


def host_plan(data, max_entries=None, room=None):
    """host_plan_bytes with the records as tuples"""
    import compu_amd

    rows, summ = host_plan_bytes(data, max_entries, room)
    return [tuple(int(v) for v in e) for e in np.frombuffer(rows, compu_amd.tar_entry_dtype()).tolist()], summ


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_plan_equals_the_reference_walk(case):
    want = R.plan(case.data)
    assert want[1][5] == case.status
    assert host_plan(case.data) == want
    n = want[1][0]
    for m in sorted({0, 1, n}):
        rows, summ = host_plan(case.data, m, room=n + 3)
        assert summ == want[1] and rows == want[0][:m]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_plan_equals_the_reference_walk_on_every_cut(case):
    import compu_amd

    assert host_plan(case.data[:0]) == R.plan(b"") == ([], (0, 0, 0, 0, 0, R.OK, 0))
    full, memo = R.plan(case.data)[0], R.Memo()
    full_bytes = np.array(full, dtype=compu_amd.tar_entry_dtype()).tobytes() if full else b""
    for c in T.cuts(case.data, every_block=True):
        want = R.plan(case.data, n=c, memo=memo)
        if len(full) <= 100:  # the walk with what it keeps between prefixes is the walk without
            assert want == R.plan(case.data[:c]), c
        k = len(want[0])
        assert want[0] == full[:k], c  # a walk that stops keeps the members in front of the stop
        rows, summ = host_plan_bytes(case.data[:c])
        assert summ == want[1] and rows == full_bytes[:72 * k], c
    if len(full) > 100:  # and on the long image at sampled cuts
        for c in T.cuts(case.data, every_block=False):
            assert R.plan(case.data, n=c, memo=memo) == R.plan(case.data[:c]), c


def tarfile_members(data):
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:", encoding="utf-8", errors="surrogateescape") as t:
        return [(m.offset_data, m.size if m.isreg() else 0, m.linkname.encode("utf-8", "surrogateescape"),
                 m.name.encode("utf-8", "surrogateescape").rstrip(b"/")) for m in t.getmembers()]


WELLFORMED = [c for c in CASES if c.wellformed]


@pytest.mark.parametrize("case", WELLFORMED, ids=[c.name for c in WELLFORMED])
def test_host_plan_agrees_with_tarfile(case):
    """member count, offset_data, size (0 where tarfile says the member is no regular file), link name and name of every member"""
    import compu_amd

    entries, summ = compu_amd.tar_plan_host(case.data)
    assert summ.status == compu_amd.TarStatus.Ok and summ.stop_off == summ.bad_off
    names = compu_amd.tar_names(entries, case.data)
    links = [case.data[int(e["link_off"]):int(e["link_off"]) + int(e["link_len"])] for e in entries]
    got = [(int(e["data_off"]), int(e["size"]), link, name.rstrip(b"/")) for e, link, name in zip(entries, links, names)]
    assert got == tarfile_members(case.data)
    assert summ.n_entries == len(got) and summ.total_size == sum(g[1] for g in got)
    assert names == R.names(R.plan(case.data)[0], case.data)


def test_what_the_cases_pin():
    """the verdict each case is named for"""
    def plan(name):
        c = T.by_name(name)
        rows, summ = R.plan(c.data)
        assert host_plan(c.data) == (rows, summ), name  # the pins below hold for the library as for the reference
        return [dict(zip(R.FIELDS, r)) for r in rows], summ, R.names(rows, c.data), c.data

    for tag in ("ustar", "gnu", "pax"):
        rows, summ, names, data = plan("tarfile_" + tag)
        assert summ[5] == R.OK and summ[6] == 2 and summ[1] == (1 if tag == "pax" else 0)
        for want in (T.NAME_99, T.NAME_100, T.NAME_102, T.NAME_241) + ((T.NAME_300,) if tag != "ustar" else ()):
            assert want in names
        assert not any(n.startswith((b"inner/", b"decoy/")) for n in names)  # the marking never reached the decoys
        by = dict(zip(names, rows))
        assert by[T.NAME_241]["prefix_len"] == (140 if tag == "ustar" else 0)
        assert by[T.NAME_241]["flags"] == {"ustar": 0, "gnu": R.NAME_GNU, "pax": R.NAME_PAX}[tag]
        if tag != "ustar":
            assert by[b"long/symlink"]["flags"] == (R.LINK_GNU if tag == "gnu" else R.LINK_PAX) and by[b"long/symlink"]["link_len"] == 200
            assert by[T.NAME_300]["group_off"] < by[T.NAME_300]["header_off"]
        assert by[b"dir/hardlink"]["typeflag"] == ord("1") and by[b"dir/hardlink"]["size"] == 0
        nested = by[b"nested.tar"]
        assert data[nested["data_off"] + 257:nested["data_off"] + 262] == b"ustar"
    rows, summ, names, _ = plan("many_members")
    assert summ[:3] == (3000, 0, 3000) and names[2999] == b"many/02999"
    rows, summ, names, _ = plan("base256_size")
    assert rows[1]["size"] == 700 and rows[1]["flags"] == R.SIZE_BASE256
    rows, summ, names, _ = plan("pax_size_disagrees")
    assert rows[1]["size"] == 600 and rows[1]["flags"] == R.SIZE_PAX and names[2] == b"last"
    assert plan("name_L_then_x")[2][1] == b"from-x" and plan("name_L_then_x")[0][1]["flags"] == R.NAME_PAX
    assert plan("name_x_then_L")[2][1] == b"from-L" + b"l" * 130 and plan("name_x_then_L")[0][1]["flags"] == R.NAME_GNU
    rows, summ, names, data = plan("link_K_and_pax")
    assert data[rows[1]["link_off"]:rows[1]["link_off"] + rows[1]["link_len"]] == b"x-target" and rows[1]["flags"] == R.LINK_PAX
    rows, summ, names, _ = plan("prefix_and_name")
    assert names[1] == b"some/dir/leaf" and rows[1]["prefix_len"] == 8
    rows, summ, names, _ = plan("invalid_mode_and_mtime_are_zero")
    assert (rows[1]["mode"], rows[1]["mtime"], rows[0]["mode"], rows[0]["mtime"]) == (0, 0, 0o644, 0o14000000000)
    first = 1024  # the member in front of what each of these is about
    assert plan("typeflag_S")[1] == (1, 0, 3, first, first, R.UNSUPPORTED, 0)
    assert plan("gnu_sparse_key")[1] == (1, 0, 3, first, first, R.UNSUPPORTED, 0)
    assert plan("sixteen_extension_headers")[1][:2] == (3, 0) and plan("sixteen_extension_headers")[2][1] == b"name-15"
    assert plan("seventeen_extension_headers")[1] == (1, 0, 3, first, first + 16 * 1024, R.UNSUPPORTED, 0)
    assert plan("extension_data_too_large")[1] == (1, 0, 3, first, first, R.UNSUPPORTED, 0)
    assert plan("g_behind_L")[1] == (1, 0, 3, first, first + 1024, R.BAD_HEADER, 0)
    assert plan("g_twice_then_members")[1][:3] == (2, 2, 8)
    assert plan("extension_header_before_a_bad_header")[1] == (1, 0, 3, first, first + 1024, R.BAD_HEADER, 0)
    assert plan("extension_header_at_the_end")[1] == (1, 0, 3, first, first, R.TRUNCATED, 0)
    for name, _ in T.malformed_pax():
        assert plan(name)[1] == (1, 0, 3, first, first, R.BAD_HEADER, 0), name
    assert plan("flipped_byte_in_a_middle_header")[1] == (1, 0, 3, first, first, R.BAD_HEADER, 0)
    assert plan("one_zero_block_then_garbage")[1] == (1, 0, 3, first, first, R.OK, 1)
    for k, blocks in ((0, 0), (1, 1), (2, 2), (20, 2)):
        assert plan("zero_blocks_%d" % k)[1] == (2, 0, 8, 2048, 2048, R.OK, blocks)
    assert plan("header_first_bytes_only")[1] == (0, 0, 0, 0, 0, R.TRUNCATED, 0)
    assert plan("content_without_padding")[1] == (0, 0, 0, 0, 0, R.TRUNCATED, 0)
    assert plan("empty")[1] == (0, 0, 0, 0, 0, R.OK, 0) and plan("zero_blocks_only")[1] == (0, 0, 0, 0, 0, R.OK, 2)


def test_number_fields():
    """the rule of a number field, on the reference and through the size field on the host plan"""
    for field, want in ((b"00000000017\0", 15), (b"         17 ", 15), (b" " * 12, 0), (b"\0" * 12, 0), (b"17\0garbage!!", 15), (b"777777777777", (1 << 36) - 1),
                        (b"0000000001a\0", None), (b"00000000018\0", None), (b"\xff" * 12, None), (b"-1\0" + b"\0" * 9, None),
                        (b"\x80" + (5).to_bytes(11, "big"), 5), (b"\x80" + ((1 << 63) - 1).to_bytes(11, "big"), (1 << 63) - 1),
                        (b"\x80" + (1 << 63).to_bytes(11, "big"), None), (b"\x80" + b"\xff" * 11, None)):
        got = R.number(field)
        assert (got[0] if got else None) == want, field
        image = T.header(b"n", size_field=field, typeflag=b"g") + bytes(1024)  # (a global header: its size only moves the end)
        rows, summ = host_plan(image)
        if want is None:
            assert summ == (0, 0, 0, 0, 0, R.BAD_HEADER, 0), field
        else:
            assert summ[5] == (R.OK if want <= 1024 else R.TRUNCATED), field
        assert (rows, summ) == R.plan(image)


def test_names_from_host_bytes():
    import compu_amd

    case = T.by_name("tarfile_ustar")
    entries, summ = compu_amd.tar_plan_host(case.data)
    names = compu_amd.tar_names(entries, case.data)
    assert names == R.names(R.plan(case.data)[0], case.data) and T.NAME_241 in names and "dir/grüße-世界.txt".encode() in names
    assert compu_amd.tar_names(entries[:3], np.frombuffer(case.data, np.uint8)) == names[:3]
    assert compu_amd.tar_names(entries[:0], case.data) == []
    assert compu_amd.tar_plan_host(case.data, max_entries=4)[0].tobytes() == entries[:4].tobytes()
    assert compu_amd.tar_entry_dtype().itemsize == 72 and compu_amd.tar_entry_dtype().names == R.FIELDS


def test_host_walk_under_the_sanitizers(tmp_path):
    """compu_amd/csrc/tar_plan_core.h in a stand-alone program built with the address and undefined-behaviour sanitizers: every case
    against the reference walk from exact-size heap buffers, every prefix and every single-byte corruption of three small images
    (extension headers of every kind, pax records, a global header)"""
    exe = str(tmp_path / "test_tar_plan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_tar_plan.cpp")])
    dt = np.dtype([(f, t) for f, t in zip(R.FIELDS, ("<u8",) * 6 + ("<i8",) + ("<u4",) * 3 + ("<u2", "u1", "u1"))])
    assert dt.itemsize == 72
    small = (T.ext(b"g", T.pax_record(b"comment", b"c")) + T.group_of([T.ext(b"x", T.pax_record(b"path", b"p/q") + T.pax_record(b"size", b"7") +
                                                                         T.pax_record(b"linkpath", b"l"))]) + T.END,
             T.group_of([T.ext(b"L", b"long-name\0"), T.ext(b"K", b"long-link")], b"m", b"") + T.member(b"n", b"x" * 513, prefix=b"pre") + bytes(512),
             T.header(b"b256", size_field=b"\x80" + (3).to_bytes(11, "big")) + T.padded(b"abc") + T.member(b"h\xff", b"", signed=True, typeflag=b"5"))
    images = [c.data for c in CASES] + list(small)
    for k, data in enumerate(images):
        rows, summ = R.plan(data)
        (tmp_path / f"{k}.tar").write_bytes(data)
        (tmp_path / f"{k}.want").write_bytes(struct.pack("<5Q2i", *summ) + np.array(rows, dtype=dt).tobytes())
    for data in small:
        assert R.plan(data)[1][5] == R.OK
    out = subprocess.run([exe, str(tmp_path), str(len(images))] + [str(len(CASES) + j) for j in range(len(small))], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "test result: ok" in out.stdout, out.stdout + out.stderr
    print(out.stdout.strip())


def test_argument_errors_need_no_device():
    import compu_amd
    from compu_amd.api import _TarPlanSummary

    lib, s, E_INVALID = compu_amd.lib(), _TarPlanSummary(), -101
    data = np.frombuffer(T.by_name("zero_blocks_2").data, np.uint8)
    ptr = data.ctypes.data_as(C.c_void_p)
    rows = np.zeros(4 * 72, np.uint8).ctypes.data_as(C.c_void_p)
    for host in (True, False):
        call = (lambda *a: lib.chip_tar_plan_host(*a)) if host else (lambda *a: lib.chip_tar_plan(*a, None))
        assert call(ptr, data.size, 0, None, None) == E_INVALID  # no summary
        assert call(None, 512, 0, None, C.byref(s)) == E_INVALID  # no buffer
        assert call(ptr, data.size, 1, None, C.byref(s)) == E_INVALID  # no array
        assert call(ptr, (1 << 40) + 1, 4, rows, C.byref(s)) == E_INVALID  # too long
        s.status, s.n_entries = 7, 7
        assert call(None, 0, 0, None, C.byref(s)) == 0 and (s.n_entries, s.n_global, s.total_size, s.stop_off, s.bad_off, s.status, s.zero_blocks) == (
            0, 0, 0, 0, 0, 0, 0)  # an empty image is fine, and needs no device either
    assert lib.chip_tar_plan(C.c_void_p(ptr.value + 2), 512, 0, None, C.byref(s), None) == E_INVALID  # misaligned
