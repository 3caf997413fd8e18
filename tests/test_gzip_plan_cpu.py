"""The gzip member index without a GPU: the reference plan of every case (gzip_plan_ref.py: the walk of include/compu_hip.h over the
CPU oracle) against an independent reading by Python's zlib; the zeros member of the 2^32 cases against zlib; chip_gzip_plan's
argument refusals, which come before the device is looked for; the header's enum and struct against the ctypes mirror.  Without
the feature the refusal and mirror tests fail at the missing symbol."""
import ctypes as C
import os
import re
import zlib

import pytest

import gzip_plan_cases as G
import gzip_plan_ref as R

E_INVALID, E_NO_DEVICE = -101, -100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def zlib_members(twin):
    """whole members from position 0 as zlib reads them, one decompressobj(31) each: [(start, length, content)], and where it stopped"""
    p, out = 0, []
    while p < len(twin):
        d = zlib.decompressobj(31)
        try:
            content = d.decompress(twin[p:])
        except zlib.error:
            break
        if not d.eof:
            break
        used = len(twin) - p - len(d.unused_data)
        out.append((p, used, content))
        p += used
    return out, p


@pytest.mark.parametrize("case", G.all_cases(), ids=[c.name for c in G.all_cases()])
def test_reference_plan_equals_zlibs_reading(case):
    rows, summ = R.reference(case.name)
    members, stopped = zlib_members(case.twin)
    assert [(r[0], r[1]) for r in rows] == [(m[0], m[1]) for m in members]
    assert [r[3] for r in rows] == [len(m[2]) for m in members]
    assert [r[2] for r in rows] == [sum(len(m[2]) for m in members[:i]) for i in range(len(members))]
    assert summ[:3] == (len(members), sum(len(m[2]) for m in members), stopped)
    assert [m[2] for m in members] == case.contents
    assert (summ[3] == G.OK) == (stopped == len(case.twin))
    assert (summ[4] != 0) == (summ[3] == G.BAD_MEMBER)
    # the file differs from its twin in the CRC-32 of the members named, and nowhere else
    diff = [i for i in range(len(case.data)) if case.data[i] != case.twin[i]]
    spans = [range(rows[k][0] + rows[k][1] - 8, rows[k][0] + rows[k][1] - 4) for k in case.bad_crc]
    if case.name != "third_wrong_crc_and_cut_isize":
        assert diff and all(any(i in s for s in spans) for i in diff) if case.bad_crc else not diff


def test_every_stop_is_reached():
    """the statuses the cases were built for, each as the first member and behind two good ones"""
    want = {
        "cut_in_header": G.TRUNCATED, "cut_in_header_after_4": G.TRUNCATED, "cut_in_deflate": G.TRUNCATED, "cut_in_trailer_1": G.TRUNCATED,
        "cut_in_trailer_5": G.TRUNCATED, "cut_before_trailer": G.TRUNCATED, "trailing_1": G.TRUNCATED, "trailing_2": G.TRUNCATED,
        "trailing_3": G.TRUNCATED, "trailing_zeros": G.BAD_HEADER, "trailing_zeros_4": G.BAD_HEADER, "zlib_stream": G.BAD_HEADER,
        "1f_8b_07": G.BAD_HEADER, "reserved_flg_bit_5": G.BAD_HEADER, "reserved_flg_bit_7": G.BAD_HEADER, "block_type_3": G.BAD_MEMBER,
        "wrong_isize": G.BAD_MEMBER, "wrong_fhcrc": G.BAD_MEMBER, "distance_too_far": G.BAD_MEMBER, "stored_len_nlen": G.BAD_MEMBER,
    }
    two = sum(len(G.member(c, level=lv)) for c, lv in ((G.text(700, 1), 6), (G.text(90, 2), 1)))
    for stop, status in want.items():
        for prefix, n, at in (("first_", 0, 0), ("third_", 2, two)):
            rows, summ = R.reference(prefix + stop)
            assert (summ[0], summ[2], summ[3]) == (n, at, status), prefix + stop
            assert summ[4] == (-3 if status == G.BAD_MEMBER else 0), prefix + stop
    assert R.reference("block_type_3_then_a_good_member")[1] == (2, 790, two, G.BAD_MEMBER, -3)
    assert R.reference("zeros_then_a_good_member")[1] == (2, 790, two, G.BAD_HEADER, 0)
    assert R.reference("first_wrong_crc")[1][3] == G.OK and R.reference("third_wrong_crc")[1][:1] + R.reference("third_wrong_crc")[1][3:] == (4, G.OK, 0)
    assert R.reference("third_wrong_crc_and_cut_isize")[1] == (2, 790, two, G.TRUNCATED, 0)
    assert R.reference("three_thousand_tiny")[1][0] == 3000


def test_zeros_member_inflates_under_zlib():
    """the member of the 2^32 cases in its 64-chunk form, and with the short last chunk: zlib reads what the arithmetic says"""
    c, d = G.zero_chunks()
    assert len(c) == 1037
    for short in (False, True):
        m, size = G.zeros_member(64, short_tail=short)
        assert size == 64 * G.MIB + (G.MIB - 2 if short else 0)
        dec = zlib.decompressobj(-15)
        body = m[10:-8]
        total, pos = 0, 0
        while pos < len(body):  # (in pieces: the whole output need not be held)
            out = dec.decompress(body[pos:pos + 4096])
            assert out.count(0) == len(out)
            total += len(out)
            pos += 4096
        assert dec.eof and dec.unused_data == b"" and total == size
        assert int.from_bytes(m[-4:], "little") == size
    for name, data, rows, summ in G.edge_cases():
        assert summ[0] == len(rows) and (not rows or rows[-1][0] + rows[-1][1] == summ[2]) and sum(r[3] for r in rows) == summ[1]
        assert all(r[3] <= 0xFFFFFFFE for r in rows)


def test_arguments_are_checked_before_the_device():
    import compu_amd

    lib = compu_amd.lib()
    assert hasattr(lib, "chip_gzip_plan")
    s = G.new_summary()
    buf = (C.c_uint32 * 16)()
    base = C.cast(buf, C.c_void_p)
    arr = [C.cast((C.c_uint64 * 4)(), C.c_void_p) for _ in range(4)]
    none = [None] * 4
    call = lib.chip_gzip_plan
    assert call(base, 40, 0, *none, None, None) == E_INVALID  # no summary
    assert call(None, 40, 0, *none, C.byref(s), None) == E_INVALID  # no buffer, but a length
    assert call(base, 40, 1, *none, C.byref(s), None) == E_INVALID  # no arrays, but room asked for
    for k in range(4):
        assert call(base, 40, 1, *[None if j == k else arr[j] for j in range(4)], C.byref(s), None) == E_INVALID
    assert call(C.c_void_p(C.addressof(buf) + 2), 40, 0, *none, C.byref(s), None) == E_INVALID  # misaligned
    assert call(base, (1 << 40) + 1, 0, *none, C.byref(s), None) == E_INVALID
    assert (s.n_members, s.total_out, s.in_used, s.status, s.member_status) == (7, 7, 7, 7, 7)  # a refusal writes nothing
    assert call(None, 0, 0, *none, C.byref(s), None) == 0  # an empty buffer is fine, also without a device
    assert (s.n_members, s.total_out, s.in_used, s.status, s.member_status) == (0, 0, 0, 0, 0)
    if lib.chip_device_count() == 0:  # (with a device these host pointers must not reach a kernel)
        assert call(base, 40, 0, *none, C.byref(s), None) == E_NO_DEVICE
        assert call(base, 40, 1, *none, C.byref(s), None) == E_INVALID  # the refusal comes first


def test_header_and_mirrors_agree():
    import compu_amd
    from compu_amd.api import _GzipPlanSummary

    text = open(os.path.join(ROOT, "include", "compu_hip.h")).read()
    enum = re.search(r"enum \{ (CHIP_GZPLAN_OK[^}]*) \};", text).group(1)
    values = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(","))}
    assert values == {"CHIP_GZPLAN_OK": G.OK, "CHIP_GZPLAN_TRUNCATED": G.TRUNCATED, "CHIP_GZPLAN_BAD_HEADER": G.BAD_HEADER,
                      "CHIP_GZPLAN_TOO_LARGE": G.TOO_LARGE, "CHIP_GZPLAN_BAD_MEMBER": G.BAD_MEMBER}
    assert [(s.name, s.value) for s in compu_amd.GzipPlanStatus] == [("Ok", 0), ("Truncated", 1), ("BadHeader", 2), ("TooLarge", 3), ("BadMember", 4)]
    assert re.search(r"#define CHIP_GZPLAN_WINDOW \(\(1u << 29\) - 64u\)", text)
    assert compu_amd.GZPLAN_WINDOW == R.WINDOW == (1 << 29) - 64
    struct = re.search(r"typedef struct \{([^}]*)\} chip_gzip_plan_summary;", text).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = []
    for decl in struct.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"uint64_t": C.c_uint64, "int32_t": C.c_int32}[ctype]) for n in names.split(",")]
    assert fields == list(_GzipPlanSummary._fields_)
    assert C.sizeof(_GzipPlanSummary) == 32
    for name in ("gzip_plan", "gzip_members_decode", "gzip_members_read", "GzipPlanSummary", "GzipPlanStatus"):
        assert hasattr(compu_amd, name), name
    raw = _GzipPlanSummary(3, 4, 5, 4, -3)
    assert compu_amd.GzipPlanSummary(raw).as_tuple() == (3, 4, 5, 4, -3)
