"""The file writer without a GPU: every argument check of chip_pack_units and chip_encode_file (made before the device is looked
for), chip_encode_file_bound against its formula restated in file_cases.py, and the seek-table parser the GPU tests rely on, on a
hand-built table and on damaged ones.  Without the feature every test that touches the library fails at the missing symbols."""
import ctypes as C
import struct

import pytest

import file_cases as F
from file_cases import FMT_BGZF, FMT_GZIP, FMT_ZSTD, W_SEEK_TABLE

E_NO_DEVICE, E_INVALID = -100, -101


def new_summary(fill=9):
    from compu_amd.api import _FileSummary

    return _FileSummary(fill, fill, fill, fill, fill)


def test_pack_units_checks_its_arguments_before_the_device():
    import compu_amd

    lib = compu_amd.lib()
    arr = [C.cast((C.c_uint64 * 8)(), C.c_void_p) for _ in range(5)]
    src, off, ln, dst, doff = arr
    total = C.c_uint64(9)
    assert lib.chip_pack_units(4, src, off, ln, dst, 64, doff, None, None) == E_INVALID  # no total
    assert lib.chip_pack_units(4, None, off, ln, dst, 64, doff, C.byref(total), None) == E_INVALID
    assert lib.chip_pack_units(4, src, None, ln, dst, 64, doff, C.byref(total), None) == E_INVALID
    assert lib.chip_pack_units(4, src, off, None, dst, 64, doff, C.byref(total), None) == E_INVALID
    assert lib.chip_pack_units(4, src, off, ln, None, 64, doff, C.byref(total), None) == E_INVALID  # room, but no destination
    assert lib.chip_pack_units(1 << 32, src, off, ln, dst, 64, doff, C.byref(total), None) == E_INVALID
    total.value = 9
    assert lib.chip_pack_units(0, None, None, None, None, 0, None, C.byref(total), None) == 0 and total.value == 0  # no unit: no device needed
    total.value = 9
    assert lib.chip_pack_units(0, src, off, ln, dst, 64, doff, C.byref(total), None) == 0 and total.value == 0
    if lib.chip_device_count() == 0:  # (with a device these host pointers must not reach a kernel)
        assert lib.chip_pack_units(4, src, off, ln, dst, 64, doff, C.byref(total), None) == E_NO_DEVICE
        assert lib.chip_pack_units(4, src, off, ln, dst, 64, None, C.byref(total), None) == E_NO_DEVICE  # dst_off is optional
        assert lib.chip_pack_units(4, src, off, ln, None, 0, None, C.byref(total), None) == E_NO_DEVICE  # so is a destination without room
        assert lib.chip_pack_units((1 << 32) - 1, src, off, ln, dst, 64, doff, C.byref(total), None) == E_NO_DEVICE
        assert lib.chip_pack_units(4, src, off, ln, None, 64, doff, C.byref(total), None) == E_INVALID  # the refusal comes first


def test_encode_file_checks_its_arguments_before_the_device():
    import compu_amd

    lib = compu_amd.lib()
    buf = (C.c_uint32 * 64)()
    base, out = C.cast(buf, C.c_void_p), C.cast((C.c_uint32 * 64)(), C.c_void_p)
    misaligned = C.c_void_p(C.addressof(buf) + 2)
    s = new_summary()
    ok = dict(fmt=FMT_GZIP, level=6, unit=0, flags=0, inp=base, n=100, out=out, cap=256, summ=C.byref(s))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.chip_encode_file(a["fmt"], a["level"], a["unit"], a["flags"], a["inp"], a["n"], a["out"], a["cap"], a["summ"], None)

    refused = [
        dict(summ=None), dict(inp=None), dict(inp=misaligned), dict(out=None), dict(n=(1 << 40) + 1),
        dict(unit=1, n=1 << 31),  # 2^31 units
        dict(fmt=101), dict(fmt=-15), dict(fmt=15), dict(fmt=47), dict(fmt=0), dict(fmt=12345),  # brotli, deflate, zlib, auto, detect
        dict(level=10), dict(level=-2), dict(fmt=FMT_BGZF, level=10), dict(fmt=FMT_BGZF, level=-2),
        dict(fmt=FMT_ZSTD, level=131073), dict(fmt=FMT_ZSTD, level=-131073),
        dict(fmt=FMT_BGZF, unit=65281), dict(unit=(1 << 30) + 1), dict(fmt=FMT_ZSTD, unit=(1 << 30) + 1),
        dict(flags=2), dict(flags=0x80000000), dict(fmt=FMT_ZSTD, flags=3),
        dict(flags=W_SEEK_TABLE), dict(fmt=FMT_BGZF, flags=W_SEEK_TABLE),  # the seek table is zstd's
        dict(fmt=FMT_ZSTD, flags=W_SEEK_TABLE, unit=1, n=0x8000001),  # more frames than the table's format allows
    ]
    for kw in refused:
        assert call(**kw) == E_INVALID, kw
    if lib.chip_device_count() == 0:  # (with a device these host pointers must not reach a kernel)
        accepted = [
            dict(), dict(level=-1), dict(level=0), dict(level=9), dict(fmt=FMT_BGZF), dict(fmt=FMT_BGZF, unit=65280), dict(fmt=FMT_ZSTD, level=-131072),
            dict(fmt=FMT_ZSTD, level=131072, flags=W_SEEK_TABLE), dict(unit=1 << 30), dict(n=1 << 40), dict(unit=1, n=(1 << 31) - 1),
            dict(fmt=FMT_ZSTD, flags=W_SEEK_TABLE, unit=1, n=0x8000000), dict(fmt=FMT_ZSTD, unit=1, n=0x8000001),
            dict(inp=None, n=0), dict(out=None, cap=0),
        ]
        for kw in accepted:
            assert call(**kw) == E_NO_DEVICE, kw
        assert call(fmt=FMT_ZSTD, flags=2) == E_INVALID  # the refusal comes first


@pytest.mark.parametrize("fmt,flags", [(FMT_BGZF, 0), (FMT_GZIP, 0), (FMT_ZSTD, 0), (FMT_ZSTD, W_SEEK_TABLE)])
def test_file_bound_is_its_formula(fmt, flags):
    import compu_amd

    lib = compu_amd.lib()
    for unit_bytes in (0, 1000, 1, F.BGZF_PAYLOAD):
        unit = F.unit_of(fmt, unit_bytes)
        for length in (0, 1, unit - 1, unit, unit + 1, 3 * unit):
            want = F.file_bound(lib, fmt, unit_bytes, flags, length)
            assert lib.chip_encode_file_bound(fmt, unit_bytes, flags, length) == want, (unit_bytes, length)
            assert compu_amd.encode_file_bound(fmt, length, unit_bytes, flags) == want
    # spelled out once: three full blocks and the EOF block; one empty member; one empty frame and a table of one entry
    if fmt == FMT_BGZF:
        assert lib.chip_encode_file_bound(fmt, 0, 0, 3 * 65280) == 3 * lib.chip_encode_bound(fmt, 65280) + 28
        assert lib.chip_encode_file_bound(fmt, 0, 0, 0) == 28
    else:
        assert lib.chip_encode_file_bound(fmt, 0, flags, 0) == lib.chip_encode_bound(fmt, 0) + (25 if flags else 0)
        assert lib.chip_encode_file_bound(fmt, 0, flags, 262145) == lib.chip_encode_bound(fmt, 262144) + lib.chip_encode_bound(fmt, 1) + (33 if flags else 0)


def test_file_bound_is_zero_for_what_encode_file_refuses():
    import compu_amd

    bound = compu_amd.lib().chip_encode_file_bound
    assert bound(101, 0, 0, 100) == 0 and bound(-15, 0, 0, 100) == 0 and bound(15, 0, 0, 100) == 0  # brotli, deflate, zlib
    assert bound(FMT_BGZF, 65281, 0, 100) == 0 and bound(FMT_GZIP, (1 << 30) + 1, 0, 100) == 0
    assert bound(FMT_GZIP, 0, W_SEEK_TABLE, 100) == 0 and bound(FMT_ZSTD, 0, 2, 100) == 0
    assert bound(FMT_GZIP, 0, 0, (1 << 40) + 1) == 0 and bound(FMT_GZIP, 1, 0, 1 << 31) == 0
    assert bound(FMT_ZSTD, 1, W_SEEK_TABLE, 0x8000001) == 0 and bound(FMT_ZSTD, 1, 0, 0x8000001) != 0
    assert bound(FMT_GZIP, 0, 0, 1 << 40) > 1 << 40


def test_seek_table_parser():
    entries = [(100, 1000), (7, 0), (0xFFFFFFFF, 0x40000000)]
    table = F.seek_table(entries)
    assert len(table) == 17 + 8 * 3
    assert table == (bytes.fromhex("5e2a4d18") + struct.pack("<I", 33) + struct.pack("<6I", 100, 1000, 7, 0, 0xFFFFFFFF, 0x40000000)
                     + struct.pack("<I", 3) + b"\0" + bytes.fromhex("b1ea928f"))
    assert F.parse_seek_table(table, 0) == entries
    assert F.parse_seek_table(b"frames" + table, 6) == entries
    assert F.parse_seek_table(F.seek_table([]), 0) == []
    damaged = {
        "wrong magic": table[:-4] + struct.pack("<I", F.SEEKABLE_MAGIC ^ 1),
        "wrong skippable magic": struct.pack("<I", F.SKIPPABLE_MAGIC - 1) + table[4:],
        "wrong Frame_Size": table[:4] + struct.pack("<I", 34) + table[8:],
        "reserved bit": F.seek_table(entries, descriptor=0x04),
        "cut": table[:-1],
        "an entry too many": table + b"\0" * 8,
    }
    for why, t in damaged.items():
        with pytest.raises(ValueError):
            F.parse_seek_table(t, 0)
    with pytest.raises(ValueError):
        F.parse_seek_table(table, 1)


def test_python_mirrors_exist():
    import compu_amd

    for name in ("pack_units", "encode_file", "encode_file_bound", "bgzf_write", "FileSummary", "FileStatus", "W_SEEK_TABLE"):
        assert hasattr(compu_amd, name), name
    assert compu_amd.W_SEEK_TABLE == W_SEEK_TABLE and int(compu_amd.FileStatus.NeedOutput) == F.FILE_NEED_OUTPUT
    raw = new_summary(0)
    raw.n_units, raw.out_len, raw.table_off, raw.status = 3, 100, 59, 1
    assert compu_amd.FileSummary(raw).as_tuple() == (3, 100, 59, 1)
