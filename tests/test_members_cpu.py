"""CHIP_F_MEMBERS without a GPU: the argument checks (made before the device is looked for), and the reference walk of
tests/members_ref.py against Python's standard library and the payloads the units were built from."""
import zlib

import members_cases as MC
import members_ref as R
from conftest import golden

E_INVALID = -101
F_COMPU_STATUS, F_MEMBERS = 1, 2
DEFLATE, ZLIB, GZIP, AUTO, ZSTD, BROTLI, DETECT = -15, 15, 31, 47, 100, 101, 0


def test_flag_constant_is_exported():
    import compu_amd

    assert compu_amd.F_MEMBERS == F_MEMBERS and compu_amd.F_COMPU_STATUS == F_COMPU_STATUS


def test_argument_checks_come_before_the_device():
    import compu_amd

    lib = compu_amd.lib()
    ex = lambda fmt, flags, n: lib.chip_decode_batch_ex(fmt, flags, n, *([None] * 9), None)
    sizes = lambda fmt, flags, n: lib.chip_decode_batch_sizes(fmt, flags, n, *([None] * 6), None)
    for call in (ex, sizes):
        for fmt in (GZIP, AUTO, ZSTD, DETECT):
            assert call(fmt, F_MEMBERS, 0) == 0  # accepted: an empty batch is fine
            assert call(fmt, F_MEMBERS, 1) == E_INVALID  # null pointers
            assert call(fmt, F_MEMBERS | F_COMPU_STATUS, 0) == E_INVALID  # compu has no multi-member decode to mirror
            assert call(fmt, F_MEMBERS | 4, 0) == E_INVALID and call(fmt, F_MEMBERS | 0x80000000, 0) == E_INVALID
        for fmt in (DEFLATE, ZLIB, BROTLI):
            assert call(fmt, F_MEMBERS, 0) == E_INVALID  # no concatenation convention
        assert call(12345, F_MEMBERS, 0) == E_INVALID
    # what was pinned before still holds
    assert ex(DEFLATE, 2, 1) == E_INVALID
    assert sizes(GZIP, F_COMPU_STATUS, 0) == E_INVALID and sizes(GZIP, 0x80000000, 1) == E_INVALID and sizes(GZIP, 0, 0) == 0
    assert ex(GZIP, F_COMPU_STATUS, 0) == 0


def _stdlib_gzip(unit):
    """gzip -d as the standard library spells it: a decompressobj per member, over unused_data"""
    out, rest, used = b"", unit, 0
    while rest[:2] == b"\x1f\x8b":
        d = zlib.decompressobj(31)
        out += d.decompress(rest)
        assert d.eof
        used += len(rest) - len(d.unused_data)
        rest = d.unused_data
    return out, used


def test_reference_walk_equals_the_stdlib_on_valid_gzip_units():
    seen = 0
    for c in MC.shape_cases() + MC.tail_cases():
        if c.fmt == R.ZSTD or not c.unit.startswith(b"\x1f\x8b"):
            continue
        try:
            want, used = _stdlib_gzip(c.unit)
        except (zlib.error, AssertionError):
            continue  # (a damaged or cut member: the walk's own tests below)
        a = R.walk(c.fmt, c.unit, len(want) + 64)
        assert (a.status, a.out_len, a.in_used, a.data) == (R.FINISHED, len(want), used, want), c.name
        seen += 1
    assert seen >= 30


def test_reference_walk_on_zstd_concatenations():
    alice, xy = golden("alice29.txt"), golden("10x10y")
    az, xz = golden("alice29.txt.compressed.zstd"), golden("10x10y.compressed.zstd")
    f1, p1 = MC.zframe(MC.payload(1000, 1), checksum=True)
    f2, p2 = MC.zframe(b"q" * 77, kind="rle")
    unit, want = az + f1 + xz + f2 + az, alice + p1 + xy + p2 + alice
    a = R.walk(R.ZSTD, unit, len(want))
    assert (a.status, a.out_len, a.in_used, a.members) == (R.FINISHED, len(want), len(unit), 5) and a.data == want
    a = R.walk(R.ZSTD, unit + b"\x28\xb5\x2f", len(want))  # stray bytes are not a frame
    assert (a.status, a.in_used) == (R.FINISHED, len(unit))
    a = R.walk(R.ZSTD, unit, len(want) - 1)
    assert a.status == R.NEED_OUTPUT and a.out_len <= len(want) - 1 and a.data == want[:a.out_len]


def test_reference_walk_verdicts():
    by = {c.name: c for c in MC.all_cases()}
    w = lambda name: R.walk(by[name].fmt, by[name].unit, by[name].cap if by[name].cap is not None else 1 << 20)
    assert w("gzip_then_magic_only").status == R.NEED_INPUT and w("gzip_then_magic_only").in_used == len(by["gzip_then_magic_only"].unit)
    assert w("gzip_then_bad_method").status == -3 and w("gzip_then_reserved_flag").status == -3
    for name in ("gzip_then_zero7", "gzip_then_lone_1f", "gzip_then_zlib_behind"):
        a = w(name)
        assert a.status == R.FINISHED and a.members == 1 and a.in_used < len(by[name].unit), name
    assert w("auto_zlib_then_gzip").members == 1
    assert w("gzip_distance_to_member_start").status == R.FINISHED and w("gzip_distance_past_member_start").status == -3
    assert w("zstd_offset_to_frame_start").status == R.FINISHED and w("zstd_offset_past_frame_start").status == -20
    for ov in (1, 2, 3):
        assert w(f"zstd_repeat_offset_{ov}").status == R.FINISHED
    for name in ("gzip_empty_unit", "zstd_empty_unit"):  # in_len == 0 answers as without the flag: truncated
        assert tuple(w(name)[:3]) == (R.NEED_INPUT, 0, 0), name
    a = w("zstd_skippable_alone")
    assert (a.status, a.out_len, a.in_used) == (R.FINISHED, 0, len(by["zstd_skippable_alone"].unit))
    for k in (1, 2, 3):
        a, clean = w(f"gzip_bad_crc_in_{k}"), R.walk(R.GZIP, b"".join(MC.gz(d) for d in (MC.payload(700, 31), MC.payload(40000, 32), MC.payload(65, 33))), 1 << 20)
        assert a.status == -3 and a.members == k and a.data == clean.data[:a.out_len]
        assert w(f"zstd_bad_xxh64_in_{k}").status == -22 and w(f"zstd_bad_block_in_{k}").status == -20
    assert w("gzip_cap_total").status == R.FINISHED and w("zstd_cap_total").status == R.FINISHED
    for name in ("gzip_cap_total_less_1", "gzip_cap_member1", "gzip_cap_zero", "zstd_cap_total_less_1", "zstd_cap_member1", "zstd_cap_zero"):
        assert w(name).status == R.NEED_OUTPUT, name
