"""The zstd frame index without a GPU: chip_zstd_plan_host against the walk restated in zstd_plan_cases.py (rows, summary, nothing
written behind min(n, max)), against libzstd's own frame arithmetic, the argument checks of the three entry points (made before
the device is looked for), and the Python mirrors.  Without the feature every test here fails at the missing symbols."""
import ctypes as C

import numpy as np
import pytest

import zstd_plan_cases as Z
import zstd_ref

LIBZSTD = zstd_ref.load()
E_NO_DEVICE, E_INVALID = -100, -101


def _ids(files):
    return [n for n, _ in files]


@pytest.mark.parametrize("name,data", Z.all_files(), ids=_ids(Z.all_files()))
def test_plan_host_equals_the_walk(name, data):
    import compu_amd

    want_rows, want = Z.walk(data)
    got_rows, got = Z.host_plan(compu_amd.lib(), data, len(want_rows) + 2, len(want_rows) + 4)
    assert got == want and got_rows == want_rows


def test_the_walk_stops_where_the_cases_say():
    """the expectations themselves, pinned once: status, in_used and counts of named cases"""
    files = dict(Z.all_files())
    lead = files["cut_in_magic_1@3"][:-1]
    n_lead = (3, 1, 1, 200 + 3000, len(lead))  # three frames (one unsized), one skippable frame, in front of every @3 stop
    assert Z.walk(lead)[1] == n_lead + (Z.OK,)
    want = {"empty": Z.OK, "skippable_alone": Z.OK, "pzstd_style": Z.OK, "trailing_4_no_magic": Z.BAD_HEADER, "trailing_gzip": Z.BAD_HEADER,
            "near_magic": Z.BAD_HEADER, "skippable_range_end": Z.BAD_HEADER, "skippable_range_start": Z.BAD_HEADER, "block_type_3": Z.BAD_HEADER,
            "block_type_3_first": Z.BAD_HEADER, "fcs_ffffffff": Z.TOO_LARGE, "fcs8_2_pow_32": Z.TOO_LARGE, "fcs_ffffffff_cut": Z.TRUNCATED,
            "skippable_size_past_end": Z.TRUNCATED}
    for name, data in Z.stop_files():
        base, at = name.split("@") if "@" in name else (name, None)
        if at is None:
            continue
        status = want.get(base, Z.TRUNCATED)  # every cut, every stray byte
        summ = Z.walk(data)[1]
        assert summ == ((0, 0, 0, 0, 0) if at == "0" else n_lead) + (status,), name  # in_used is the start of the frame the walk stopped at
    assert Z.walk(files["fcs_fffffffe_is_fine"])[1][5] == Z.OK
    assert Z.walk(files["skippable_every_magic"])[1][:2] == (4, 16)
    assert Z.walk(files["pzstd_style"])[1][:3] == (4, 4, 1)
    rows, summ = Z.walk(files["fcs2_plus256"])
    assert rows == [(0, len(files["fcs2_plus256"]), 0, 256)] and files["fcs2_plus256"][5:7] == b"\0\0"
    assert Z.walk(files["dict_id_widths"])[1][:3] == (4, 0, 1)
    for name, data in Z.decoy_files().items():
        rows, summ = Z.walk(data)
        n_magic = sum(data.count((0x184D2A50 | k).to_bytes(4, "little")) for k in range(16)) + data.count(Z.MAGIC)
        assert n_magic > summ[0] + summ[1], name  # there are magic numbers the walk never visits
        assert summ[5] == (Z.BAD_HEADER if name.startswith("first_candidate") else Z.OK), name
    assert Z.walk(files["frame_at_end_of_last_block"])[1][:2] == (3, 1)
    for name, data in Z.geometry_files().items():
        assert Z.walk(data)[1][5] == (Z.TRUNCATED if "last_4_bytes" in name else Z.BAD_HEADER if name.startswith("stray_byte") else Z.OK), name
    assert Z.walk(files["nine_x_3000"])[1] == (3000, 0, 0, 0, 27000, Z.OK) and Z.walk(files["nine_x_3000_mixed"])[1][:3] == (2000, 1000, 1000)
    starts = {r[0] % 16 for n in range(4) for r in Z.walk(files[f"chunk_boundary_shift_{n}"])[0]}
    assert {0, 13, 14, 15} <= starts
    assert [Z.walk(files[f"tile_boundary_shift_{n}"])[0][1][0] for n in (1, 2, 3)] == [16383, 16382, 16381]


@pytest.mark.parametrize("name,data", Z.block_cap_files(), ids=_ids(Z.block_cap_files()))
def test_plan_host_follows_2_pow_20_blocks_and_no_more(name, data):
    import compu_amd

    want_rows, want = Z.walk(data)
    assert Z.host_plan(compu_amd.lib(), data, 4, 5) == (want_rows, want)
    if name.endswith("plus_1"):
        assert want == (1, 0, 0, 0, 9, Z.TOO_LARGE)
    else:
        assert want == (3, 0, 1, 0, len(data), Z.OK) and want_rows[1][1] == 6 + 3 * Z.MAX_BLOCKS


def test_plan_host_counts_and_fills_part_of_a_buffer():
    import compu_amd

    lib = compu_amd.lib()
    data = dict(Z.all_files())["mixed_sized_unsized"]
    all_rows, want = Z.walk(data)
    assert want[:3] == (6, 0, 4)
    for m in (0, 2, 6, 9):
        rows, got = Z.host_plan(lib, data, m, 12)
        assert got == want and rows == all_rows[:m]
    in_off, in_len, out_off, out_cap, summ = compu_amd.zstd_plan_host(data)
    assert list(zip(in_off.tolist(), in_len.tolist(), out_off.tolist(), out_cap.tolist())) == all_rows and summ.as_tuple() == want
    assert out_cap[0] == compu_amd.ZPLAN_UNSIZED == Z.UNSIZED
    assert compu_amd.zstd_plan_host(data, max_frames=2)[0].tolist() == [r[0] for r in all_rows[:2]]
    assert compu_amd.zstd_plan_host(b"")[4].as_tuple() == (0, 0, 0, 0, 0, 0)
    assert compu_amd.zstd_plan_host(np.frombuffer(data, np.uint8))[4].as_tuple() == want


@pytest.mark.skipif(LIBZSTD is None, reason="no system libzstd to cross-check against")
def test_in_len_and_out_cap_are_libzstds_on_its_own_frames(alice):
    """ZSTD_findFrameCompressedSize and ZSTD_getFrameContentSize on every frame libzstd wrote: several levels, with and without
    checksum and content size, empty input, several blocks; the golden files among them"""
    import compu_amd
    from conftest import golden

    z = LIBZSTD
    z.ZSTD_findFrameCompressedSize.restype = C.c_size_t
    z.ZSTD_findFrameCompressedSize.argtypes = [C.c_void_p, C.c_size_t]
    z.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    z.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
    rnd = np.random.default_rng(3).integers(0, 256, 300000, dtype=np.uint8).tobytes()  # incompressible: raw blocks, three of them
    frames = [golden("alice29.txt.compressed.zstd"), golden("10x10y.compressed.zstd")]
    for k, data in enumerate((b"", b"a", alice[:100], alice[:5000], alice, rnd, b"z" * 200000, alice[:70000])):
        frames.append(zstd_ref.compress(z, data, level=(1, 3, 9, 19)[k % 4], checksum=bool(k & 1), content_size=bool(k & 2) or k % 3 == 0))
    buf = b"".join(frames)
    in_off, in_len, out_off, out_cap, summ = compu_amd.zstd_plan_host(buf)
    assert summ.as_tuple()[:2] == (len(frames), 0) and summ.status == 0 and summ.in_used == len(buf) and 0 < summ.n_unsized < len(frames)
    src = C.create_string_buffer(buf, len(buf))
    for i in range(len(frames)):
        at = C.c_void_p(C.addressof(src) + int(in_off[i]))
        assert int(in_len[i]) == z.ZSTD_findFrameCompressedSize(at, len(buf) - int(in_off[i])) == len(frames[i]), i
        size = z.ZSTD_getFrameContentSize(at, len(buf) - int(in_off[i]))
        assert int(out_cap[i]) == (Z.UNSIZED if size == 2 ** 64 - 1 else size), i  # ZSTD_CONTENTSIZE_UNKNOWN
    assert (Z.walk(buf)[0], Z.walk(buf)[1]) == (list(zip(in_off.tolist(), in_len.tolist(), out_off.tolist(), out_cap.tolist())), summ.as_tuple())


def test_arguments_are_checked_before_the_device():
    import compu_amd

    lib = compu_amd.lib()
    for name in ("chip_zstd_plan_host", "chip_zstd_plan", "chip_layout_units"):
        assert hasattr(lib, name)
    s = Z.new_summary()
    buf = (C.c_uint32 * 16)()
    base = C.cast(buf, C.c_void_p)
    arr = [C.cast((C.c_uint64 * 4)(), C.c_void_p) for _ in range(4)]
    none = [None] * 4
    for call, tail in ((lib.chip_zstd_plan_host, ()), (lib.chip_zstd_plan, (None,))):
        assert call(base, 40, 0, *none, None, *tail) == E_INVALID  # no summary
        assert call(None, 40, 0, *none, C.byref(s), *tail) == E_INVALID  # no buffer, but a length
        assert call(base, 40, 1, *none, C.byref(s), *tail) == E_INVALID  # no arrays, but room asked for
        assert call(base, 40, 1, *arr[:3], None, C.byref(s), *tail) == E_INVALID
        s.n_frames = s.n_skippable = s.n_unsized = s.total_out = s.in_used = s.status = 9
        assert call(None, 0, 0, *none, C.byref(s), *tail) == 0  # an empty buffer is fine, also without a device
        assert (s.n_frames, s.n_skippable, s.n_unsized, s.total_out, s.in_used, s.status, s.pad) == (0, 0, 0, 0, 0, 0, 0)
    misaligned = C.c_void_p(C.addressof(buf) + 2)
    assert lib.chip_zstd_plan(misaligned, 40, 0, *none, C.byref(s), None) == E_INVALID
    assert lib.chip_zstd_plan(base, (1 << 40) + 1, 0, *none, C.byref(s), None) == E_INVALID
    total, over = C.c_uint64(9), C.c_uint64(9)
    assert lib.chip_layout_units(4, arr[0], arr[1], arr[2], None, C.byref(over), None) == E_INVALID
    assert lib.chip_layout_units(4, arr[0], arr[1], arr[2], C.byref(total), None, None) == E_INVALID
    assert lib.chip_layout_units(4, None, arr[1], arr[2], C.byref(total), C.byref(over), None) == E_INVALID
    assert lib.chip_layout_units(4, arr[0], None, arr[2], C.byref(total), C.byref(over), None) == E_INVALID
    assert lib.chip_layout_units(4, arr[0], arr[1], None, C.byref(total), C.byref(over), None) == E_INVALID
    assert lib.chip_layout_units(4, arr[0], arr[0], arr[2], C.byref(total), C.byref(over), None) == E_INVALID  # in place
    assert lib.chip_layout_units(1 << 32, arr[0], arr[1], arr[2], C.byref(total), C.byref(over), None) == E_INVALID
    assert lib.chip_layout_units(0, None, None, None, C.byref(total), C.byref(over), None) == 0  # no unit: no device needed
    assert (total.value, over.value) == (0, 0)
    if lib.chip_device_count() == 0:  # (with a device these host pointers must not reach a kernel)
        assert lib.chip_zstd_plan(base, 40, 0, *none, C.byref(s), None) == E_NO_DEVICE
        assert lib.chip_zstd_plan(base, 40, 1, *none, C.byref(s), None) == E_INVALID  # the refusal comes first
        assert lib.chip_layout_units(4, arr[0], arr[1], arr[2], C.byref(total), C.byref(over), None) == E_NO_DEVICE


def test_python_mirrors_exist():
    import compu_amd

    for name in ("zstd_plan", "zstd_plan_host", "layout_units", "zstd_frames_decode", "ZstdPlanSummary", "ZstdPlanStatus", "ZPLAN_UNSIZED"):
        assert hasattr(compu_amd, name), name
    assert [s.value for s in compu_amd.ZstdPlanStatus] == [Z.OK, Z.TRUNCATED, Z.BAD_HEADER, Z.TOO_LARGE]
