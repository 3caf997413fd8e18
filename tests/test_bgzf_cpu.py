"""BGZF without a GPU: the exported symbols, the argument checks (made before the device is looked for), htslib's EOF marker,
chip_bgzf_plan_host against the walk restated in bgzf_cases.py, chip_encode_bound for CHIP_FMT_BGZF, and the Python mirrors."""
import ctypes as C
import gzip

import pytest

import bgzf_cases as B

E_NO_DEVICE, E_INVALID = -100, -101
FMT_BGZF = 131


def test_symbols_are_exported_and_arguments_are_checked_before_the_device():
    import compu_amd
    from compu_amd.api import _BgzfSummary

    lib = compu_amd.lib()
    for name in ("chip_bgzf_plan_host", "chip_bgzf_plan", "chip_bgzf_eof_block"):
        assert hasattr(lib, name)
    s = _BgzfSummary()
    buf = (C.c_uint32 * 16)()
    base = C.cast(buf, C.c_void_p)
    arr = [C.cast((C.c_uint64 * 4)(), C.c_void_p) for _ in range(4)]
    none = [None] * 4
    for call, tail in ((lib.chip_bgzf_plan_host, ()), (lib.chip_bgzf_plan, (None,))):
        assert call(base, 40, 0, *none, None, *tail) == E_INVALID  # no summary
        assert call(None, 40, 0, *none, C.byref(s), *tail) == E_INVALID  # no buffer, but a length
        assert call(base, 40, 1, *none, C.byref(s), *tail) == E_INVALID  # no arrays, but room asked for
        assert call(base, 40, 1, *arr[:3], None, C.byref(s), *tail) == E_INVALID
        s.n_blocks = s.total_out = s.in_used = s.status = s.eof = 9
        assert call(None, 0, 0, *none, C.byref(s), *tail) == 0  # an empty buffer is fine, also without a device
        assert (s.n_blocks, s.total_out, s.in_used, s.status, s.eof) == (0, 0, 0, 0, 0)
    misaligned = C.c_void_p(C.addressof(buf) + 2)
    assert lib.chip_bgzf_plan(misaligned, 40, 0, *none, C.byref(s), None) == E_INVALID
    if lib.chip_device_count() == 0:  # (with a device this host pointer must not reach a kernel)
        assert lib.chip_bgzf_plan(base, 40, 0, *none, C.byref(s), None) == E_NO_DEVICE
        assert lib.chip_bgzf_plan(base, 40, 1, *none, C.byref(s), None) == E_INVALID  # the refusal comes first


def test_eof_block_is_htslibs():
    import compu_amd

    n = C.c_size_t(0)
    p = compu_amd.lib().chip_bgzf_eof_block(C.byref(n))
    assert n.value == 28 and C.string_at(p, 28) == B.EOF == compu_amd.bgzf_eof_block()
    assert compu_amd.lib().chip_bgzf_eof_block(None)  # the length is optional
    assert gzip.decompress(B.EOF) == b""
    assert B.walk(B.EOF) == ([(0, 28, 0, 0)], (1, 0, 28, B.OK, 1))


@pytest.mark.parametrize("name,data", B.plan_files(), ids=[n for n, _ in B.plan_files()])
def test_plan_host_equals_the_walk(name, data):
    import compu_amd

    want_rows, want = B.walk(data)
    got_rows, got = B.host_plan(compu_amd.lib(), data, len(want_rows) + 2, len(want_rows) + 4)
    assert got == want and got_rows == want_rows
    base = name.split("@")[0]
    if base.startswith("cut") or base == "bsize_past_end":
        assert want[3] == B.TRUNCATED
    elif base in ("empty", "eof_only", "three_eof", "no_eof", "five_eof", "any_mtime_xfl_os") or base in B.geometry_files():
        assert want[3] == B.OK and want[4] == (0 if base in ("empty", "no_eof") else 1)
    else:
        assert want[3] == B.BAD_HEADER
    assert want[0] == (0 if "@0" in name else 3 if "@3" in name else want[0])  # the fault stops the walk where it sits


def test_plan_host_counts_and_fills_part_of_a_file():
    import compu_amd

    lib = compu_amd.lib()
    data = dict(B.fault_files())["five_eof"]
    all_rows, want = B.walk(data)
    assert want[0] == 6  # five blocks and the EOF marker
    for m in (0, 2, 6, 9):
        rows, got = B.host_plan(lib, data, m, 12)
        assert got == want and rows == all_rows[:m]
    in_off, in_len, out_off, out_cap, summ = compu_amd.bgzf_plan_host(data)
    assert list(zip(in_off.tolist(), in_len.tolist(), out_off.tolist(), out_cap.tolist())) == all_rows and summ.as_tuple() == want
    assert compu_amd.bgzf_plan_host(data, max_blocks=2)[0].tolist() == [r[0] for r in all_rows[:2]]
    assert compu_amd.bgzf_plan_host(b"")[4].as_tuple() == (0, 0, 0, 0, 0)


def test_plan_host_on_decoys_depth_and_large_blocks():
    """The files of the GPU tests through the host walk (their expectations are checked here once, without a device)."""
    import compu_amd

    lib = compu_amd.lib()
    for name, data in B.decoy_files().items():
        want_rows, want = B.walk(data)
        assert B.host_plan(lib, data, len(want_rows), len(want_rows) + 1) == (want_rows, want), name
        assert want[3] == (B.BAD_HEADER if name.endswith("at_0") else B.OK), name
        assert data.count(B.MAGIC) > want[0], name  # there are headers the walk never visits
    for data, payload in (B.deep_file(), B.large_file()):
        want_rows, want = B.walk(data)
        assert B.host_plan(lib, data, len(want_rows), len(want_rows) + 1) == (want_rows, want)
        assert want[1] == len(payload) and want[3:] == (B.OK, 1)
    data, _ = B.deep_file()
    assert len(data) % 4 != 0 and {r[0] % 16 for r in B.walk(data)[0]} == set(range(16))
    assert len(B.large_file()[0]) == 40 * 65311 + 28


def test_encode_bound_covers_a_stored_block():
    import compu_amd

    for n in (0, 1, 65280):
        stored = n + 5 * max(1, -(-n // 65535))
        assert compu_amd.encode_bound(FMT_BGZF, n) >= 26 + stored
        assert compu_amd.lib().chip_encode_bound(FMT_BGZF, n) >= 26 + stored
    assert compu_amd.FMT_BGZF == FMT_BGZF
    # the streaming encoder does not take the tag, and a batch refuses bad levels before it looks for a device
    opts = compu_amd.api._EncoderOpts(FMT_BGZF, 6, -1, 0, 0)
    assert not compu_amd.lib().chip_encoder_new(C.byref(opts))


def test_python_mirrors_exist():
    import compu_amd

    for name in ("bgzf_plan", "bgzf_plan_host", "bgzf_decode", "bgzf_eof_block", "BgzfSummary", "BgzfStatus"):
        assert hasattr(compu_amd, name), name
    assert callable(compu_amd.bgzf_plan) and callable(compu_amd.bgzf_decode)
