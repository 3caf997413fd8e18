"""chip_decode_batch_sizes without a GPU: the symbol, the argument checks (made before the device is looked for, as
chip_decode_batch_ex makes them), and the expected answers of the hand-built DEFLATE cases from the oracle, with the list of cases
the size pass may answer differently from a decode pinned to what its rule produces."""
import ctypes as C

import deflate_cases as K
import sizes_ref as R

E_NO_DEVICE, E_INVALID = -100, -101


def _call(lib, fmt, flags, n, ptrs):
    return lib.chip_decode_batch_sizes(fmt, flags, n, *ptrs, None)


def test_entry_point_is_exported_and_checks_arguments_before_the_device():
    import compu_amd

    lib = compu_amd.lib()
    assert hasattr(lib, "chip_decode_batch_sizes")
    none = [None] * 6
    for fmt in (-15, 15, 31, 47):
        assert _call(lib, fmt, 0, 0, none) == 0  # an empty batch is fine
        assert _call(lib, fmt, 1, 0, none) == E_INVALID  # flags must be 0, also for an empty batch
        assert _call(lib, fmt, 0x80000000, 1, none) == E_INVALID
        assert _call(lib, fmt, 0, 1, none) == E_INVALID  # null pointers
    for fmt in (100, 0):  # zstd, CHIP_FMT_DETECT
        assert _call(lib, fmt, 0, 0, none) == 0 and _call(lib, fmt, 1, 0, none) == E_INVALID and _call(lib, fmt, 0, 1, none) == E_INVALID
    # brotli: a size pass would be a full decode (include/compu_hip.h); an unknown format
    for fmt in (101, 12345):
        assert _call(lib, fmt, 0, 0, none) == E_INVALID
        assert _call(lib, fmt, 0, 1, none) == E_INVALID
    buf = (C.c_uint32 * 8)()
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(4)
    size, used, st = (C.c_uint64 * 1)(), (C.c_uint32 * 1)(), (C.c_int32 * 1)()
    ptrs = [C.cast(x, C.c_void_p) for x in (buf, off, ln, size, used, st)]
    misaligned = [C.c_void_p(C.addressof(buf) + 1)] + ptrs[1:]
    assert _call(lib, -15, 0, 1, misaligned) == E_INVALID
    assert _call(lib, -15, 0, 1 << 31, ptrs) == E_INVALID
    if lib.chip_device_count() == 0:  # (with a device these host pointers must not reach a kernel)
        assert _call(lib, -15, 0, 1, ptrs) == E_NO_DEVICE
        assert _call(lib, -15, 1, 1, ptrs) == E_INVALID  # the refusal comes first


def test_python_mirror_exists():
    import compu_amd

    assert callable(compu_amd.decode_batch_sizes)


def test_deflate_expectations_and_the_exception_list():
    cases = K.all_cases()
    assert len(cases) == 523
    exempt = {c.name for c in cases if R.by_rule_exempt(c)}
    assert exempt == R.DEFLATE_EXCEPTIONS == {"zlib_adler", "gzip_crc"}
    seen = set()
    for c in cases:
        st, size, used = R.expected(c)
        seen.add(st)
        if c.name in exempt:
            assert (st, size) == (R.FINISHED, len(c.content)) and used == len(c.data)
            continue
        assert (st, size) == R.oracle_triple(c)[:2]
        if isinstance(c.want, bytes):
            assert (st, size, used) == (R.FINISHED, len(c.want), len(c.data) - c.tail), c.name
        elif isinstance(c.want, K.Err):
            assert st == (R.NEED_DICT if c.want.code == 2 else c.want.code), c.name
        else:
            assert st == R.NEED_INPUT and used is None, c.name
    assert {R.FINISHED, R.NEED_INPUT, R.NEED_DICT, -3} <= seen


def test_zstd_expectations_and_the_exception_list():
    import zstd_cases as Z

    cases = Z.all_cases()
    exempt = {c.name for c in cases if R.zstd_exempt(c)}
    assert exempt == R.ZSTD_EXCEPTIONS
    tags_exact = set()
    for c in cases:
        e = R.zstd_expected(c)
        if e is None:
            continue
        st, size, used = e
        tags_exact |= c.tags
        if isinstance(c.want, bytes):
            assert (st, size) == (R.FINISHED, len(c.want)) and used is not None, c.name
        else:
            assert st == c.want, c.name
    # faults in headers, table descriptions, the sequence stream and offsets compare exactly, and so do valid frames of each kind
    for t in ("fcs_off_by_one", "bad_lit_size", "bad_weights", "bad_weight_12", "bad_accuracy", "bad_fse_symbol", "bad_seq_overread", "bad_seq_leftover",
              "bad_nseq", "bad_reserved_modes", "offset_past_start", "treeless_first", "window_nofcs", "single_fcs4", "rep_across_blocks", "ov1_ll0",
              "rle_ll", "rle_of", "rle_ml", "rep_ll_after_fse", "rep_of_after_rle"):
        assert t in tags_exact, t
