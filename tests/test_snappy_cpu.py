"""Snappy without a GPU: chip_snappy_block_decode_host and chip_snappy_chunks_host against tests/snappy_ref.py over the case lists
of tests/snappy_cases.py; the golden fixtures libsnappy wrote (tests/golden/snappy, tools/make_snappy_golden.py);
compu_amd/csrc/snappy_core.h in a stand-alone program under the address and undefined-behaviour sanitizers; the refusals that answer
before a device is looked for; and, where pyarrow imports, the cross-check with libsnappy.  Every test here but the reference's own
CRC check calls the library, so without the feature each fails at the missing symbol."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

import snappy_cases as K
import snappy_ref as R
import snappy_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TEXTS = ("10x10y", "alice29.txt")
BLOCK_STATUSES = {R.FINISHED, R.NEED_INPUT, R.NEED_OUTPUT, R.E_PREAMBLE, R.E_OFFSET, R.E_LENGTH}


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def cap_of(data, cap):
    return K.ample_block(data) if cap is None else cap


def test_reference_crc32c():
    assert R.crc32c(b"123456789") == 0xE3069283 and R.crc32c(b"") == 0
    assert R.mask(0) == 0xA282EAD8 and R.mask(0xFFFFFFFF) == (0xFFFFFFFF + 0xA282EAD8) & 0xFFFFFFFF


def test_host_block_decoder_equals_the_reference():
    from compu_amd import snappy

    seen = set()
    for name, data, cap in K.block_cases():
        cap = cap_of(data, cap)
        content, n, used, status = R.block_decode(data, cap)
        seen.add(status)
        assert snappy.snappy_block_decode_host(data, cap) == (content, used, status), name
    assert seen == BLOCK_STATUSES


def test_the_cases_answer_what_the_issue_says():
    """a few verdicts pinned by hand, so that the reference itself is held to the header's text"""
    by_name = {c[0]: c for c in K.block_cases()}
    ref = lambda name: R.block_decode(by_name[name][1], cap_of(by_name[name][1], by_name[name][2]))[1:]  # noqa: E731
    assert ref("block_00") == (0, 1, R.FINISHED)
    assert ref("block_00_and_a_byte") == (0, 1, R.E_LENGTH)
    assert ref("empty_input") == (0, 0, R.NEED_INPUT)
    assert ref("preamble_80_00") == (0, 2, R.FINISHED)
    assert ref("preamble_fifth_0f") == (0, 0, R.NEED_OUTPUT)
    assert R.block_decode(by_name["preamble_fifth_0f"][1], None)[1:] == (10, 16, R.NEED_INPUT)
    assert ref("preamble_fifth_10") == (0, 0, R.E_PREAMBLE)
    assert ref("lit_2pow32") == (0, 1, R.NEED_INPUT) and ref("lit_2pow32_behind") == (2, 4, R.NEED_INPUT)
    assert ref("n_one_too_few")[2] == R.NEED_INPUT and ref("n_one_too_much")[2] == R.E_LENGTH
    assert ref("cap0") == (0, 0, R.NEED_OUTPUT) and ref("cap139") == (0, 0, R.NEED_OUTPUT) and ref("cap140")[2] == R.FINISHED
    frames = {c[0]: c for c in K.frame_cases()}
    fref = lambda name: R.frame_decode(frames[name][1], K.ample_frame(frames[name][1]) if frames[name][2] is None else frames[name][2])[1:]  # noqa: E731
    assert fref("ident_alone") == (0, 10, R.FINISHED)
    assert fref("no_ident")[1:] == (0, R.E_HEADER) and fref("ident_wrong_length")[1:] == (0, R.E_HEADER)
    assert fref("three_chunks") == (1650, len(frames["three_chunks"][1]), R.FINISHED)
    assert fref("ident_repeated")[0::2] == (1650, R.FINISHED) and fref("ident_repeated_wrong")[0::2] == (700, R.E_HEADER)
    assert fref("compressed_65536")[2] == R.FINISHED and fref("compressed_65537")[2] == R.E_CHUNK_SIZE
    assert fref("uncompressed_65536")[2] == R.FINISHED and fref("uncompressed_65537")[2] == R.E_CHUNK_SIZE
    assert fref("type0_s3")[0::2] == (700, R.E_CHUNK_SIZE) and fref("reserved_02")[0::2] == (700, R.E_CHUNK)
    assert fref("reserved_and_cut")[0::2] == (700, R.NEED_INPUT)
    assert fref("bad_crc1")[0::2] == (700, R.E_CHECKSUM) and fref("crc_unmasked")[0::2] == (0, R.E_CHECKSUM)
    assert fref("block_cut_inside")[2] == R.E_BLOCK and fref("block_trailing_byte")[0::2] == (650 + 700, R.E_LENGTH)
    assert fref("damaged_then_cut")[2] == R.E_BLOCK and fref("too_large_and_bad_crc")[2] == R.E_CHUNK_SIZE
    assert fref("stated_too_large_no_room")[2] == R.E_CHUNK_SIZE
    assert fref("room699") == (0, 10, R.NEED_OUTPUT) and fref("room1349")[0::2] == (700, R.NEED_OUTPUT)


def test_host_block_decoder_arguments():
    import compu_amd

    lib = compu_amd.lib()
    ol, iu = C.c_uint64(9), C.c_uint64(9)
    one = C.create_string_buffer(b"\x00", 1)
    assert lib.chip_snappy_block_decode_host(one, 1, None, 0, C.byref(ol), C.byref(iu)) == R.FINISHED and (ol.value, iu.value) == (0, 1)
    assert lib.chip_snappy_block_decode_host(None, 0, None, 0, C.byref(ol), C.byref(iu)) == R.NEED_INPUT and (ol.value, iu.value) == (0, 0)
    assert lib.chip_snappy_block_decode_host(None, 1, None, 0, C.byref(ol), C.byref(iu)) == -101
    assert lib.chip_snappy_block_decode_host(one, 1, None, 1, C.byref(ol), C.byref(iu)) == -101
    assert lib.chip_snappy_block_decode_host(one, 1, None, 0, None, C.byref(iu)) == -101
    assert lib.chip_snappy_block_decode_host(one, 1 << 32, None, 0, C.byref(ol), C.byref(iu)) == -101


def rows_of(rec):
    return [tuple(int(v) for v in r)[:4] for r in rec.tolist()]


def test_host_walk_equals_the_reference():
    from compu_amd import snappy

    seen = set()
    for name, data, _ in K.frame_cases():
        want = R.chunks_walk(data)
        seen.add(want[1][3])
        rec, summ = snappy.snappy_chunks_host(data)
        assert (rows_of(rec), summ.as_tuple()) == want, name
        for m in sorted({0, 1, want[1][0]}):  # count-then-fill, and an early stop of the caller's
            rec, summ = snappy.snappy_chunks_host(data, m)
            assert (rows_of(rec), summ.as_tuple()) == R.chunks_walk(data, m), (name, m)
    assert seen == {R.OK, R.TRUNCATED, R.BAD_HEADER}
    assert snappy.snappy_chunk_dtype().itemsize == 24


def test_host_walk_too_large_and_refusals():
    import compu_amd
    from compu_amd import snappy
    from compu_amd._ffi import _SnappyChunksSummary, _SnappyParallelSummary

    data = R.IDENT + W.chunk(1, b"\0\0\0\0") * (R.MAX_BLOCKS + 1)
    rec, summ = snappy.snappy_chunks_host(data, 2)
    assert summ.as_tuple() == (R.MAX_BLOCKS, 0, 10 + 8 * R.MAX_BLOCKS, R.TOO_LARGE) and rows_of(rec) == [(10, 4, 1, 0), (18, 4, 1, 0)]
    lib, s = compu_amd.lib(), _SnappyChunksSummary()
    buf = C.create_string_buffer(data[:64], 64)
    assert lib.chip_snappy_chunks_host(buf, 64, 0, None, None) == -101
    assert lib.chip_snappy_chunks_host(None, 64, 0, None, C.byref(s)) == -101
    assert lib.chip_snappy_chunks_host(buf, 64, 1, None, C.byref(s)) == -101
    # the device forms and the batch calls refuse before they look for a device
    assert lib.chip_snappy_chunks(C.c_void_p(2), 64, 0, None, C.byref(s), None) == -101
    assert lib.chip_snappy_chunks(C.c_void_p(4), (1 << 40) + 1, 0, None, C.byref(s), None) == -101
    assert lib.chip_snappy_parallel(C.c_void_p(4), 64, None, 0, 1, C.byref(_SnappyParallelSummary()), None) == -101
    assert lib.chip_snappy_parallel(C.c_void_p(6), 64, None, 0, 0, C.byref(_SnappyParallelSummary()), None) == -101
    assert lib.chip_snappy_parallel(C.c_void_p(4), 64, None, 0, 0, None, None) == -101
    assert lib.chip_crc32c_batch(1, None, None, None, None, None) == -101
    assert lib.chip_crc32c_batch(0, None, None, None, None, None) == 0
    for fmt in (snappy.FMT_SNAPPY_BLOCK, snappy.FMT_SNAPPY):
        assert fmt in (104, 105)
        for flags in (1, 2, 3):
            assert lib.chip_decode_batch_ex(fmt, flags, 0, None, None, None, None, None, None, None, None, None, None) == -101
        assert lib.chip_decode_batch_sizes(fmt, 2, 0, None, None, None, None, None, None, None) == -101
        assert lib.chip_decode_batch_sizes(fmt, 0, 0, None, None, None, None, None, None, None) == 0
        assert lib.chip_decode_batch_ex(fmt, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0
        assert lib.chip_decoder_new(fmt, None) in (None, 0)  # the streaming objects do not take the tags
    assert lib.chip_detect(data[:4], 4) == 3  # Detection::Unknown: Snappy is never routed


def test_encode_entry_points_refuse_the_tags():
    """arguments that would pass for a format that encodes: the refusal is the tag's (chip_encode_batch_host looks for the device
    first, as it always has: tests/test_snappy_gpu.py asks it)"""
    import compu_amd

    lib = compu_amd.lib()
    buf = C.create_string_buffer(64)
    off, ln, st = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(16), (C.c_int32 * 1)(0)
    for fmt in (104, 105):
        assert lib.chip_encode_batch_ex(fmt, 1, 0, 1, buf, off, ln, buf, off, ln, ln, st, None) == -101
        assert lib.chip_encode_batch(fmt, 1, 1, buf, off, ln, buf, off, ln, ln, st, None) == -101


def test_golden_fixtures():
    """what libsnappy wrote through pyarrow 25 (snappy::RawCompress): the committed files, not pyarrow"""
    from compu_amd import snappy

    for name in TEXTS:
        data, blk = golden(name), golden(f"snappy/{name}.block")
        assert R.block_decode(blk, len(data)) == (data, len(data), len(blk), R.FINISHED)
        assert snappy.snappy_block_decode_host(blk, len(data)) == (data, len(blk), R.FINISHED)
        assert snappy.snappy_block_decode_host(blk, len(data) - 1) == (b"", 0, R.NEED_OUTPUT)
    assert 80000 <= len(golden("snappy/alice29.txt.block")) <= 100000


def test_core_under_the_sanitizers(tmp_path):
    """compu_amd/csrc/snappy_core.h in a stand-alone program built with the address and undefined-behaviour sanitizers: every case
    against the reference from exact-size heap buffers, every truncation and every single-byte change of three small inputs"""
    exe = str(tmp_path / "test_snappy_core")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_snappy_core.cpp")])
    blocks, frames = K.block_cases(), K.frame_cases()
    small = {}
    for k, (name, data, cap) in enumerate(blocks):
        cap = cap_of(data, cap)
        content, n, used, status = R.block_decode(data, cap)
        (tmp_path / f"b{k}.bin").write_bytes(data)
        (tmp_path / f"b{k}.want").write_bytes(struct.pack("<3Qi", cap, n, used, status) + content)
        if name == "copy_from_copy" or name.startswith("cut"):  # (the last cut: the longest prefix of the ~150-byte block)
            small["b_cut" if name.startswith("cut") else name] = f"b{k}"
    for k, (name, data, _) in enumerate(frames):
        rows, summ = R.chunks_walk(data)
        (tmp_path / f"f{k}.bin").write_bytes(data)
        (tmp_path / f"f{k}.want").write_bytes(struct.pack("<3QiI", *summ, 0) + b"".join(struct.pack("<Q4I", o, s, t, c, 0) for o, s, t, c in rows))
        if name.startswith("cut"):  # (the longest prefix of the ~250-byte stream)
            small["f_cut"] = f"f{k}"
    assert len(small) == 3, small
    out = subprocess.run([exe, str(tmp_path), str(len(blocks)), str(len(frames))] + sorted(small.values()), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test result: ok" in out.stdout, out.stdout + out.stderr
    print(out.stdout.strip())


# ---- the cross-check with libsnappy ----------------------------------------------------------------------------------------------


def libsnappy():
    try:
        import pyarrow
    except ImportError:
        pytest.skip("pyarrow does not import: the cross-check only")
    return pyarrow


def test_what_libsnappy_writes_decodes_to_the_same_bytes():
    from compu_amd import snappy

    pa = libsnappy()
    rng = random.Random(7)
    payloads = [K.text(rng.randrange(1, 3000), i) for i in range(396)] + [K.noise(500, 1), b"a" * 3000, K.text(70000, 5), golden("alice29.txt")]
    assert len(payloads) == 400
    for data in payloads:
        blk = pa.compress(data, codec="snappy", asbytes=True)
        assert snappy.snappy_block_decode_host(blk, len(data)) == (data, len(blk), R.FINISHED)
        assert R.block_decode(blk, len(data)) == (data, len(data), len(blk), R.FINISHED)


def preamble_bytes(blk):
    k = 0
    while blk[k] & 0x80:
        k += 1
    return k + 1


def test_damaged_blocks_against_libsnappy():
    """16 000 seeded mutations (a bit flip, a byte replaced, a byte deleted) of 400 short word-salad payloads compressed by
    libsnappy, applied BEHIND the preamble, so that the stated length stays fixed.  Each is accepted by both decoders with the
    same bytes, or rejected by both: zero disagreements, in both directions, no case left out."""
    from compu_amd import snappy

    pa = libsnappy()
    rng = random.Random(2024)
    accepted = rejected = 0
    for i in range(400):
        data = K.text(rng.randrange(20, 400), i)
        blk = pa.compress(data, codec="snappy", asbytes=True)
        pre = preamble_bytes(blk)
        for _ in range(40):
            m = bytearray(blk)
            kind, at = rng.randrange(3), rng.randrange(pre, len(blk))
            if kind == 0:
                m[at] ^= 1 << rng.randrange(8)
            elif kind == 1:
                m[at] = rng.randrange(256)
            else:
                del m[at]
            m = bytes(m)
            try:
                theirs = pa.decompress(m, len(data), codec="snappy", asbytes=True)
            except Exception:
                theirs = None
            content, used, status = snappy.snappy_block_decode_host(m, len(data))
            assert R.block_decode(m, len(data)) == (content, len(content), used, status)
            if theirs is None:
                assert status != R.FINISHED, (m.hex(), status)
                rejected += 1
            else:
                assert status == R.FINISHED and content == theirs, (m.hex(), status)
                accepted += 1
    print(f"{accepted + rejected} mutations: {accepted} accepted by both, {rejected} rejected by both")
    assert accepted + rejected == 16000 and accepted > 0 and rejected > 0
