"""The block description of one zstd frame on the host (chip_zstd_blocks_host): every record and the summary
against what each case of tests/zstd_parallel_cases.py built and against that file's reading of the headers in Python; the walk's
verdicts; frames of the system libzstd.  No GPU.  Without the entry point every test here fails at the missing symbol."""
import numpy as np
import pytest

import zstd_parallel_cases as P

CASES = P.all_cases()


def rows_of(blocks):
    """the records of zstd_blocks_host as the tuples of P.py_blocks"""
    return [(int(b["offset"]), int(b["size"]), int(b["lit_regen"]), int(b["lit_comp"]), int(b["n_seq"]), int(b["type"]), int(b["flags"]),
             int(b["lit_type"]), tuple(int(m) for m in b["mode"]), tuple(int(s) for s in b["src"])) for b in blocks]


def describe(data, max_blocks=None):
    import compu_amd

    blocks, summ = compu_amd.zstd_blocks_host(data, max_blocks)
    assert not blocks["pad"].any()
    return rows_of(blocks), summ.as_tuple()


def assert_matches_python(data):
    got = describe(data)
    want = P.py_blocks(data)
    assert got[1] == want[1]
    assert got[0] == want[0]
    return got


def test_record_layout():
    import ctypes as C

    import compu_amd
    from compu_amd.api import _ZstdBlock, _ZstdBlocksSummary

    assert C.sizeof(_ZstdBlock) == 48 == compu_amd.zstd_block_dtype().itemsize and C.sizeof(_ZstdBlocksSummary) == 48
    dt = compu_amd.zstd_block_dtype()
    for name in ("offset", "size", "lit_regen", "lit_comp", "n_seq", "type", "flags", "lit_type", "mode", "src"):
        assert dt.fields[name][1] == getattr(_ZstdBlock, name).offset, name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_blocks_are_what_the_case_built(case):
    rows, summ = assert_matches_python(case.frame)
    names = ("n_blocks", "in_used", "content_size", "window_size", "status", "descriptor", "header_bytes")
    for key, want in case.summary.items():
        assert summ[names.index(key)] == want, key
    assert len(rows) == len(case.rows)
    for k, (got, want) in enumerate(zip(rows, case.rows)):
        offset, size, lit_regen, lit_comp, n_seq, btype, flags, lit_type, modes, src = got
        assert (offset, size, btype, flags) == (want["offset"], want["size"], want["type"], P.LAST if want["last"] else 0), k
        assert src == want["src"], k
        if btype == P.COMPRESSED:
            assert (lit_type, lit_regen, n_seq, modes) == (want["lit_type"], want["lit_regen"], want["n_seq"], want["modes"]), k
            if "lit_comp" in want:
                assert lit_comp == want["lit_comp"], k
        else:
            assert (lit_type, lit_regen, lit_comp, n_seq, modes) == (0, 0, 0, 0, (0, 0, 0)), k


def test_offsets_and_sizes_against_block_cuts():
    import zstd_cases as Z

    seen = 0
    for c in Z.all_cases():
        if not isinstance(c.want, bytes) or c.frame[:4] != P.W.MAGIC:  # (the frames that decode: their headers are as the writer laid them)
            continue
        rows, summ = assert_matches_python(c.frame)
        assert summ[4] == P.OK and summ[0] == len(c.cuts) - 1 and summ[6] == c.cuts[0], c.name
        assert [r[0] for r in rows] == c.cuts[:-1], c.name
        assert summ[1] == c.cuts[-1] + (4 if summ[5] & 4 else 0) == len(c.frame), c.name
        seen += 1
    assert seen > 60


@pytest.mark.parametrize("name,frame,want", P.malformed_cases(), ids=[m[0] for m in P.malformed_cases()])
def test_section_headers_that_do_not_fit(name, frame, want):
    rows, summ = assert_matches_python(frame)
    assert summ[4] == P.OK
    assert [(r[6], r[7], r[2], r[3], r[4], r[8]) for r in rows] == want


def test_truncated_at_every_byte_of_a_three_block_frame():
    case = P.three_block_frame()
    cuts = [c.get("offset") for c in case.rows] + [len(case.frame) - 4]  # (the frame has a checksum)
    for n in range(len(case.frame)):
        rows, summ = assert_matches_python(case.frame[:n])
        assert summ[4] == P.TRUNCATED and summ[1] == 0, n
        whole = sum(1 for k in range(3) if cuts[k + 1] <= n)  # blocks whose header and body are in front of the cut
        assert summ[0] == whole == len(rows), n
    rows, summ = assert_matches_python(case.frame)
    assert summ[4] == P.OK and summ[1] == len(case.frame)
    # bytes behind the frame do not belong to it
    assert describe(case.frame + b"\xff" * 7) == (rows, summ)


@pytest.mark.parametrize("name,data,status,n", P.verdict_files(), ids=[v[0] for v in P.verdict_files()])
def test_walk_verdicts(name, data, status, n):
    rows, summ = assert_matches_python(data)
    assert (summ[4], summ[0], len(rows)) == (status, n, n)
    assert (summ[1] == 0) == (status != P.OK)


@pytest.mark.parametrize("name,data,status,n", P.block_cap_files(), ids=[v[0] for v in P.block_cap_files()])
def test_walk_follows_2_pow_20_blocks_and_no_more(name, data, status, n):
    import compu_amd

    blocks, summ = compu_amd.zstd_blocks_host(data)
    assert (int(summ.status), summ.n_blocks, len(blocks)) == (status, n, n)
    assert (blocks["offset"] == 6 + 3 * np.arange(n, dtype=np.uint64)).all() and (blocks["src"] == -1).all()
    assert int(blocks["flags"][-1]) == (P.LAST if status == P.OK else 0) and not blocks["flags"][:-1].any()


def test_counts_and_fills_part_of_a_frame():
    import ctypes as C

    import compu_amd
    from compu_amd.api import _ZstdBlocksSummary

    case = CASES[0]
    full = describe(case.frame)
    n = len(full[0])
    assert describe(case.frame, 0) == ([], full[1])
    for m in (1, n - 1, n, n + 3):
        assert describe(case.frame, m) == (full[0][:m], full[1])
    # nothing is written behind min(n_blocks, max_blocks) records
    lib = compu_amd.lib()
    buf = np.frombuffer(case.frame, np.uint8)
    room = np.full((n + 2) * 48, 0xEE, np.uint8)
    s = _ZstdBlocksSummary()
    assert lib.chip_zstd_blocks_host(buf.ctypes.data, buf.size, 3, room.ctypes.data, C.byref(s)) == 0
    assert (room[3 * 48:] == 0xEE).all() and rows_of(room[:3 * 48].view(compu_amd.zstd_block_dtype())) == full[0][:3]
    # arguments
    assert lib.chip_zstd_blocks_host(buf.ctypes.data, buf.size, 0, None, None) == -101
    assert lib.chip_zstd_blocks_host(None, 5, 0, None, C.byref(s)) == -101
    assert lib.chip_zstd_blocks_host(buf.ctypes.data, buf.size, 1, None, C.byref(s)) == -101
    assert lib.chip_zstd_blocks(buf.ctypes.data + 1, buf.size - 1, 0, None, C.byref(s), None) == -101  # misaligned: refused before the device
    assert lib.chip_zstd_blocks(None, 0, 0, None, C.byref(s), None) == 0 and s.status == P.TRUNCATED


def test_damaged_frames_are_read_as_the_python_reading_reads_them():
    """bytes of the small cases flipped, cut out and inserted, with the headers hit more often than the bodies: whatever the walk
    makes of them, both readings make the same of them"""
    import random

    rnd = random.Random(2718)
    small = [c.frame for c in CASES if len(c.frame) < 6000]
    statuses = set()
    for k in range(1500):
        data = bytearray(rnd.choice(small))
        cuts = [r[0] for r in P.py_blocks(bytes(data))[0]]
        for _ in range(rnd.randrange(1, 4)):
            at = rnd.choice(cuts) + rnd.randrange(0, 8) if cuts and rnd.random() < 0.7 else rnd.randrange(len(data))
            at = min(at, len(data) - 1)
            how = rnd.randrange(3)
            if how == 0:
                data[at] ^= 1 << rnd.randrange(8)
            elif how == 1:
                del data[at:at + rnd.randrange(1, 4)]
            else:
                data[at:at] = rnd.randbytes(rnd.randrange(1, 4))
        statuses.add(assert_matches_python(bytes(data))[1][4])
    assert statuses == {P.OK, P.TRUNCATED, P.BAD_HEADER}


def test_libzstd_frames_reach_treeless_blocks_and_repeat_modes(alice):
    """What the system libzstd writes for 1 to 2 MiB at levels 1, 3 and 19: every frame's description equals the Python reading,
    the block sizes add up to the input, and among them are treeless literals and Repeat modes with their sources."""
    import zstd_ref
    from bench_support import synth

    z = zstd_ref.load()
    assert z is not None
    contents = {"synth": synth.payloads(20, threads=2).tobytes(), "alice": (alice * 12)[:1500000]}
    treeless = repeat = 0
    for cname, data in contents.items():
        for level in (1, 3, 19):
            frame = zstd_ref.compress(z, data, level, True, True)
            rows, summ = assert_matches_python(frame)
            assert summ[4] == P.OK and summ[1] == len(frame) and summ[2] == len(data) and summ[3] > 128 * 1024, (cname, level)
            assert len(rows) >= len(data) // (128 * 1024)
            for i, r in enumerate(rows):
                _, _, _, _, n_seq, btype, flags, lit_type, modes, src = r
                assert not flags & P.MALFORMED
                if btype != P.COMPRESSED:
                    continue
                if lit_type == 3:
                    treeless += 1
                    assert 0 <= src[0] < i and rows[src[0]][7] == 2
                for k in range(3):
                    if n_seq and modes[k] == 3:
                        repeat += 1
                        assert 0 <= src[1 + k] < i and rows[src[1 + k]][4] > 0 and rows[src[1 + k]][8][k] != 3
    assert treeless > 0 and repeat > 0
