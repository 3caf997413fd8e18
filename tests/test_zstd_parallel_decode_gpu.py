"""chip_zstd_parallel against the one-unit chip_decode_batch(CHIP_FMT_ZSTD) on the same buffer: path, bytes,
out_len, in_used and status, into a poisoned output whose bytes behind out_len must stay as they were; for hand-built frames
(tests/zstd_writer.py) also the writer's own content.  Without the feature every test here fails at the missing symbol."""
import ctypes as C
import random

import numpy as np
import pytest

import zstd_parallel_cases as P
import zstd_writer as W
from zstd_writer import new_offset as N

pytestmark = pytest.mark.gpu

FMT_ZSTD, FINISHED, NEED_OUTPUT = 100, 2, 1
SERIAL, PARALLEL, REFUSED = 0, 1, 2
NO_CHECKSUM, ROUNDS_MAX = 1, 40
POISON, SLACK = 0xC7, 64


def upload(torch, data):
    t = torch.full(((len(data) + 3) // 4 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


def batch(torch, data, cap):
    """the one-unit batch decode: (bytes, out_len, in_used, status)"""
    import compu_amd

    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda").to(torch.int32)  # noqa: E731
    out = torch.full((cap + SLACK,), POISON, dtype=torch.uint8, device="cuda")
    ol, iu, st = compu_amd.decode_batch(FMT_ZSTD, upload(torch, data), i64(0), i32(len(data)), out, i64(0), i32(cap))
    torch.cuda.synchronize()
    n = int(ol[0]) & 0xFFFFFFFF
    return out.cpu().numpy()[:n].tobytes(), n, int(iu[0]) & 0xFFFFFFFF, int(st[0])


def par(torch, data, cap, flags=0, wlog=0, null_out=False):
    """chip_zstd_parallel into a poisoned room of cap + SLACK bytes: (bytes, summary).  Nothing behind out_len is touched on the parallel
    path; the serial path is the batch kernel, which uses the room up to `cap` while it decodes, and nothing behind that"""
    import compu_amd
    from compu_amd.api import _ZstdParallelSummary

    d_in = upload(torch, data)
    out = torch.full((cap + SLACK,), POISON, dtype=torch.uint8, device="cuda")
    s = _ZstdParallelSummary()
    rc = compu_amd.lib().chip_zstd_parallel(C.c_void_p(d_in.data_ptr()), len(data), None if null_out else C.c_void_p(out.data_ptr()), cap, wlog, flags,
                                            C.byref(s), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = out.cpu().numpy()
    summ = compu_amd.ZstdParallelSummary(s)
    assert (got[summ.out_len if summ.path == PARALLEL else cap:] == POISON).all(), "bytes behind out_len were written"
    return got[:summ.out_len].tobytes(), summ


def assert_parallel(torch, data, content=None, flags=0, cap=None):
    want = batch(torch, data, len(content) if cap is None and content is not None else cap)
    assert want[3] == FINISHED, want[1:]
    got, summ = par(torch, data, want[1] if cap is None else cap, flags)
    assert summ.path == PARALLEL, summ
    assert (summ.out_len, summ.in_used, summ.status, summ.total_out) == (want[1], want[2], FINISHED, want[1]) and got == want[0]
    assert summ.rounds <= ROUNDS_MAX and summ.check == 0
    if content is not None:
        assert got == content
    return summ


def assert_serial(torch, data, cap, flags=0, wlog=0):
    want = batch(torch, data, cap)
    got, summ = par(torch, data, cap, flags, wlog)
    assert summ.path == SERIAL, summ
    assert (got, summ.out_len, summ.in_used, summ.status) == want
    return summ


def three_blocks(rnd, bad=None, **kw):
    """three compressed blocks of about 100 bytes whose matches reach into the block in front; `bad` goes to the middle block"""
    f = W.Frame(**kw)
    f.compressed(P._rb(rnd, 60), [(20, 30, N(15)), (10, 12, N(40))])
    f.compressed(P._rb(rnd, 50), [(15, 40, N(90)), (5, 10, 1), (0, 8, N(120))], **(bad or {}))
    f.compressed(P._rb(rnd, 40), [(10, 50, N(150)), (8, 9, 2)], last=True)
    return f


def test_three_blocks_with_matches_into_the_block_in_front(gpu):
    frame, content = three_blocks(random.Random(1), checksum=True).finish()
    summ = assert_parallel(gpu, frame, content)
    assert (summ.n_blocks, summ.n_sequences) == (3, 7)


@pytest.mark.parametrize("kw", [dict(), dict(checksum=True), dict(fcs=None, window=(0, 0)), dict(fcs=None, window=(4, 3), checksum=True),
                                dict(fcs=4, window=(1, 0)), dict(fcs=8, checksum=True)], ids=str)
def test_frame_header_forms(gpu, kw):
    frame, content = three_blocks(random.Random(2), **kw).finish()
    assert_parallel(gpu, frame, content)
    assert_parallel(gpu, frame, content, flags=NO_CHECKSUM)


CASES = P.all_cases()
# (two description cases are corrupt to a decoder: mixed_empty_last_window holds an RLE block above its window's Block_Maximum_Size,
# every_header_form compressed blocks of two bytes)
MUST_BE_PARALLEL = [c.name for c in CASES if len(c.rows) >= 2 and "without_source" not in c.name and c.name not in ("mixed_empty_last_window", "every_header_form")]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_table_source_and_header_form(gpu, case):
    """the CPU list: the frames with a source for every reuse decode in parallel, the others are the batch's verdict"""
    if case.name in MUST_BE_PARALLEL:
        assert_parallel(gpu, case.frame, case.content)
    else:
        assert_serial(gpu, case.frame, len(case.content) + 8)


def test_raw_rle_and_compressed_blocks_mixed_with_an_empty_last_block(gpu):
    rnd = random.Random(13)
    for last in ("raw", "compressed"):
        f = W.Frame(fcs=None, window=(7, 0), checksum=True)
        f.raw(rnd.randbytes(9000)).rle(0x5A, 70000).compressed(P._rb(rnd, 10), [(2, 50, N(9000)), (3, 400, N(75000))]).rle(7, 0).raw(b"")
        f.compressed(P._rb(rnd, 700), [(300, 2000, N(60000))], lit="huf", streams=4)
        if last == "raw":
            f.raw(b"", last=True)
        else:
            f.compressed(b"", [], lit="rle", last=True)
        frame, content = f.finish()
        assert_parallel(gpu, frame, content)


@pytest.mark.parametrize("ov", [1, 2, 3])
@pytest.mark.parametrize("ll", [0, 4])
def test_first_sequence_of_a_later_block_uses_the_repeat_history(gpu, ov, ll):
    rnd = random.Random(10 * ov + ll)
    f = W.Frame(checksum=True)
    f.raw(rnd.randbytes(100))
    f.compressed(P._rb(rnd, 10), [(2, 5, N(10)), (1, 4, N(20)), (3, 6, N(33))])
    f.rle(0x11, 7)
    f.compressed(P._rb(rnd, 12), [(ll, 5, ov), (2, 6, 1), (0, 4, 2), (1, 7, 3)], last=True)
    frame, content = f.finish()
    assert_parallel(gpu, frame, content)


def test_a_run_of_rep0_minus_1_reaches_the_clamp_from_a_symbolic_value(gpu):
    rnd = random.Random(3)
    f = W.Frame(checksum=True)
    f.raw(rnd.randbytes(64))
    f.compressed(P._rb(rnd, 4), [(2, 5, N(5))])
    f.compressed(P._rb(rnd, 3), [(0, 3, 3)] * 9 + [(1, 4, 1), (0, 3, 2), (0, 5, 3)], last=True)  # 4, 3, 2, 1, 1, ..
    frame, content = f.finish()
    assert_parallel(gpu, frame, content)


def test_a_match_of_offset_1_longer_than_65539(gpu):
    f = W.Frame(fcs=None, window=(7, 0), checksum=True)
    f.raw(b"start of a long run: a")
    f.compressed(b"", [(0, 65539 + 23456, N(1))], modes=("pre", "pre", ("rle", 52)), last=True)
    frame, content = f.finish()
    summ = assert_parallel(gpu, frame, content)
    assert summ.rounds <= ROUNDS_MAX  # a chain of depth 2^16 and more; nothing tighter: a round may read words the same round wrote


def test_forty_blocks_that_each_copy_the_one_in_front(gpu):
    rnd = random.Random(4)
    f = W.Frame(fcs=None, window=(0, 0))
    f.raw(rnd.randbytes(100))
    for k in range(40):
        f.compressed(b"", [(0, 100, N(100))], last=k == 39)
    frame, content = f.finish()
    assert content == content[:100] * 41
    assert_parallel(gpu, frame, content)


def test_a_one_block_frame_and_a_skippable_frame_in_front_are_serial(gpu):
    rnd = random.Random(5)
    f = W.Frame(checksum=True)
    f.compressed(P._rb(rnd, 60), [(20, 30, N(15))], last=True)
    frame, content = f.finish()
    assert_serial(gpu, frame, len(content))
    three, content = three_blocks(rnd).finish()
    assert_serial(gpu, W.skippable(b"abc") + three, len(content))
    assert_serial(gpu, b"", 16)
    assert_serial(gpu, three[:len(three) - 5], len(content))


BAD = [dict(lit_regen=60), dict(seq_extra=3), dict(seq_extra=9), dict(seq_drop=1), dict(seq_drop=5), dict(seq_zero_tail=True), dict(modes_low=1),
       dict(modes_low=2), dict(modes_low=3), dict(nseq=2), dict(body_tail=b"\0")]


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_a_damaged_middle_block_is_the_batchs_verdict(gpu, bad):
    frame, content = three_blocks(random.Random(6), bad=bad).finish()
    summ = assert_serial(gpu, frame, len(content) + 64)
    assert summ.status < 0


def test_a_short_huffman_regenerated_size_in_the_middle_block(gpu):
    rnd = random.Random(7)
    f = W.Frame()
    f.compressed(P._rb(rnd, 60), [(20, 30, N(15))])
    f.compressed(P._rb(rnd, 50, 60, 70), [(15, 40, N(90))], lit="huf", lit_regen=49)
    f.compressed(P._rb(rnd, 40), [(10, 50, N(150))], last=True)
    frame, content = f.finish()
    assert assert_serial(gpu, frame, len(content) + 64).status < 0


def around(rnd, lits, seqs, **mid):
    """a three-block frame whose middle block is compressed(lits, seqs, **mid)"""
    f = W.Frame()
    f.compressed(P._rb(rnd, 60), [(20, 30, N(15))])
    f.compressed(lits, seqs, **mid)
    f.compressed(P._rb(rnd, 40), [(10, 50, N(50))], last=True)
    return f.finish()


def _fse_damages():
    """tests/zstd_cases.py's table-description damages: an accuracy above the table's limit, more symbols than the table has"""
    out = []
    for k, (t, al) in enumerate((("ll", 10), ("of", 9), ("ml", 10))):
        out.append((f"accuracy_{t}_{al}", dict(modes=tuple(("fse", [2] * 16, 5) if j == k else "pre" for j in range(3)), al_field={t: al}, invalid=1)))
    for k, (t, nsym) in enumerate((("ll", 37), ("of", 33), ("ml", 54))):
        norm = [1] * (nsym - 1) + [64 - nsym + 1]
        out.append((f"fse_symbols_{t}_{nsym}", dict(modes=tuple(("fse", norm, 6) if j == k else "pre" for j in range(3)), invalid=1)))
    return out


@pytest.mark.parametrize("name,mid", _fse_damages(), ids=[d[0] for d in _fse_damages()])
def test_a_damaged_table_description_in_the_middle_block(gpu, name, mid):
    frame, content = around(random.Random(15), b"ab", [(1, 5, N(9))], **mid)
    assert assert_serial(gpu, frame, len(content) + 64).status < 0


@pytest.mark.parametrize("name,tree", [("rest_not_pow2", bytes([127 + 2, 0x31])), ("all_zero", bytes([127 + 2, 0x00])),
                                       ("weight_12", bytes([127 + 3, 0xC1, 0x10]))], ids=lambda v: v if isinstance(v, str) else "")
def test_a_damaged_huffman_tree_in_the_middle_block(gpu, name, tree):
    rnd = random.Random(16)
    frame, content = around(rnd, P._rb(rnd, 100, 97, 100), [], lit="huf", weights=[0] * 97 + [2, 1, 1], tree_bytes=tree)
    assert assert_serial(gpu, frame, len(content) + 64).status < 0


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("key,val", [("lit_extra", 5), ("lit_drop", 2)])
def test_damaged_huffman_streams_in_the_middle_block(gpu, key, val, streams):
    rnd = random.Random(17)
    frame, content = around(rnd, P._rb(rnd, 300, 60, 70), [(3, 9, N(40)), (1, 5, 2), (0, 30, N(20))], lit="huf", streams=streams, **{key: val})
    assert assert_serial(gpu, frame, len(content) + 64).status < 0


@pytest.mark.parametrize("what", ["fse", "huffman"])
def test_a_damaged_description_that_a_later_block_replays(gpu, what):
    """the block behind the damaged one reuses its table: the replay pass meets the damage too"""
    rnd = random.Random(18)
    f = W.Frame()
    f.raw(rnd.randbytes(200))
    if what == "fse":
        f.compressed(b"ab", [(1, 5, N(9))], modes=(("fse", [2] * 16, 5), "pre", "pre"), al_field={"ll": 10}, invalid=1)
        f.compressed(b"cd", [(1, 5, N(9))], modes=("rep", "pre", "pre"), last=True)
    else:
        f.compressed(P._rb(rnd, 100, 97, 100), [], lit="huf", weights=[0] * 97 + [2, 1, 1], tree_bytes=bytes([127 + 2, 0x00]))
        f.compressed(P._rb(rnd, 50, 97, 100), [(3, 4, N(20))], lit="treeless", last=True)
    frame, content = f.finish()
    assert assert_serial(gpu, frame, len(content) + 64).status < 0


def test_blocks_behind_byte_2_pow_28_of_the_frame(gpu):
    """2 049 raw blocks of 128 KiB, then compressed blocks -- Huffman, treeless and Repeat over a raw block -- that begin behind byte 2^28
    of the frame and reach into the raw content.  No unit holds such a frame, so the content is the writer's."""
    rnd = random.Random(14)
    nraw, size = 2049, 128 << 10
    body = np.empty((nraw, 3 + size), np.uint8)
    body[:, :3] = np.frombuffer((size << 3).to_bytes(3, "little"), np.uint8)
    body[:, 3:] = np.frombuffer(rnd.randbytes(size), np.uint8) ^ np.arange(nraw, dtype=np.uint8)[:, None]
    f = W.Frame(fcs=None, window=(7, 0))
    f.content = bytearray(body[-1, 3:].tobytes())  # what the writer's matches may reach
    f.compressed(P._rb(rnd, 300, 60, 90) + bytes(range(60, 90)), [(50, 1000, N(100000)), (20, 300, N(5))], lit="huf", streams=1)
    f.raw(b"xyz" * 10)
    f.compressed(P._rb(rnd, 200, 60, 90), [(10, 40, 1), (5, 2000, N(70000)), (0, 9, 3)], lit="treeless", streams=1, modes=("rep", "rep", "rep"), last=True)
    frame = f.header() + body.tobytes() + bytes(f.blocks)
    content = body[:, 3:].tobytes() + bytes(f.content[size:])
    assert len(f.header()) + body.size > 1 << 28
    got, summ = par(gpu, frame, len(content))
    assert (summ.path, summ.status, summ.out_len, summ.in_used, summ.n_blocks) == (PARALLEL, FINISHED, len(content), len(frame), nraw + 3), summ
    assert got == content
    # what is not clean in such a frame fits no unit: refused, and nothing written
    got, summ = par(gpu, frame[:-1], len(content))
    assert (summ.path, summ.out_len, got) == (REFUSED, 0, b"")


def test_offsets_one_beyond_the_content_and_one_beyond_the_window(gpu):
    rnd = random.Random(8)
    for off, ok in ((110, True), (111, False)):  # 100 bytes of the raw block and 10 literals lie in front of the match
        f = W.Frame(fcs=None, window=(0, 0))
        f.raw(rnd.randbytes(100))
        f.compressed(P._rb(rnd, 10), [(10, 5, N(off))], last=True, invalid=1)
        frame, content = f.finish()
        if ok:
            assert_parallel(gpu, frame, content)
        else:
            assert assert_serial(gpu, frame, len(content) + 8).status < 0
    for off, ok in ((1024, True), (1025, False)):  # a window of 1 KiB
        f = W.Frame(fcs=None, window=(0, 0))
        f.raw(rnd.randbytes(1000)).raw(rnd.randbytes(1000))
        f.compressed(P._rb(rnd, 10), [(10, 5, N(off))], last=True)
        frame, content = f.finish()
        if ok:
            assert_parallel(gpu, frame, content)
        else:
            assert assert_serial(gpu, frame, len(content) + 8).status < 0


def test_a_wrong_checksum_is_minus_22_and_finished_when_waived(gpu):
    frame, content = three_blocks(random.Random(9), checksum=True).finish(checksum_value=0x12345678)
    assert assert_serial(gpu, frame, len(content)).status == -22
    got, summ = par(gpu, frame, len(content), NO_CHECKSUM)
    assert (summ.path, summ.status, summ.out_len, summ.in_used, summ.check) == (PARALLEL, FINISHED, len(content), len(frame), 0) and got == content


def test_a_window_above_the_limit_is_the_batchs_verdict(gpu):
    f = W.Frame(fcs=None, window=(11, 0))  # 2 MiB
    f.raw(b"abc").raw(b"def", last=True)
    frame, content = f.finish()
    assert_parallel(gpu, frame, content)
    got, summ = par(gpu, frame, 16, wlog=20)
    assert (summ.path, summ.status) == (SERIAL, -16)


def test_room(gpu):
    frame, content = three_blocks(random.Random(11), checksum=True).finish()
    n = len(content)
    got, summ = par(gpu, frame, n - 1)
    assert (summ.path, summ.status, summ.out_len, summ.total_out) == (PARALLEL, NEED_OUTPUT, 0, n) and got == b""
    got, summ = par(gpu, frame, 0, null_out=True)
    assert (summ.path, summ.status, summ.out_len, summ.total_out) == (PARALLEL, NEED_OUTPUT, 0, n)
    got, summ = par(gpu, frame, n + 33)
    assert (summ.path, summ.status, summ.out_len, summ.total_out) == (PARALLEL, FINISHED, n, n) and got == content


def test_arguments_and_the_python_call(gpu):
    import compu_amd
    from compu_amd.api import _ZstdParallelSummary

    lib, s = compu_amd.lib(), _ZstdParallelSummary()
    frame, content = three_blocks(random.Random(12), checksum=True).finish()
    d_in = upload(gpu, frame)
    p = C.c_void_p(d_in.data_ptr())
    assert lib.chip_zstd_parallel(p, len(frame), None, 0, 0, 0, None, None) == -101
    assert lib.chip_zstd_parallel(None, 5, None, 0, 0, 0, C.byref(s), None) == -101
    assert lib.chip_zstd_parallel(C.c_void_p(d_in.data_ptr() + 1), 5, None, 0, 0, 0, C.byref(s), None) == -101
    assert lib.chip_zstd_parallel(p, len(frame), None, 0, 0, 2, C.byref(s), None) == -101
    assert lib.chip_zstd_parallel(p, 1 << 32, None, 0, 0, 0, C.byref(s), None) == -101
    out, summ = compu_amd.zstd_parallel(d_in, len(frame))
    assert summ.path == PARALLEL and summ.status == FINISHED and out.cpu().numpy().tobytes() == content
    room = gpu.zeros(len(content) + 5, dtype=gpu.uint8, device="cuda")
    out, summ = compu_amd.zstd_parallel(d_in, len(frame), room, checksum=False)
    assert summ.out_len == len(content) and out.cpu().numpy().tobytes() == content
    compu_amd.trim()
    out, summ = compu_amd.zstd_parallel(d_in, len(frame))
    assert out.cpu().numpy().tobytes() == content


def test_the_python_call_sizes_a_frame_of_the_serial_path(gpu):
    import compu_amd

    f = W.Frame(fcs=None, window=(0, 0), checksum=True)
    f.compressed(P._rb(random.Random(19), 60), [(20, 30, N(15))], last=True)
    frame, content = f.finish()
    out, summ = compu_amd.zstd_parallel(upload(gpu, frame), len(frame))
    assert (summ.path, summ.status, summ.out_len) == (SERIAL, FINISHED, len(content)) and out.cpu().numpy().tobytes() == content
    out, summ = compu_amd.zstd_parallel(upload(gpu, frame[:-6]), len(frame) - 6)  # a cut frame: no size, no bytes
    assert summ.path == SERIAL and out.numel() == 0


def libzstd_frames(alice):
    import zstd_ref
    from bench_support import synth

    z = zstd_ref.load()
    for cname, data in (("synth", synth.payloads(20, threads=2).tobytes()), ("alice", (alice * 12)[:1500000])):
        for level in (1, 3, 19):
            yield cname, level, data, zstd_ref.compress(z, data, level, True, True)


def test_libzstd_frames_decode_in_parallel(gpu, alice):
    import compu_amd

    treeless = repeat = 0
    for cname, level, data, frame in libzstd_frames(alice):
        blocks, bs = compu_amd.zstd_blocks_host(frame)
        assert bs.window_size > 128 * 1024
        comp = blocks["type"] == 2
        treeless += int((comp & (blocks["lit_type"] == 3)).sum())
        repeat += int((comp[:, None] & (blocks["n_seq"][:, None] > 0) & (blocks["mode"] == 3)).sum())
        summ = assert_parallel(gpu, frame, data)
        assert summ.n_blocks == bs.n_blocks, (cname, level)
        assert_parallel(gpu, frame, data, flags=NO_CHECKSUM)
    assert treeless > 0 and repeat > 0  # what the case is for (tests/test_zstd_parallel_cpu.py checks the same on the host)


def test_two_calls_give_the_same_bytes_and_summary(gpu, alice):
    for cname, level, data, frame in libzstd_frames(alice):
        if level != 3:
            continue
        a, sa = par(gpu, frame, len(data))
        b, sb = par(gpu, frame, len(data))
        assert a == b == data and sa.as_tuple() == sb.as_tuple() and sa.path == PARALLEL
