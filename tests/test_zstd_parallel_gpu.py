"""The block description of one zstd frame on the GPU (chip_zstd_blocks) against chip_zstd_blocks_host, itself
pinned to the cases and to a second reading of the headers by tests/test_zstd_parallel_cpu.py: every case of
tests/zstd_parallel_cases.py, every cut of a three-block frame, the block cap, more than one tile of the source scan, frames of the
system libzstd, part of a frame into a poisoned array, every alignment, a stream of the caller's, chip_trim.  Without the feature
every test here fails at the missing symbol."""
import ctypes as C

import numpy as np
import pytest

import zstd_parallel_cases as P
from test_zstd_parallel_cpu import rows_of

pytestmark = pytest.mark.gpu

POISON = 0xEE
CASES = P.all_cases()


def upload(torch, data, shift=0, fill=0xA5):
    """`data` in a device tensor at a 4-byte aligned start `shift` bytes behind a 16-byte aligned one, padded to a multiple of 4;
    the bytes around it hold `fill`."""
    room = shift + (len(data) + 3) // 4 * 4 + 4
    t = torch.full((room,), fill, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t[shift:]


def host(data, max_blocks=None):
    import compu_amd

    blocks, summ = compu_amd.zstd_blocks_host(data, max_blocks)
    return blocks.tobytes(), summ.as_tuple()


def device(torch, data, max_blocks, room, shift=0, fill=0xA5, stream=None):
    """chip_zstd_blocks into a poisoned device array of `room` records: (the bytes of the records written, summary tuple); what
    lies behind min(n_blocks, max_blocks) records must still hold the poison"""
    import compu_amd
    from compu_amd.api import _ZstdBlocksSummary

    d_buf = upload(torch, data, shift, fill)
    recs = torch.full((room * 48,), POISON, dtype=torch.uint8, device="cuda")
    s = _ZstdBlocksSummary()
    sp = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = compu_amd.lib().chip_zstd_blocks(C.c_void_p(d_buf.data_ptr()) if data else None, len(data), max_blocks,
                                          C.c_void_p(recs.data_ptr()) if max_blocks else None, C.byref(s), sp)
    assert rc == 0
    got = recs.cpu().numpy()
    k = min(int(s.n_blocks), max_blocks)
    assert k <= room and (got[k * 48:] == POISON).all()
    return got[:k * 48].tobytes(), compu_amd.ZstdBlocksSummary(s).as_tuple()


def assert_same(torch, data, max_blocks=None, **kw):
    n = host(data, 0)[1][0]
    m = n + 2 if max_blocks is None else max_blocks
    want = host(data, m)
    got = device(torch, data, m, max(n, m) + 3, **kw)
    assert got[1] == want[1]
    assert got[0] == want[0]
    return got


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_blocks_equal_the_host_form(gpu, case):
    assert_same(gpu, case.frame, shift=4 * (len(case.frame) % 4))
    assert_same(gpu, case.frame, shift=(8, 12, 0, 4)[len(case.frame) % 4], fill=0xFD)


@pytest.mark.parametrize("name,frame,want", P.malformed_cases(), ids=[m[0] for m in P.malformed_cases()])
def test_section_headers_that_do_not_fit(gpu, name, frame, want):
    import compu_amd

    got, summ = assert_same(gpu, frame)
    rows = rows_of(np.frombuffer(got, compu_amd.zstd_block_dtype()))
    assert [(r[6], r[7], r[2], r[3], r[4], r[8]) for r in rows] == want


def test_truncated_at_every_byte_of_a_three_block_frame(gpu):
    frame = P.three_block_frame().frame
    for n in range(len(frame) + 1):
        got, summ = assert_same(gpu, frame[:n], fill=frame[n] if n < len(frame) else 0)  # the byte behind the cut is there, and not read
        assert summ[4] == (P.TRUNCATED if n < len(frame) else P.OK)


@pytest.mark.parametrize("name,data,status,n", P.verdict_files(), ids=[v[0] for v in P.verdict_files()])
def test_walk_verdicts(gpu, name, data, status, n):
    got, summ = assert_same(gpu, data)
    assert (summ[4], summ[0]) == (status, n)


@pytest.mark.parametrize("name,data,status,n", P.block_cap_files(), ids=[v[0] for v in P.block_cap_files()])
def test_walk_follows_2_pow_20_blocks_and_no_more(gpu, name, data, status, n):
    got, summ = assert_same(gpu, data)
    assert (summ[4], summ[0]) == (status, n)


def test_sources_across_the_tiles_of_the_scan(gpu):
    """3000 blocks: the scan's workgroup makes three trips; definers sit at a tile's last and first block, and a source is found
    more than a tile back"""
    rnd = np.random.default_rng(7)
    b = P.Built(fcs=None, window=(10, 0))
    defs = {0, 1023, 1024, 2047, 2900}
    for i in range(3000):
        last = i == 2999
        if i in defs:
            b.compressed(bytes(range(65, 91)) * 2, [(3, 4, P.N(2))], lit="huf", streams=1, last=last)
        elif i % 3 == 0:
            b.compressed(b"ABC", [(1, 3, 1)], lit="treeless", streams=1, modes=("rep", "rep", "rep"), last=last)
        elif i % 3 == 1:
            b.raw(rnd.bytes(5), last=last)
        else:
            b.rle(i & 255, 3, last=last)
    frame, _ = b.f.finish()
    got, summ = assert_same(gpu, frame)
    import compu_amd

    src = np.frombuffer(got, compu_amd.zstd_block_dtype())["src"]
    want = np.array([max([d for d in defs if d < i], default=-1) for i in range(3000)])
    assert summ[0] == 3000 and (src == want[:, None]).all()


def test_libzstd_frames(gpu, alice):
    import zstd_ref
    from bench_support import synth

    z = zstd_ref.load()
    for data in (synth.payloads(20, threads=2).tobytes(), (alice * 12)[:1500000]):
        for level in (1, 3, 19):
            frame = zstd_ref.compress(z, data, level, True, True)
            got, summ = assert_same(gpu, frame, shift=4)
            assert summ[4] == P.OK and summ[1] == len(frame) and summ[2] == len(data)


def test_counts_and_fills_part_of_a_frame(gpu):
    import compu_amd

    case = CASES[0]
    n = len(case.rows)
    for m in (0, 1, n - 1, n, n + 5):
        assert_same(gpu, case.frame, max_blocks=m)
    blocks, summ = compu_amd.zstd_blocks(upload(gpu, case.frame), len(case.frame))
    want, wsum = compu_amd.zstd_blocks_host(case.frame)
    assert blocks.shape == (n, 48) and blocks.cpu().numpy().tobytes() == want.tobytes() and summ.as_tuple() == wsum.as_tuple()
    blocks, summ = compu_amd.zstd_blocks(upload(gpu, b""), 0)
    assert blocks.shape == (0, 48) and summ.as_tuple() == compu_amd.zstd_blocks_host(b"")[1].as_tuple()


def test_a_stream_of_the_callers_and_trim(gpu):
    """the same answer on another stream, twice; chip_trim() releases the slots and the next call allocates again"""
    import compu_amd

    case = CASES[1]
    want = host(case.frame, len(case.rows))
    side = gpu.cuda.Stream()
    for _ in range(2):
        with gpu.cuda.stream(side):
            assert device(gpu, case.frame, len(case.rows), len(case.rows) + 1, stream=side) == want
        assert device(gpu, case.frame, len(case.rows), len(case.rows) + 1) == want
    gpu.cuda.synchronize()
    compu_amd.trim()
    assert device(gpu, case.frame, len(case.rows), len(case.rows) + 1) == want
