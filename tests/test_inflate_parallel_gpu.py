"""chip_inflate_parallel on the GPU: one stream decoded by a wave per chunk.  Files with small blocks (alice29.txt at memLevel 2;
the 2.5 MiB bench payload) and built streams (tests/inflate_parallel_cases.py) give the content of zlib.decompress, the answers of
chip_decode_batch, the points the reference names (the first block and every true start), their checks and windows, and they run on
the parallel path; the index they leave reads back through chip_inflate_index_read; a decoy start costs nothing but its wave; what
is not clean, and what has one block, is answered as chip_decode_batch answers it; too little room names the size to come back
with.  Without the feature every test fails at the missing symbols."""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_writer as W
import inflate_index_cases as IC
import inflate_index_ref as XR
import inflate_parallel_cases as PC
import inflate_parallel_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD, WINDOW = 0xEE, 64, 32768
POISON64 = int.from_bytes(bytes([POISON]) * 8, "little")
FINISHED, NEED_INPUT, NEED_OUTPUT = 2, 0, 1
SERIAL, PARALLEL = 0, 1


def upload(torch, data):
    """`data` in a 16-byte aligned device tensor padded to a multiple of 4 (and never empty)"""
    t = torch.full(((len(data) + 3) // 4 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


def u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def run(torch, fmt, data, out_cap, chunk_bytes, max_points, room=None, null_out=False):
    """chip_inflate_parallel into a poisoned room and poisoned arrays of `room` entries -> dict of everything it answered"""
    import compu_amd
    from compu_amd.api import _InflateParallelSummary

    room = max_points if room is None else room
    d_in = upload(torch, data)
    out = torch.full((out_cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    pt_bit = torch.full((room * 8,), POISON, dtype=torch.uint8, device="cuda").view(torch.int64) if room else None
    pt_out = pt_bit.clone() if room else None
    pt_check = torch.full((room * 4,), POISON, dtype=torch.uint8, device="cuda").view(torch.int32) if room else None
    windows = torch.full((room * WINDOW,), POISON, dtype=torch.uint8, device="cuda") if room else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    raw = _InflateParallelSummary()
    rc = compu_amd.lib().chip_inflate_parallel(XR.FMT[fmt], p(d_in), len(data), None if null_out else p(out), out_cap, chunk_bytes, max_points,
                                               p(pt_bit), p(pt_out), p(pt_check), p(windows), C.byref(raw), None)
    assert rc == 0
    torch.cuda.synchronize()
    return dict(d_in=d_in, out=out, pt_bit=pt_bit, pt_out=pt_out, pt_check=pt_check, windows=windows, summ=compu_amd.InflateParallelSummary(raw))


def decode_one(torch, fmt, data, out_cap):
    """chip_decode_batch of the same unit into the same poisoned room -> (out tensor, out_len, in_used, status)"""
    import compu_amd

    out = torch.full((out_cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")  # noqa: E731
    out_len, in_used, status = compu_amd.decode_batch(XR.FMT[fmt], upload(torch, data), i64(0), i32(len(data)), out, i64(0), i32(out_cap))
    torch.cuda.synchronize()
    return out, u32(out_len)[0], u32(in_used)[0], int(status[0])


def same_as_decode(torch, fmt, data, out_cap, b):
    out, out_len, in_used, status = decode_one(torch, fmt, data, out_cap)
    s = b["summ"]
    assert (s.out_len, s.in_used, s.status) == (out_len, in_used, status)
    assert torch.equal(b["out"], out), "the bytes written are chip_decode_batch's, and nothing behind the room"
    return status


def guard_untouched(b, out_cap):
    assert (b["out"][out_cap:] == POISON).all()


def check_points(b, want, content, n_all=None):
    """the first len(want) entries equal `want` [(bit, out, check)], the windows hold the content in front of each point, and
    nothing is written behind the entries"""
    s, n = b["summ"], len(want)
    assert s.n_points == (n if n_all is None else n_all)
    bits, outs, checks = u64(b["pt_bit"]), u64(b["pt_out"]), u32(b["pt_check"])
    assert list(zip(bits[:n], outs[:n], checks[:n])) == want
    assert all(v == POISON64 for v in bits[n:] + outs[n:]) and all(v == POISON64 & 0xFFFFFFFF for v in checks[n:])
    win = b["windows"].cpu().numpy()
    for k, (_, o, _) in enumerate(want):
        wl = min(WINDOW, o)
        assert win[k * WINDOW:k * WINDOW + wl].tobytes() == content[o - wl:o], k
    assert (win[n * WINDOW:] == POISON).all()


def points_of(bounds, first_bit, chunk_bytes, length, wrap, content):
    """the chain's points when every start is true: the first block and the first non-final dynamic block of every later chunk"""
    out_at = {b: o for b, o, _, _ in bounds}
    bits = [first_bit] + R.true_starts(bounds, first_bit, chunk_bytes, length)
    return [(b, out_at[b], XR.check_of(wrap, content[:out_at[b]])) for b in bits]


def whole_answer(torch, fmt, data, content, bounds, first_bit, chunk_bytes):
    """everything the issue asks of a clean stream on the parallel path"""
    wrap, cap = XR.WRAP[fmt], len(content)
    want = points_of(bounds, first_bit, chunk_bytes, len(data), wrap, content)
    assert len(want) >= 2
    b = run(torch, fmt, data, cap, chunk_bytes, len(want) + 2)
    s = b["summ"]
    assert b["out"][:cap].cpu().numpy().tobytes() == content
    guard_untouched(b, cap)
    assert (s.path, s.status, s.out_len, s.total_out, s.wrap, s.n_false) == (PARALLEL, FINISHED, cap, cap, wrap, 0)
    assert s.n_starts == len(want) - 1 and s.check == XR.check_of(wrap, content)
    check_points(b, want, content)
    assert same_as_decode(torch, fmt, data, cap, b) == FINISHED
    return b, want


def stream_bounds(s):
    """[(bit, out, btype, final)] of a built stream"""
    heads = [r for r in s.layout if r.kind == "block"]
    return [(r.bit, r.out, blk[1], bool(blk[2])) for r, blk in zip(heads, s.blocks)]


def serial_bounds(torch, fmt, data, cap):
    """the block boundaries of a file too long for the Python inflate: the serial index build at spacing 1 names every boundary
    with new output, and the stream's own bits say what kind of block starts there"""
    import compu_amd

    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    index, summ = compu_amd.inflate_index_build(XR.FMT[fmt], upload(torch, data), len(data), out, spacing=1)
    assert summ.status == FINISHED
    return [(b, o, R.bits(data, b + 1, 2), bool(R.bits(data, b, 1))) for b, o in zip(u64(index.pt_bit), u64(index.pt_out))]


@pytest.mark.parametrize("chunk_bytes", PC.CHUNKS)
@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_alice_with_small_blocks(gpu, fmt, chunk_bytes):
    content = IC.file_content("alice")
    if fmt == "gzip":  # FEXTRA and FNAME in front of the stream
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 2)
        data = IC.GZIP_FIELDS + co.compress(content) + co.flush() + W.gzip_trailer(content)
        first_bit = 8 * len(IC.GZIP_FIELDS)
    else:
        data, first_bit = PC.alice(fmt)
    bounds, walked = R.walk_cached(data, first_bit)
    assert walked == content == zlib.decompress(data, XR.FMT[fmt])
    whole_answer(gpu, fmt, data, content, bounds, first_bit, chunk_bytes)


def test_bench_payload(gpu):
    content = IC.file_content("bench")
    data = IC.compressed("bench", 6, "gzip")
    bounds = serial_bounds(gpu, "gzip", data, len(content))
    b, want = whole_answer(gpu, "gzip", data, content, bounds, 80, 16384)
    n_chunks = -(-len(data) // 16384)
    assert len(want) - 1 >= (n_chunks - 1) // 2  # most chunks hold a block start


@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_built_edges(gpu, fmt):
    s = PC.built_edges(fmt)
    whole_answer(gpu, fmt, s.data, s.content, stream_bounds(s), 8 * s.hdr_len, PC.EDGE_CHUNK)


def test_index_hand_on(gpu):
    """the arrays go to chip_inflate_index_read unchanged: the whole content with every chunk good, also from a truncated index"""
    import compu_amd

    s = PC.built_edges("gzip")
    d_in = upload(gpu, s.data)
    out, index, summ = compu_amd.inflate_parallel(31, d_in, len(s.data), chunk_bytes=PC.EDGE_CHUNK, index=True)
    assert (summ.path, summ.status) == (PARALLEL, FINISHED) and out.cpu().numpy().tobytes() == s.content
    assert index.n_points == summ.n_points >= 6 and index.total_out == len(s.content)
    assert compu_amd.gzip_index_decode(index, d_in).cpu().numpy().tobytes() == s.content
    got, _ = compu_amd.gzip_index_read(index, d_in, [(0, 10), (32760, 20), (len(s.content) - 5, 5), (40000, 100000)])
    want = s.content[:10] + s.content[32760:32780] + s.content[-5:] + s.content[40000:140000]
    assert got.cpu().numpy().tobytes() == want
    b = run(gpu, "gzip", s.data, len(s.content), PC.EDGE_CHUNK, 3, room=5)
    assert b["summ"].n_points == summ.n_points and u64(b["pt_bit"])[:3] == u64(index.pt_bit)[:3] and u64(b["pt_bit"])[3:] == [POISON64] * 2
    cut = compu_amd.InflateIndex(31, len(s.data), len(s.content), b["pt_bit"][:3], b["pt_out"][:3], b["pt_check"][:3], b["windows"][:3 * WINDOW])
    assert compu_amd.gzip_index_decode(cut, d_in).cpu().numpy().tobytes() == s.content


@pytest.mark.parametrize("chunk_bytes", PC.CHUNKS)
def test_decoy_costs_its_wave(gpu, chunk_bytes):
    s, at = PC.decoy(chunk_bytes)
    cap = len(s.content)
    b = run(gpu, "raw", s.data, cap, chunk_bytes, 64)
    summ = b["summ"]
    assert b["out"][:cap].cpu().numpy().tobytes() == s.content
    guard_untouched(b, cap)
    assert (summ.path, summ.status, summ.out_len) == (PARALLEL, FINISHED, cap) and summ.n_false >= 1
    bits = u64(b["pt_bit"])[:summ.n_points]
    assert at not in bits and set(bits) <= {blk[0] for blk in s.blocks} and summ.n_points == summ.n_starts - summ.n_false + 1
    assert same_as_decode(gpu, "raw", s.data, cap, b) == FINISHED


def test_too_far_back(gpu):
    s = PC.too_far_back()
    cap = len(s.content) + 100
    b = run(gpu, "raw", s.data, cap, 256, 16)
    assert same_as_decode(gpu, "raw", s.data, cap, b) == -3
    assert b["summ"].path == SERIAL and b["summ"].n_starts >= 2


def _not_clean():
    out = []
    for fmt in ("zlib", "gzip"):
        s = IC.damage(fmt)
        out.append((f"wrong-check-{fmt}", fmt, IC.flipped_stored_byte(s, IC.DAMAGE_BLOCK)[0], len(s.content)))
    s = IC.damage("gzip")
    huff = next(r for r in s.layout if r.kind == "lit" and r.block == 6)
    data = bytearray(s.data)
    data[huff.bit // 8 + 40] ^= 0x10
    out.append(("flipped-huffman", "gzip", bytes(data), len(s.content)))
    for cut in (len(s.data) - 1, len(s.data) - 5, len(s.data) - 9, len(s.data) // 2, 700, 30, 11, 3):
        out.append((f"cut-{cut}", "gzip", s.data[:cut], len(s.content)))
    z = IC.damage("zlib")
    out.append(("fdict", "zlib", W.zlib_header(fdict=True, dictid=0x12345678) + z.data[2:], len(z.content)))
    out.append(("trailing", "gzip", s.data + b"\x00" * 37, len(s.content)))
    out.append(("two-members", "gzip", s.data + IC.damage("gzip").data, 2 * len(s.content)))
    out.append(("empty", "gzip", b"", 16))
    return out


def test_not_clean_answers_as_decode_batch(gpu):
    for name, fmt, data, cap in _not_clean():
        b = run(gpu, fmt, data, cap, 256, 8)
        assert same_as_decode(gpu, fmt, data, cap, b) is not None, name
        if name.startswith(("wrong", "flipped", "cut", "fdict", "empty")):
            assert b["summ"].path == SERIAL, name
        if name.startswith(("wrong", "flipped")) or name in ("cut-30", "cut-700"):
            assert b["summ"].n_points == 1, name  # the first block; a refused or cut wrapper has none
        if name in ("empty", "cut-3", "cut-11"):
            assert b["summ"].n_points == 0, name


@pytest.mark.parametrize("case", ["parallel", "serial"])
def test_room_short(gpu, case):
    content = IC.file_content("alice")
    data = PC.alice("gzip")[0] if case == "parallel" else IC.compressed("alice", 6, "gzip")
    for cap, null_out in ((len(content) - 1, False), (0, True)):
        b = run(gpu, "gzip", data, cap, 2048 if case == "parallel" else 0, 0, null_out=null_out)
        s = b["summ"]
        assert (s.status, s.out_len, s.total_out) == (NEED_OUTPUT, 0, len(content)), (case, cap)
        assert s.path == (PARALLEL if case == "parallel" else SERIAL)
        guard_untouched(b, cap)


def test_serial_path(gpu):
    import compu_amd

    content = IC.file_content("alice")
    # the library's own level-1 output: one block
    src = upload(gpu, content)
    room = gpu.empty(compu_amd.encode_bound(31, len(content)), dtype=gpu.uint8, device="cuda")
    i64 = lambda v: gpu.tensor([v], dtype=gpu.int64, device="cuda")  # noqa: E731
    i32 = lambda v: gpu.tensor([v], dtype=gpu.int32, device="cuda")  # noqa: E731
    enc_len, _ = compu_amd.encode_batch(31, 1, src, i64(0), i32(len(content)), room, i64(0), i32(room.numel()))[:2]
    own = room[:u32(enc_len)[0]].cpu().numpy().tobytes()
    assert zlib.decompress(own, 31) == content
    for name, data in (("own-level-1", own), ("default-memlevel", IC.compressed("alice", 6, "gzip"))):
        b = run(gpu, "gzip", data, len(content), 0, 4)  # the default chunk is longer than the file
        s = b["summ"]
        assert b["out"][:len(content)].cpu().numpy().tobytes() == content, name
        assert (s.path, s.status, s.n_points, s.n_false) == (SERIAL, FINISHED, 1, 0), name
        assert same_as_decode(gpu, "gzip", data, len(content), b) == FINISHED, name


def test_python_face(gpu):
    import compu_amd

    data, _ = PC.alice("zlib")
    content = IC.file_content("alice")
    d_in = upload(gpu, data)
    out, summ = compu_amd.inflate_parallel(15, d_in, len(data), chunk_bytes=2048)
    assert out.cpu().numpy().tobytes() == content and (summ.path, summ.status) == (PARALLEL, FINISHED)
    out, index, summ = compu_amd.inflate_parallel(47, d_in, len(data), chunk_bytes=2048, index=True)  # auto names the wrapper
    assert out.cpu().numpy().tobytes() == content and index.fmt == 15 and index.n_points == summ.n_points > 20
    got, _ = compu_amd.gzip_index_read(index, d_in, [(1000, 50), (100000, 3000)])
    assert got.cpu().numpy().tobytes() == content[1000:1050] + content[100000:103000]
