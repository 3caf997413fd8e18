"""chip_inflate_parallel_next on the GPU: one stream decoded slab by slab from a carried cursor.  The bytes are zlib's whatever the
slabs; after every call the cursor stands on a true block boundary, the window holds the last bytes of the content and the check
is zlib's over it; the calls of the listed inputs run on the parallel path (tests/test_inflate_stream_cpu.py shows why), slabs
without a start on one wave; blocks longer than the slab, room shorter than a chunk, headers and trailers across slabs, errors,
totals beyond 2^32 and the Python loop.  Without the feature every test fails at the missing symbol."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import deflate_writer as W
import inflate_index_cases as IC
import inflate_parallel_cases as PC
import inflate_parallel_ref as R
import inflate_stream_cases as SC
import inflate_stream_ref as SR

pytestmark = pytest.mark.gpu

POISON, GUARD, WINDOW = 0xEE, 64, 32768
NEED_INPUT, NEED_OUTPUT, FINISHED, NEED_DICT = 0, 1, 2, 3
SERIAL, PARALLEL = 0, 1
HEADER, BLOCKS, TRAILER, DONE, ERROR = range(5)


def check_of(wrap, content):
    return zlib.adler32(content) if wrap == 1 else zlib.crc32(content) if wrap == 2 else 0


def upload(torch, data, shift=0):
    """`data` at byte `shift` of a device tensor, padded behind to a multiple of 4 and more"""
    t = torch.full((shift + (len(data) + 3) // 4 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


class Drive:
    """a decode of `data` through slabs of `slab` bytes into a room of `room`: every call's summary and the cursor behind it"""

    def __init__(self, torch, fmt, data, slab, room, chunk_bytes, cursor=None):
        import compu_amd

        self.torch, self.api, self.data, self.slab, self.room, self.chunk = torch, compu_amd, data, slab, room, chunk_bytes
        self.cur = cursor if cursor is not None else compu_amd.InflateCursor(fmt)
        self.d_in = upload(torch, data, 1)  # the stream at an odd address: no slab is aligned unless its offset happens to be
        self.pos, self.got, self.calls = 0, bytearray(), []

    def step(self, slab=None, room=None):
        torch = self.torch
        slab, room = self.slab if slab is None else slab, self.room if room is None else room
        n = min(slab, len(self.data) - self.pos)
        out = torch.full((room + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        before = (self.cur.in_total, self.cur.out_total, self.cur.bit, self.cur.phase)
        s = self.api.inflate_parallel_next(self.cur, self.d_in[1 + self.pos:1 + self.pos + n], out[:room], self.chunk)
        torch.cuda.synchronize()
        assert s.out_len <= room and (out[room:] == POISON).all(), "nothing is written behind the room"
        assert s.in_used <= n
        self.got += out[:s.out_len].cpu().numpy().tobytes()
        self.pos += s.in_used
        s.before, s.slab, s.pos = before, n, self.pos - s.in_used
        s.moved = (self.cur.in_total, self.cur.out_total, self.cur.bit, self.cur.phase) != before
        self.calls.append(s)
        assert self.cur.in_total - before[0] == s.in_used and self.cur.out_total - before[1] == s.out_len
        return s

    def run(self, limit=400):
        """to the end, doubling the slab or the room where a call says so without moving"""
        slab, room = self.slab, self.room
        for _ in range(limit):
            s = self.step(slab, room)
            if s.status not in (NEED_INPUT, NEED_OUTPUT):
                return s
            if s.in_used == 0 and s.out_len == 0:
                if s.status == NEED_INPUT:
                    assert s.slab == slab, "the stream ends inside a step"
                    slab *= 2
                else:
                    room = max(2 * room, s.need_out)
        raise AssertionError("the decode does not end")

    def state_is_true(self, bits, out_at, content, base=(0, 0)):
        """the cursor stands on a boundary of the stream; window and check are those of the content in front of it"""
        cur = self.cur
        in_total, out_total = cur.in_total - base[0], cur.out_total - base[1]
        if cur.phase == BLOCKS:
            assert out_at.get(8 * in_total + cur.bit) == out_total, (cur, self.calls[-1])
        assert out_total == len(self.got) and bytes(self.got) == content[:out_total]
        assert cur.hist == min(cur.out_total, WINDOW)
        hist = min(out_total, WINDOW)
        assert cur.window[cur.hist - hist:cur.hist].cpu().numpy().tobytes() == content[out_total - hist:out_total]
        if not base[1]:
            assert cur.check == check_of(cur.wrap, content[:out_total]), self.calls[-1]


def decode_one(torch, fmt, data, out_cap):
    """chip_decode_batch of the whole stream as one unit -> (bytes, in_used, status)"""
    import compu_amd

    out = torch.zeros(out_cap + GUARD, dtype=torch.uint8, device="cuda")
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")  # noqa: E731
    out_len, in_used, status = compu_amd.decode_batch(SC.FMT[fmt], upload(torch, data), i64(0), i32(len(data)), out, i64(0), i32(out_cap))
    torch.cuda.synchronize()
    return out[:int(out_len[0])].cpu().numpy().tobytes(), int(in_used[0]), int(status[0])


# ---- 1. the listed inputs at the listed slabs, ample room ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt,data,first_bit,chunk_bytes,slabs", SC.parallel_inputs(), ids=[c[0] for c in SC.parallel_inputs()])
def test_slabs_give_the_content_on_the_parallel_path(gpu, name, fmt, data, first_bit, chunk_bytes, slabs):
    bits, out_at, content = SR.boundaries(data, first_bit, SC.TRAILER[fmt])
    assert content == zlib.decompress(data, SC.FMT[fmt])
    _, whole_used, whole_status = decode_one(gpu, fmt, data, len(content))
    assert whole_status == FINISHED
    for slab in slabs:
        model, _ = SR.calls(data, first_bit, chunk_bytes, slab, trailer=SC.TRAILER[fmt])
        d = Drive(gpu, SC.FMT[fmt], data, slab, len(content), chunk_bytes)
        for m in model:
            s = d.step()
            d.state_is_true(bits, out_at, content)
            assert (s.pos, s.slab, s.path, s.status, s.out_len) == (m.pos, m.slab, m.path, m.status, m.out_len), (slab, s, m)
            assert s.path == PARALLEL and s.n_starts == len(m.starts) and s.n_false == len(m.starts) - m.links
        assert s.status == FINISHED and d.cur.phase == DONE and d.pos == whole_used
        assert bytes(d.got) == content and d.cur.wrap == {"raw": 0, "zlib": 1, "gzip": 2}[fmt]
        assert d.step().status == FINISHED and len(d.got) == len(content)  # a finished cursor stays finished


# ---- 2. a block longer than the slab ------------------------------------------------------------------------------------------------
def test_block_longer_than_the_slab(gpu):
    import compu_amd

    s = PC.built_edges("zlib")
    bits, out_at, content = SR.boundaries(s.data, 8 * s.hdr_len, 4)
    d = Drive(gpu, 15, s.data, 2048, len(content), PC.EDGE_CHUNK)
    stuck = 0
    for _ in range(200):
        c = d.step()
        d.state_is_true(bits, out_at, content)
        if c.status == FINISHED:
            break
        if c.in_used == 0 and c.out_len == 0:
            assert c.status == NEED_INPUT and not c.moved
            stuck += 1
            c = d.step(slab=8192)  # the longest block is 5 898 bytes
            assert c.moved
    assert c.status == FINISHED and bytes(d.got) == content and stuck >= 1
    assert compu_amd.inflate_parallel_stream(s.data, slab_bytes=2048, chunk_bytes=PC.EDGE_CHUNK) == content


# ---- 3. room ------------------------------------------------------------------------------------------------------------------------
def test_room_shorter_than_a_chunk(gpu):
    s = PC.built_edges("gzip")
    bits, out_at, content = SR.boundaries(s.data, 8 * s.hdr_len, 8)
    d = Drive(gpu, 31, s.data, len(s.data), 64 << 10, PC.EDGE_CHUNK)
    short = 0
    for _ in range(400):
        c = d.step()
        d.state_is_true(bits, out_at, content)
        if c.status == FINISHED:
            break
        assert c.status == NEED_OUTPUT, c  # the slab holds the whole stream
        if c.out_len == 0 and c.in_used == 0:
            assert c.path == PARALLEL and c.need_out > (64 << 10) and not c.moved
            nxt = min(o for o in out_at.values() if o - d.cur.out_total >= c.need_out)
            assert nxt - d.cur.out_total == c.need_out, "need_out is the next chain chunk's size: it ends on a boundary"
            short += 1
            need = c.need_out
            c = d.step(room=need)
            assert c.out_len == need and c.moved, "success at need_out"
            d.state_is_true(bits, out_at, content)
            if c.status == FINISHED:
                break
    assert c.status == FINISHED and bytes(d.got) == content and short >= 1
    # room for some chunks and not all: the calls go on where the last one ended
    d = Drive(gpu, 31, s.data, len(s.data), 300 << 10, PC.EDGE_CHUNK)
    assert d.run().status == FINISHED and bytes(d.got) == content and len(d.calls) >= 3
    assert all(c.out_len <= (300 << 10) for c in d.calls)


# ---- 4. slabs without a start: one wave ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3), ids=["fixed", "stored", "chunk-edges"])
def test_serial_slabs(gpu, k):
    name, data, content, chunk_bytes, slabs = SC.serial_inputs()[k]
    bits, out_at, walked = SR.boundaries(data, 0, 0)
    assert walked == content
    for slab in slabs:
        model, _ = SR.calls(data, 0, chunk_bytes, slab)
        d = Drive(gpu, -15, data, slab, len(content), chunk_bytes)
        for m in model:
            at = d.pos
            s = d.step()
            d.state_is_true(bits, out_at, content)
            assert s.moved, (name, slab, s)
            if at == m.pos:  # (a wave may stop in front of the model's last boundary; then the calls part ways)
                assert s.path == m.path, (name, slab, s, m)
            if s.status == FINISHED:
                break
        if s.status != FINISHED:
            s = d.run()
        assert s.status == FINISHED and bytes(d.got) == content and d.pos == len(data)
        if name != "chunk-edges":  # (its two dynamic blocks are starts; the stored and fixed blocks around them are not)
            assert all(c.path == SERIAL and c.n_starts == 0 for c in d.calls)


# ---- 5. a false start ---------------------------------------------------------------------------------------------------------------
def test_false_start_costs_its_wave(gpu):
    s, at = PC.decoy(256)
    bits, out_at, content = SR.boundaries(s.data, 0, 0)
    for slab in (4096, 3000):
        assert 8 * 256 <= at < 8 * slab  # the decoy stands in the first slab, behind its first chunk
        d = Drive(gpu, -15, s.data, slab, len(content), 256)
        c = d.step()
        d.state_is_true(bits, out_at, content)
        assert c.path == PARALLEL and c.n_false >= 1 and c.out_len > 0
        assert d.run().status == FINISHED and bytes(d.got) == content


# ---- 6. header and trailer across slabs ---------------------------------------------------------------------------------------------
def test_header_and_trailer_across_slabs(gpu):
    data, first_bit = SC.alice_gzip_fields()
    content = IC.file_content("alice")
    bits, out_at, _ = SR.boundaries(data, first_bit, 8)
    d = Drive(gpu, 31, data, 20, len(content), 512)  # the header has 27 bytes
    c = d.step()
    assert (c.status, c.in_used, c.out_len, c.moved) == (NEED_INPUT, 0, 0, False) and d.cur.phase == HEADER
    c = d.step(slab=27)  # the header alone: the cursor moves behind it
    assert (c.status, c.in_used, c.out_len) == (NEED_INPUT, 27, 0) and d.cur.phase == BLOCKS and d.cur.wrap == 2
    d.slab = 8192
    assert d.run().status == FINISHED and bytes(d.got) == content
    for cut in (1, 4, 7):
        whole = len(data) - 8 + cut
        d = Drive(gpu, 47, data[:whole], 1 << 20, len(content), 512)
        c = d.step()
        d.state_is_true(bits, out_at, content)
        assert c.status == NEED_INPUT and d.cur.phase == TRAILER and c.out_len == len(content) and c.in_used == len(data) - 8
        c = d.step()
        assert (c.status, c.in_used, c.out_len, c.moved) == (NEED_INPUT, 0, 0, False)
        d.data, d.d_in = data + b"garbage behind the trailer", upload(gpu, data + b"garbage behind the trailer", 1)
        c = d.step()
        assert (c.status, c.in_used) == (FINISHED, 8) and d.cur.phase == DONE and d.pos == len(data)


# ---- 7. verdicts --------------------------------------------------------------------------------------------------------------------
def test_wrong_trailers_are_data_errors_behind_all_content(gpu):
    content = IC.file_content("alice")
    gz, zl = PC.alice("gzip")[0], PC.alice("zlib")[0]
    flip = lambda data, k: data[:k] + bytes([data[k] ^ 1]) + data[k + 1:]  # noqa: E731
    for fmt, data in ((31, flip(gz, len(gz) - 7)), (31, flip(gz, len(gz) - 2)), (15, flip(zl, len(zl) - 3))):
        d = Drive(gpu, fmt, data, 8192, len(content), 512)
        assert d.run().status == -3 and bytes(d.got) == content and d.cur.phase == ERROR and d.cur.error == -3
        assert all(c.status == NEED_INPUT for c in d.calls[:-1])
        c = d.step()
        assert (c.status, c.in_used, c.out_len) == (-3, 0, 0)  # sticky


def test_damage_in_the_middle(gpu):
    s = IC.damage("gzip")
    bit, good = next((r.bit, r.out) for r in s.layout if r.kind == "block" and r.block == 6)  # a dynamic block in the middle
    cases = []
    for name, at in (("invalid block type", bit + 1), ("invalid code lengths set", bit + 20), ("invalid bit length repeat", bit + 100)):
        data = bytearray(s.data)
        data[at >> 3] = (data[at >> 3] | 1 << (at & 7)) if at == bit + 1 else (data[at >> 3] ^ 1 << (at & 7))
        with pytest.raises(zlib.error, match=name):
            zlib.decompress(bytes(data), 31)
        cases.append((name, bytes(data)))
    for name, data in cases:
        for slab in (len(data), 1500):
            _, _, want = decode_one(gpu, "gzip", data, len(s.content))
            d = Drive(gpu, 31, data, slab, len(s.content), 256)
            c = d.run()
            assert c.status == want == -3 and d.cur.phase == ERROR and d.cur.error == -3, (name, slab, c)
            # zlib delivers `good` bytes in front of each of these; a prefix of the content, no shorter than that boundary's
            assert s.content.startswith(bytes(d.got)) and len(d.got) >= good, (name, slab, len(d.got), good)
            c = d.step()
            assert (c.status, c.in_used, c.out_len) == (-3, 0, 0)
    z = IC.damage("zlib")
    d = Drive(gpu, 15, W.zlib_header(fdict=True, dictid=0x12345678) + z.data[2:], 4096, len(z.content), 256)
    assert d.run().status == NEED_DICT and d.cur.phase == ERROR and not d.got
    assert d.step().status == NEED_DICT
    t = PC.too_far_back()
    for slab in (len(t.data), 2048):
        d = Drive(gpu, -15, t.data, slab, len(t.content) + 100, 256)
        assert d.run().status == -3 and t.content.startswith(bytes(d.got))


# ---- 8. totals beyond 2^32 ----------------------------------------------------------------------------------------------------------
def test_totals_are_64_bit(gpu):
    data, first_bit = PC.alice("gzip")
    content = IC.file_content("alice")
    add_in, add_out = 1 << 32, (1 << 32) - 70000
    fixed = data[:-4] + ((len(content) + add_out) & 0xFFFFFFFF).to_bytes(4, "little")
    bits, out_at, _ = SR.boundaries(data, first_bit, 8)
    d = Drive(gpu, 31, fixed, 8192, len(content), 512)
    c = d.step(slab=16384)  # (a full window, so that the cursor stays one a call could have left)
    assert WINDOW <= c.out_len < 70000 and c.status == NEED_INPUT
    d.cur.in_total += add_in
    d.cur.out_total += add_out
    wrapped = False
    while c.status == NEED_INPUT:
        low = d.cur.out_total & 0xFFFFFFFF
        c = d.step()
        wrapped |= (d.cur.out_total & 0xFFFFFFFF) < low
        d.state_is_true(bits, out_at, content, base=(add_in, add_out))
    assert c.status == FINISHED and wrapped and bytes(d.got) == content
    assert (d.cur.in_total, d.cur.out_total) == (add_in + len(data), add_out + len(content))
    assert d.cur.check == zlib.crc32(content)


# ---- 9. one slab --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", IC.WRAPPERS)
def test_one_slab_answers_as_inflate_parallel(gpu, fmt):
    import compu_amd

    s = PC.built_edges(fmt)
    out, summ = compu_amd.inflate_parallel(SC.FMT[fmt], upload(gpu, s.data), len(s.data), chunk_bytes=PC.EDGE_CHUNK)
    assert (summ.status, summ.path) == (FINISHED, PARALLEL)
    d = Drive(gpu, SC.FMT[fmt], s.data, len(s.data), len(s.content), PC.EDGE_CHUNK)
    c = d.step()
    assert (c.status, c.path, c.out_len, c.in_used) == (FINISHED, PARALLEL, summ.out_len, summ.in_used)
    assert bytes(d.got) == out.cpu().numpy().tobytes() == s.content
    assert (d.cur.out_total, d.cur.check, d.cur.wrap) == (summ.total_out, summ.check, summ.wrap)
    assert (c.n_starts, c.n_false) == (summ.n_starts, summ.n_false)


# ---- 10. bounded scratch ------------------------------------------------------------------------------------------------------------
def test_scratch_is_bounded_by_slab_and_room(gpu):
    import compu_amd

    data, content = SC.salted()
    d_in = upload(gpu, data)
    room = gpu.empty(8 << 20, dtype=gpu.uint8, device="cuda")
    cur = compu_amd.InflateCursor(15)
    pos, crc, total, free, calls = 0, 1, 0, [], 0
    while True:
        s = compu_amd.inflate_parallel_next(cur, d_in[pos:min(pos + (1 << 20), len(data))], room)
        gpu.cuda.synchronize()
        free.append(gpu.cuda.mem_get_info()[0])
        got = room[:s.out_len].cpu().numpy().tobytes()
        assert got == content[total:total + len(got)]
        pos, total, calls = pos + s.in_used, total + len(got), calls + 1
        if s.status == FINISHED:
            break
        assert s.status == NEED_INPUT and s.out_len > 0 and s.path == PARALLEL, s
    assert total == len(content) and cur.check == zlib.adler32(content) and calls >= 5
    assert min(free[2:]) >= free[1] - (1 << 20), "device memory in use does not grow after the second call"
    compu_amd.lib().chip_trim()
    assert gpu.cuda.mem_get_info()[0] > free[-1]


# ---- 11. the Python loop ------------------------------------------------------------------------------------------------------------
def test_python_stream(gpu):
    import compu_amd

    content = IC.file_content("alice")
    data = PC.alice("gzip")[0]
    assert compu_amd.inflate_parallel_stream(data, slab_bytes=8192, out_bytes=65536, chunk_bytes=512) == content
    assert compu_amd.inflate_parallel_stream(io.BytesIO(data), slab_bytes=5001, chunk_bytes=512) == content
    assert compu_amd.inflate_parallel_stream(PC.alice("raw")[0], slab_bytes=8192, chunk_bytes=512, fmt=-15) == content
    two = data + IC.compressed("alice", 6, "gzip")
    assert compu_amd.inflate_parallel_stream(two, slab_bytes=8192, chunk_bytes=512) == content  # the first member only
    assert compu_amd.inflate_parallel_stream(io.BytesIO(two), slab_bytes=8192, chunk_bytes=512, members=True) == content + content
    sink = io.BytesIO()
    assert compu_amd.inflate_parallel_stream(data, sink, slab_bytes=4096, chunk_bytes=512) == len(content) and sink.getvalue() == content
    with pytest.raises(compu_amd.DecodeError) as err:
        compu_amd.inflate_parallel_stream(data[:-3] + b"\x00\x00\x00", slab_bytes=8192, chunk_bytes=512)
    assert err.value.code == -3
    with pytest.raises(EOFError):
        compu_amd.inflate_parallel_stream(data[:-5], slab_bytes=8192, chunk_bytes=512)
    c = compu_amd.InflateCursor(31)
    s = compu_amd.inflate_parallel_next(c, upload(gpu, data)[:8192], gpu.empty(len(content), dtype=gpu.uint8, device="cuda"), 512)
    twin = c.copy()
    assert s.out_len > 0 and twin.raw is not c.raw and repr(twin) == repr(c) and gpu.equal(twin.window, c.window)
    twin.out_total += 1
    assert twin.out_total == c.out_total + 1
