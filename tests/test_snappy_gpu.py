"""Snappy on the GPU: the CHIP_FMT_SNAPPY_BLOCK and CHIP_FMT_SNAPPY batches and their size pass against
tests/snappy_ref.py and chip_snappy_block_decode_host over the case lists of tests/snappy_cases.py -- every unit of a list in ONE
batch, at odd input offsets, into poisoned output with an untouched-tail check behind every out_cap --, chip_snappy_chunks against
its host form and the reference walk, chip_crc32c_batch against the reference CRC, chip_snappy_parallel against the one-unit decode,
the golden fixtures and the two whole-file helpers.  Without the feature every test fails: the tags answer CHIP_E_INVALID and the
symbols are missing."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import snappy_cases as K
import snappy_ref as R
import snappy_writer as W

pytestmark = pytest.mark.gpu

FMT_SNAPPY_BLOCK, FMT_SNAPPY = 104, 105
POISON, GAP = 0xC7, 24
SERIAL, PARALLEL, REFUSED = 0, 1, 2


@pytest.fixture(scope="module")
def torch(gpu):
    return gpu


def u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def expected(fmt, cases):
    """per case (content, out_len, in_used, status, cap) by the reference, with the room the case asks for"""
    out = []
    for _, data, cap in cases:
        if cap is None:
            cap = K.ample_block(data) if fmt == FMT_SNAPPY_BLOCK else K.ample_frame(data)
        out.append((R.block_decode if fmt == FMT_SNAPPY_BLOCK else R.frame_decode)(data, cap) + (cap,))
    return out


_EXPECTED = {}


def expected_of(fmt):
    if fmt not in _EXPECTED:
        cases = K.block_cases() if fmt == FMT_SNAPPY_BLOCK else K.frame_cases()
        _EXPECTED[fmt] = (cases, expected(fmt, cases))
    return _EXPECTED[fmt]


def pack(cases):
    """the units' bytes at odd offsets (every unit starts at an odd address, one byte of 0xEE filler at least between two units)"""
    buf, offs = bytearray(), []
    for _, data, _ in cases:
        buf += b"\xee" if len(buf) % 2 == 0 else b"\xee\xee"
        offs.append(len(buf))
        buf += data
    buf += b"\xee" * (4 - len(buf) % 4)
    return bytes(buf), offs


def run_batch(torch, fmt, cases, want):
    import compu_amd

    blob, offs = pack(cases)
    assert all(o % 2 == 1 for o in offs)
    caps = [w[4] for w in want]
    out_off = np.concatenate(([0], np.cumsum([c + GAP for c in caps]))).astype(np.int64)
    d_in = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    d_out = torch.full((int(out_off[-1]) + GAP,), POISON, dtype=torch.uint8, device="cuda")
    dev = lambda a, dt: torch.from_numpy(np.asarray(a, np.int64)).cuda().to(dt)  # noqa: E731
    in_off, in_len = dev(offs, torch.int64), dev([len(c[1]) for c in cases], torch.int32)
    ol, iu, st = compu_amd.decode_batch(fmt, d_in, in_off, in_len, d_out, dev(out_off[:-1], torch.int64), dev(caps, torch.int32))
    size, siu, sst = compu_amd.decode_batch_sizes(fmt, d_in, in_off, in_len)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_off, u32(ol), u32(iu), st.cpu().numpy(), size.cpu().numpy(), u32(siu), sst.cpu().numpy()


@pytest.fixture(scope="module")
def block_run(torch):
    cases, want = expected_of(FMT_SNAPPY_BLOCK)
    return cases, want, run_batch(torch, FMT_SNAPPY_BLOCK, cases, want)


@pytest.fixture(scope="module")
def frame_run(torch):
    cases, want = expected_of(FMT_SNAPPY)
    return cases, want, run_batch(torch, FMT_SNAPPY, cases, want)


def check_decode(cases, want, run):
    out, out_off, ol, iu, st = run[:5]
    bad = []
    for i, ((name, _, _), (content, n, used, status, cap)) in enumerate(zip(cases, want)):
        o = int(out_off[i])
        got = (int(ol[i]), int(iu[i]), int(st[i]))
        if got != (n, used, status) or out[o:o + n].tobytes() != content:
            bad.append((name, got, (n, used, status)))
        elif not (out[o + cap:int(out_off[i + 1])] == POISON).all():
            bad.append((name, "bytes behind out_cap were written"))
    assert not bad, (len(bad), bad[:8])


def test_block_batch_equals_the_reference(block_run):
    cases, want, run = block_run
    assert {w[3] for w in want} == {R.FINISHED, R.NEED_INPUT, R.NEED_OUTPUT, R.E_PREAMBLE, R.E_OFFSET, R.E_LENGTH}
    check_decode(cases, want, run)


def test_block_batch_equals_the_host_decoder(block_run):
    from compu_amd import snappy

    cases, want, run = block_run
    out, out_off, ol, iu, st = run[:5]
    for i, (name, data, _) in enumerate(cases):
        content, used, status = snappy.snappy_block_decode_host(data, want[i][4])
        o = int(out_off[i])
        assert (len(content), used, status) == (int(ol[i]), int(iu[i]), int(st[i])) and out[o:o + len(content)].tobytes() == content, name


def test_frame_batch_equals_the_reference(frame_run):
    cases, want, run = frame_run
    assert {w[3] for w in want} == {R.FINISHED, R.NEED_INPUT, R.NEED_OUTPUT, R.E_PREAMBLE, R.E_OFFSET, R.E_LENGTH, R.E_HEADER, R.E_CHUNK,
                                    R.E_CHUNK_SIZE, R.E_BLOCK, R.E_CHECKSUM}
    check_decode(cases, want, run)


@pytest.mark.parametrize("fmt", [FMT_SNAPPY_BLOCK, FMT_SNAPPY])
def test_size_pass_keeps_the_contract(fmt, block_run, frame_run):
    """rules 1 to 4 of chip_decode_batch_sizes, measured against the decode with ample room (snappy_ref, which the decode tests pin
    the kernel to): the same status, length and in_used on every unit, except that a CRC-32C is not compared -- a unit whose decode
    stops at CHIP_SNAPPY_E_CHECKSUM is walked on"""
    cases, _, run = block_run if fmt == FMT_SNAPPY_BLOCK else frame_run
    size, siu, sst = run[5:]
    blind = 0
    for i, (name, data, _) in enumerate(cases):
        if fmt == FMT_SNAPPY_BLOCK:
            _, n, used, status = R.block_decode(data, None)
        else:
            _, n, used, status = R.frame_decode(data, None, checks=False)
            full = R.frame_decode(data, None)[1:]
            if full != (n, used, status):  # rule 4: the price of not producing the bytes
                assert full[2] == R.E_CHECKSUM, name
                blind += 1
        assert status != R.NEED_OUTPUT
        assert (int(size[i]), int(siu[i]), int(sst[i])) == (n, used, status), name
    assert fmt == FMT_SNAPPY_BLOCK or blind >= 5


def test_flags_are_refused(torch):
    import compu_amd

    t = torch.zeros(8, dtype=torch.uint8, device="cuda")
    z64, z32 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    for fmt in (FMT_SNAPPY_BLOCK, FMT_SNAPPY):
        for flags in (1, 2):
            with pytest.raises(RuntimeError, match="-101"):
                compu_amd.decode_batch(fmt, t, z64, z32, t, z64, z32, flags=flags)
        with pytest.raises(RuntimeError, match="-101"):
            compu_amd.decode_batch_sizes(fmt, t, z64, z32, flags=2)


def test_encode_entry_points_still_refuse_the_tags(torch):
    import compu_amd

    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    z64, l32 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 16, dtype=torch.int32, device="cuda")
    host = np.zeros(64, np.uint8)
    for fmt in (FMT_SNAPPY_BLOCK, FMT_SNAPPY):
        with pytest.raises(RuntimeError, match="-101"):
            compu_amd.encode_batch(fmt, 1, t, z64, l32, t, z64, l32)
        with pytest.raises(RuntimeError, match="chip_encode_batch_host failed"):
            compu_amd.encode_batch_host(fmt, 1, host, np.zeros(1, np.uint64), np.full(1, 16, np.uint32), host, np.zeros(1, np.uint64), np.full(1, 64, np.uint32))
        with pytest.raises((RuntimeError, ValueError)):
            compu_amd.encode_file(fmt, 1, t, 16)


def test_host_batch_takes_the_tags():
    import compu_amd

    for fmt, cases in ((FMT_SNAPPY, [c for c in K.frame_cases() if not c[0].startswith("cut")][:40]),
                       (FMT_SNAPPY_BLOCK, [c for c in K.block_cases() if c[0].startswith(("elems", "copy1_off7_", "n_", "preamble"))])):
        want = expected(fmt, cases)
        blob, offs = pack(cases)
        caps = [w[4] for w in want]
        out_off = np.concatenate(([0], np.cumsum(caps))).astype(np.uint64)
        out = np.full(int(out_off[-1]) + 8, POISON, np.uint8)
        ol, iu, st = compu_amd.decode_batch_host(fmt, np.frombuffer(blob, np.uint8), np.asarray(offs, np.uint64), np.asarray([len(c[1]) for c in cases], np.uint32),
                                                 out, out_off[:-1], np.asarray(caps, np.uint32))
        for i, w in enumerate(want):
            assert (int(ol[i]), int(iu[i]), int(st[i])) == w[1:4] and out[int(out_off[i]):int(out_off[i]) + w[1]].tobytes() == w[0], cases[i][0]


# ---- chip_snappy_chunks ------------------------------------------------------------------------------------------------------------


def upload(torch, data):
    t = torch.full(((len(data) + 3) // 4 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


def device_walk(torch, data, max_chunks=None):
    from compu_amd import snappy

    chunks, summ = snappy.snappy_chunks(upload(torch, data), len(data), max_chunks=max_chunks)
    rows = chunks.cpu().numpy().reshape(-1).view(snappy.snappy_chunk_dtype())
    return [tuple(int(v) for v in r)[:4] for r in rows.tolist()], summ.as_tuple()


def test_chunks_device_equals_host_equals_reference(torch):
    from compu_amd import snappy

    names = ("three_chunks", "ident_alone", "no_ident", "ident_wrong_length", "ident_repeated", "ident_repeated_wrong", "empty_chunks", "type0_s3",
             "type1_s0", "padding", "skippable_80", "skippable_fd", "reserved_02", "reserved_7f", "bad_crc1", "block_cut_inside", "reserved_and_cut",
             "s3_and_cut", "header_cut_3", "cut0", "cut3", "cut5", "cut9", "cut10", "cut13", "cut14", "cut100", "cut200")
    by_name = {c[0]: c[1] for c in K.frame_cases()}
    statuses = set()
    for name in names:
        data = by_name[name]
        want = R.chunks_walk(data)
        statuses.add(want[1][3])
        host = snappy.snappy_chunks_host(data)
        assert ([tuple(int(v) for v in r)[:4] for r in host[0].tolist()], host[1].as_tuple()) == want, name
        assert device_walk(torch, data) == want, name
        for m in sorted({0, 1, want[1][0]}):  # count, then fill; an early stop of the caller's
            assert device_walk(torch, data, m) == R.chunks_walk(data, m), (name, m)
    assert statuses == {R.OK, R.TRUNCATED, R.BAD_HEADER}


# ---- chip_crc32c_batch -------------------------------------------------------------------------------------------------------------


def test_crc32c_batch(torch):
    from compu_amd import snappy

    lens = list(range(41)) + [4095, 4096, 4097, 100000]
    rng = random.Random(5)
    blob, offs = bytearray(b"\x11"), []
    for n in lens:
        offs.append(len(blob))
        blob += rng.randbytes(n) + b"\x22" * rng.randrange(1, 4)
    offs.append(len(blob))
    lens.append(9)
    blob += b"123456789"
    d = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).cuda()
    off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    ln = torch.tensor(lens, dtype=torch.int64, device="cuda").to(torch.int32)
    got = u32(snappy.crc32c_batch(d, off, ln))
    for i, n in enumerate(lens):
        assert int(got[i]) == R.crc32c(bytes(blob[offs[i]:offs[i] + n])), n
    assert int(got[-1]) == 0xE3069283
    assert snappy.crc32c_batch(d, off[:0], ln[:0]).numel() == 0


# ---- chip_snappy_parallel ------------------------------------------------------------------------------------------------------------


def one_unit(torch, data, cap):
    import compu_amd

    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda").to(torch.int32)  # noqa: E731
    out = torch.full((cap + GAP,), POISON, dtype=torch.uint8, device="cuda")
    ol, iu, st = compu_amd.decode_batch(FMT_SNAPPY, upload(torch, data), i64(0), i32(len(data)), out, i64(0), i32(cap))
    torch.cuda.synchronize()
    n = int(ol[0]) & 0xFFFFFFFF
    return out.cpu().numpy()[:n].tobytes(), n, int(iu[0]) & 0xFFFFFFFF, int(st[0])


def par(torch, data, cap):
    """chip_snappy_parallel into a poisoned room of cap + GAP bytes: (bytes, summary)"""
    import compu_amd
    from compu_amd import snappy
    from compu_amd._ffi import _SnappyParallelSummary

    d_in = upload(torch, data)
    out = torch.full((cap + GAP,), POISON, dtype=torch.uint8, device="cuda")
    s = _SnappyParallelSummary()
    rc = compu_amd.lib().chip_snappy_parallel(C.c_void_p(d_in.data_ptr()), len(data), C.c_void_p(out.data_ptr()), cap, 0, C.byref(s),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = out.cpu().numpy()
    summ = snappy.SnappyParallelSummary(s)
    assert (got[summ.out_len if summ.path == PARALLEL else cap:] == POISON).all(), "bytes behind out_len were written"
    return got[:summ.out_len].tobytes(), summ


@pytest.mark.parametrize("name,stream,data,n,skipped", K.parallel_streams(), ids=[p[0] for p in K.parallel_streams()])
def test_parallel_equals_the_one_unit_decode(torch, name, stream, data, n, skipped):
    want = one_unit(torch, stream, len(data))
    assert want == (data, len(data), len(stream), R.FINISHED)
    got, s = par(torch, stream, len(data))
    assert s.path == PARALLEL, s
    assert (got, s.out_len, s.in_used, s.status, s.total_out, s.n_chunks, s.n_skipped) == (data, len(data), len(stream), R.FINISHED, len(data), n, skipped)


def test_parallel_tight_room(torch):
    _, stream, data, _, _ = K.parallel_streams()[2]
    for cap in (0, len(data) - 1):
        assert one_unit(torch, stream, cap)[3] == R.NEED_OUTPUT
        got, s = par(torch, stream, cap)
        assert (s.path, s.status, s.out_len, s.total_out, got) == (PARALLEL, R.NEED_OUTPUT, 0, len(data), b"")


def test_parallel_gets_the_serial_answer_for_anything_not_clean(torch):
    data = K.text(4000, 3)
    good = [W.data_chunk(data[:1500]), W.data_chunk(data[1500:2500], compressed=False), W.data_chunk(data[2500:])]
    blk = W.compress_block(data[:1500])
    streams = {
        "wrong_crc": ([good[0], W.data_chunk(data[1500:2500], compressed=False, crc=0xBAD), good[2]], R.E_CHECKSUM),
        "wrong_crc_compressed": ([good[0], good[1], W.data_chunk(data[2500:], crc=0xBAD)], R.E_CHECKSUM),
        "damaged": ([good[1], W.data_chunk(b"", body=blk[:40]), good[2]], R.E_BLOCK),
        "trailing_byte": ([good[1], W.data_chunk(data[:1500], body=blk + b"\0"), good[2]], R.E_LENGTH),
        "single": ([good[0]], R.FINISHED),
        "cut": ([good[0], good[1], good[2][:30]], R.NEED_INPUT),
        "ident_repeated_wrong": ([good[0], b"\xff\x06\x00\x00sNaPpy", good[1]], R.E_HEADER),
        "too_large": ([good[0], W.data_chunk(K.noise(65537, 1), compressed=False)], R.E_CHUNK_SIZE),
        "reserved": ([good[0], W.chunk(0x7F, b""), good[1]], R.E_CHUNK),
    }
    for name, (chunks, status) in streams.items():
        stream = W.stream(chunks)
        want = one_unit(torch, stream, 70000)
        assert want[3] == status, name
        got, s = par(torch, stream, 70000)
        assert s.path == SERIAL and (got, s.out_len, s.in_used, s.status) == want, (name, s)
    # a repeated identifier is stepped over: still a wave per chunk
    stream = W.stream([good[0], R.IDENT, good[1], R.IDENT, good[2]])
    got, s = par(torch, stream, len(data))
    assert (s.path, got, s.in_used, s.status, s.n_chunks, s.n_skipped) == (PARALLEL, data, len(stream), R.FINISHED, 3, 2)
    assert one_unit(torch, stream, len(data)) == (data, len(data), len(stream), R.FINISHED)


def test_golden_fixtures_on_the_device(torch):
    """what libsnappy wrote (tests/golden/snappy): both texts as raw blocks in one batch"""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    read = lambda name: open(os.path.join(root, name), "rb").read()  # noqa: E731
    texts = {name: read(name) for name in ("10x10y", "alice29.txt")}
    cases = [(name, read(f"snappy/{name}.block"), len(texts[name])) for name in texts]
    want = [(texts[c[0]], c[2], len(c[1]), R.FINISHED, c[2]) for c in cases]
    check_decode(cases, want, run_batch(torch, FMT_SNAPPY_BLOCK, cases, want))


def test_snappy_decode_and_blocks_decode(torch):
    from compu_amd import snappy

    a, b = K.text(150000, 1), K.noise(300, 2)
    sz = W.stream_of(a + b, 65536, stored_every=3, between=(W.padding(2),))
    assert snappy.snappy_decode(sz).cpu().numpy().tobytes() == a + b
    assert snappy.snappy_decode(R.IDENT).numel() == 0
    with pytest.raises(ValueError, match="status -217"):
        snappy.snappy_decode(W.stream([W.data_chunk(a[:100]), W.data_chunk(b, crc=1)]))
    pages = [a[:70000], b, b"", a[:1], a[70000:]]
    outs = snappy.snappy_blocks_decode([W.compress_block(p) for p in pages])
    assert [o.cpu().numpy().tobytes() for o in outs] == pages
    assert snappy.snappy_blocks_decode([]) == []
    with pytest.raises(ValueError):
        snappy.snappy_blocks_decode([b"\x80"])
    with pytest.raises(RuntimeError, match="block 1"):
        snappy.snappy_blocks_decode([W.compress_block(b), W.compress_block(a[:500])[:-3]])
