"""LZ4 on the GPU: the CHIP_FMT_LZ4_BLOCK and CHIP_FMT_LZ4 batches and their size pass against tests/lz4_ref.py
and chip_lz4_block_decode_host over the case lists of tests/lz4_cases.py -- every unit of a list in ONE batch, at odd input
offsets, into poisoned output with an untouched-tail check behind every out_cap --, chip_lz4_blocks against its host form and the
reference walk, chip_lz4_parallel against the one-unit decode, chip_xxh32_batch against the reference XXH32.  Without the feature
every test fails: the tags answer CHIP_E_INVALID and the symbols are missing."""
import ctypes as C
import ctypes.util
import random

import numpy as np
import pytest

import lz4_cases as K
import lz4_ref as R
import lz4_writer as W

pytestmark = pytest.mark.gpu

FMT_LZ4_BLOCK, FMT_LZ4 = 102, 103
POISON, GAP = 0xC7, 24
SERIAL, PARALLEL, REFUSED = 0, 1, 2
NO_CHECKSUM = 1


@pytest.fixture(scope="module")
def torch(gpu):
    return gpu


def u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def expected(fmt, cases):
    """per case (content, out_len, in_used, status, cap) by the reference, with the room the case asks for"""
    dec = R.block_decode if fmt == FMT_LZ4_BLOCK else R.frame_decode
    count = R.block_decode if fmt == FMT_LZ4_BLOCK else (lambda d, cap: R.frame_decode(d, cap, checks=False))
    out = []
    for _, data, cap in cases:
        if cap is None:  # what the unit counts to where no checksum stops it, and a little
            cap = K.ample(count(data, None)[1])
        out.append(dec(data, cap) + (cap,))
    return out


_EXPECTED = {}


def expected_of(fmt):
    if fmt not in _EXPECTED:
        cases = K.block_cases() if fmt == FMT_LZ4_BLOCK else K.frame_cases()
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
    cases, want = expected_of(FMT_LZ4_BLOCK)
    return cases, want, run_batch(torch, FMT_LZ4_BLOCK, cases, want)


@pytest.fixture(scope="module")
def frame_run(torch):
    cases, want = expected_of(FMT_LZ4)
    return cases, want, run_batch(torch, FMT_LZ4, cases, want)


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
    assert not bad, bad[:8]


def test_block_batch_equals_the_reference(block_run):
    cases, want, run = block_run
    assert {w[3] for w in want} == {R.FINISHED, R.NEED_INPUT, R.NEED_OUTPUT, R.E_OFFSET}
    check_decode(cases, want, run)


def test_block_batch_equals_the_host_decoder(block_run):
    import compu_amd

    cases, want, run = block_run
    out, out_off, ol, iu, st = run[:5]
    for i, (name, data, _) in enumerate(cases):
        content, used, status = compu_amd.lz4_block_decode_host(data, want[i][4])
        o = int(out_off[i])
        assert (len(content), used, status) == (int(ol[i]), int(iu[i]), int(st[i])) and out[o:o + len(content)].tobytes() == content, name


def test_frame_batch_equals_the_reference(frame_run):
    cases, want, run = frame_run
    assert {w[3] for w in want} >= {R.FINISHED, R.NEED_INPUT, R.NEED_OUTPUT, R.E_HEADER, R.E_DICT, R.E_BLOCK_SIZE, R.E_BLOCK, R.E_OFFSET,
                                    R.E_BLOCK_CHECKSUM, R.E_CONTENT_SIZE, R.E_CONTENT_CHECKSUM}
    check_decode(cases, want, run)


@pytest.mark.parametrize("fmt", [FMT_LZ4_BLOCK, FMT_LZ4])
def test_size_pass_keeps_the_contract(fmt, block_run, frame_run):
    """rules 1 to 4 of chip_decode_batch_sizes, measured against the decode with ample room (lz4_ref, which the decode tests pin
    the kernel to): the same status, length and in_used, except that a unit whose only fault is an XXH32 comparison of a block
    or of the content finishes here"""
    cases, _, run = block_run if fmt == FMT_LZ4_BLOCK else frame_run
    size, siu, sst = run[5:]
    dec = R.block_decode if fmt == FMT_LZ4_BLOCK else (lambda d, cap: R.frame_decode(d, cap, checks=False))
    blind = 0
    for i, (name, data, _) in enumerate(cases):
        _, n, used, status = dec(data, None)
        assert status != R.NEED_OUTPUT
        assert (int(size[i]), int(siu[i]), int(sst[i])) == (n, used, status), name
        if fmt == FMT_LZ4:
            full = R.frame_decode(data, None)
            if full[3] != status:  # rule 4: the price of not producing the bytes
                assert status == R.FINISHED and full[3] in (R.E_BLOCK_CHECKSUM, R.E_CONTENT_CHECKSUM), name
                blind += 1
            else:
                assert full[1:] == (n, used, status), name
    assert fmt == FMT_LZ4_BLOCK or blind >= 5


def test_size_pass_counts_lengths_no_room_could_hold(torch):
    """lengths accumulate in 64 bits: 70 000 extension bytes of 255 are a match of 17.85 million bytes, and a run of them wraps nothing"""
    import compu_amd

    big = W.sequence(b"ab", 1, 19, ml_ext=b"\xff" * 70000 + b"\x07") + W.sequence(b"")
    want = R.block_decode(big, None, count_only=True)
    assert want[1:] == (2 + 19 + 255 * 70000 + 7, len(big), R.FINISHED)
    d_in = torch.from_numpy(np.frombuffer(big + b"\0" * 8, np.uint8).copy()).cuda()
    one = lambda v, dt: torch.tensor([v], dtype=torch.int64, device="cuda").to(dt)  # noqa: E731
    size, iu, st = compu_amd.decode_batch_sizes(FMT_LZ4_BLOCK, d_in, one(0, torch.int64), one(len(big), torch.int32))
    assert (int(size[0]), int(iu[0]), int(st[0])) == want[1:]
    out = torch.full((1000 + GAP,), POISON, dtype=torch.uint8, device="cuda")
    ol, iu, st = compu_amd.decode_batch(FMT_LZ4_BLOCK, d_in, one(0, torch.int64), one(len(big), torch.int32), out, one(0, torch.int64), one(1000, torch.int32))
    assert (int(ol[0]), int(iu[0]), int(st[0])) == (2, 0, R.NEED_OUTPUT) and (out.cpu().numpy()[1000:] == POISON).all()


def test_flags_are_refused(torch):
    import compu_amd

    t = torch.zeros(8, dtype=torch.uint8, device="cuda")
    z64, z32 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    for fmt in (FMT_LZ4_BLOCK, FMT_LZ4):
        for flags in (1, 2):
            with pytest.raises(RuntimeError, match="-101"):
                compu_amd.decode_batch(fmt, t, z64, z32, t, z64, z32, flags=flags)
        with pytest.raises(RuntimeError, match="-101"):
            compu_amd.decode_batch_sizes(fmt, t, z64, z32, flags=2)


def test_host_batch_takes_the_tags():
    import compu_amd

    cases = [c for c in K.frame_cases() if c[0].startswith("flags_")]
    want = expected(FMT_LZ4, cases)
    blob, offs = pack(cases)
    caps = [w[4] for w in want]
    out_off = np.concatenate(([0], np.cumsum(caps))).astype(np.uint64)
    out = np.full(int(out_off[-1]) + 8, POISON, np.uint8)
    ol, iu, st = compu_amd.decode_batch_host(FMT_LZ4, np.frombuffer(blob, np.uint8), np.asarray(offs, np.uint64), np.asarray([len(c[1]) for c in cases], np.uint32),
                                             out, out_off[:-1], np.asarray(caps, np.uint32))
    for i, w in enumerate(want):
        assert (int(ol[i]), int(iu[i]), int(st[i])) == w[1:4] and out[int(out_off[i]):int(out_off[i]) + w[1]].tobytes() == w[0]


# ---- chip_lz4_blocks ---------------------------------------------------------------------------------------------------------------


def upload(torch, data):
    t = torch.full(((len(data) + 3) // 4 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


def device_walk(torch, data, max_blocks=None):
    import compu_amd

    blocks, summ = compu_amd.lz4_blocks(upload(torch, data), len(data), max_blocks=max_blocks)
    rows = blocks.cpu().numpy().reshape(-1).view(compu_amd.lz4_block_dtype())
    return [tuple(int(v) for v in r)[:4] for r in rows.tolist()], summ.as_tuple()


def test_blocks_device_equals_host_equals_reference(torch):
    import compu_amd

    names = ("flags_l0b1c1c1", "flags_l1b0c0c0", "stored_mixed", "no_block", "short_middle", "trailing", "magic_legacy", "bad_hc", "dict_id",
             "size_field_above_max", "size_field_above_max_absent", "no_end_mark", "cut5", "cut6", "cut7", "cut14", "cut15", "cut40", "cut150")
    by_name = {c[0]: c[1] for c in K.frame_cases()}
    statuses = set()
    for name in names:
        data = by_name[name]
        want = R.blocks_walk(data)
        statuses.add(want[1][8])
        host = compu_amd.lz4_blocks_host(data)
        assert ([tuple(int(v) for v in r)[:4] for r in host[0].tolist()], host[1].as_tuple()) == want, name
        assert device_walk(torch, data) == want, name
        n = want[1][0]
        for m in sorted({0, 1, n}):  # count, then fill; LAST only on a record that is written
            assert device_walk(torch, data, m) == R.blocks_walk(data, m), (name, m)
    assert statuses == {R.OK, R.TRUNCATED, R.BAD_HEADER}


def test_blocks_too_large(torch):
    """2^20 + 1 empty stored blocks: the walk follows 2^20 of them"""
    data = W.header() + b"\x00\x00\x00\x80" * (R.MAX_BLOCKS + 1) + b"\0\0\0\0"
    rows, summ = device_walk(torch, data, 3)
    assert summ == (R.MAX_BLOCKS, 0, R.UNSIZED, 65536, 0x60, 0x40, 7, 0, R.TOO_LARGE)
    assert rows == [(7 + 4 * i, 0, R.STORED, 0) for i in range(3)]
    assert device_walk(torch, data[:-8], 0)[1] == (R.MAX_BLOCKS, 0, R.UNSIZED, 65536, 0x60, 0x40, 7, 0, R.TRUNCATED)


# ---- chip_lz4_parallel --------------------------------------------------------------------------------------------------------------


def one_unit(torch, data, cap):
    import compu_amd

    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda").to(torch.int32)  # noqa: E731
    out = torch.full((cap + GAP,), POISON, dtype=torch.uint8, device="cuda")
    ol, iu, st = compu_amd.decode_batch(FMT_LZ4, upload(torch, data), i64(0), i32(len(data)), out, i64(0), i32(cap))
    torch.cuda.synchronize()
    n = int(ol[0]) & 0xFFFFFFFF
    return out.cpu().numpy()[:n].tobytes(), n, int(iu[0]) & 0xFFFFFFFF, int(st[0])


def par(torch, data, cap, flags=0):
    """chip_lz4_parallel into a poisoned room of cap + GAP bytes: (bytes, summary)"""
    import compu_amd
    from compu_amd.api import _Lz4ParallelSummary

    d_in = upload(torch, data)
    out = torch.full((cap + GAP,), POISON, dtype=torch.uint8, device="cuda")
    s = _Lz4ParallelSummary()
    rc = compu_amd.lib().chip_lz4_parallel(C.c_void_p(d_in.data_ptr()), len(data), C.c_void_p(out.data_ptr()), cap, flags, C.byref(s),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = out.cpu().numpy()
    summ = compu_amd.Lz4ParallelSummary(s)
    assert (got[summ.out_len if summ.path == PARALLEL else cap:] == POISON).all(), "bytes behind out_len were written"
    return got[:summ.out_len].tobytes(), summ


@pytest.mark.parametrize("name,data,sizes", K.parallel_frames(), ids=[p[0] for p in K.parallel_frames()])
def test_parallel_equals_the_one_unit_decode(torch, name, data, sizes):
    for bchk, csize, cchk, stored in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 2), (0, 0, 1, 0), (1, 1, 1, 3)):
        frame = W.frame_of(data, sizes, bchk=bool(bchk), csize=bool(csize), cchk=bool(cchk), stored_every=stored) + b"trailing"
        want = one_unit(torch, frame, len(data))
        assert want == (data, len(data), len(frame) - 8, R.FINISHED)
        got, s = par(torch, frame, len(data))
        assert s.path == PARALLEL, s
        assert (got, s.out_len, s.in_used, s.status, s.total_out, s.n_blocks) == (data, len(data), len(frame) - 8, R.FINISHED, len(data), len(sizes))
        assert s.check == (R.xxh32(data) if cchk else 0)


def test_parallel_linked_frame_is_serial(torch):
    _, data, sizes = K.parallel_frames()[1]
    frame = W.frame_of(data, sizes, linked=True, cchk=True)
    want = one_unit(torch, frame, len(data))
    got, s = par(torch, frame, len(data))
    assert want[3] == R.FINISHED and s.path == SERIAL and (got, s.out_len, s.in_used, s.status) == want


def test_parallel_tight_room(torch):
    _, data, sizes = K.parallel_frames()[2]
    frame = W.frame_of(data, sizes, cchk=True, cchk_value=77)  # (no checksum is compared by the call that has no room)
    for cap in (0, len(data) - 1):
        got, s = par(torch, frame, cap)
        assert (s.path, s.status, s.out_len, s.total_out, got) == (PARALLEL, R.NEED_OUTPUT, 0, len(data), b"")


def test_parallel_checksum_mismatches_get_the_serial_answer(torch):
    _, data, sizes = K.parallel_frames()[1]
    for frame, status in ((W.frame_of(data, sizes, bchk=True, cchk=True, bchk_values={1: 0xBAD}), R.E_BLOCK_CHECKSUM),
                          (W.frame_of(data, sizes, bchk=True, cchk=True, cchk_value=0xBAD), R.E_CONTENT_CHECKSUM),
                          (W.frame_of(data, sizes, csize=True, csize_value=len(data) + 1), R.E_CONTENT_SIZE)):
        want = one_unit(torch, frame, len(data))
        assert want[3] == status
        got, s = par(torch, frame, len(data))
        assert s.path == SERIAL and (got, s.out_len, s.in_used, s.status) == want
    frame = W.frame_of(data, sizes, cchk=True, cchk_value=0xBAD)
    got, s = par(torch, frame, len(data), NO_CHECKSUM)
    assert (s.path, s.status, got, s.in_used, s.check) == (PARALLEL, R.FINISHED, data, len(frame), 0)


def test_parallel_damaged_block_and_single_block_are_serial(torch):
    _, data, sizes = K.parallel_frames()[1]
    blocks = [(False, W.compress_block(data[:3000])), (False, W.block([(b"abcd", 9, 6)], b"x")), (True, b"tail")]
    for frame in (W.frame(blocks, content=b""), W.frame_of(data[:500], [500], cchk=True)):
        want = one_unit(torch, frame, 4000)
        got, s = par(torch, frame, 4000)
        assert s.path == SERIAL and (got, s.out_len, s.in_used, s.status) == want


def test_lz4_decode_and_tar_open(torch):
    """whole-file contents: concatenated frames with a skippable frame between them; a .tar.lz4"""
    import io
    import tarfile

    import compu_amd

    a, b = K.text(5000, 1), K.noise(300, 2)
    blob = W.frame_of(a, 2000, cchk=True) + b"\x53\x2a\x4d\x18\x05\x00\x00\x00hello" + W.frame_of(b, 300, stored_every=1) + W.frame([])
    assert compu_amd.lz4_decode(blob).cpu().numpy().tobytes() == a + b
    with pytest.raises(ValueError):
        compu_amd.lz4_decode(blob + b"\x02\x21\x4c\x18")
    bio = io.BytesIO()
    with tarfile.open(fileobj=bio, mode="w", format=tarfile.USTAR_FORMAT) as tf:
        for name, body in (("a.txt", a), ("dir/b.bin", b)):
            ti = tarfile.TarInfo(name)
            ti.size = len(body)
            tf.addfile(ti, io.BytesIO(body))
    image = bio.getvalue()
    packed = W.frame_of(image, 4096, cchk=True)
    ar = compu_amd.tar_open(upload(torch, packed), len(packed))
    assert ar.names == [b"a.txt", b"dir/b.bin"] and ar.member("dir/b.bin").cpu().numpy().tobytes() == b


def test_golden_fixtures_on_the_device(torch):
    """what liblz4 wrote (tests/golden/lz4): both texts as raw blocks of both compressors in one batch, and as frames through the
    one-unit decode and chip_lz4_parallel -- LZ4F's default frame has linked blocks (serial), the full one independent blocks with
    every checksum (parallel where it has two blocks or more)"""
    import os

    import compu_amd

    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    read = lambda name: open(os.path.join(root, name), "rb").read()  # noqa: E731
    texts = {name: read(name) for name in ("10x10y", "alice29.txt")}
    cases = [(f"{name}.{kind}", read(f"lz4/{name}.{kind}.block"), len(texts[name])) for name in texts for kind in ("default", "hc")]
    want = [(texts[c[0].rsplit(".", 1)[0]], c[2], len(c[1]), R.FINISHED, c[2]) for c in cases]
    check_decode(cases, want, run_batch(torch, FMT_LZ4_BLOCK, cases, want))
    for name, data in texts.items():
        for kind in ("default", "full"):
            frame = read(f"lz4/{name}.{kind}.lz4")
            assert one_unit(torch, frame, len(data)) == (data, len(data), len(frame), R.FINISHED)
            got, s = par(torch, frame, len(data))
            assert (got, s.out_len, s.in_used, s.status) == (data, len(data), len(frame), R.FINISHED)
            assert s.path == (PARALLEL if (kind, name) == ("full", "alice29.txt") else SERIAL), (name, kind, s)


# ---- chip_xxh32_batch ---------------------------------------------------------------------------------------------------------------


def test_xxh32_batch(torch):
    import compu_amd

    lens = list(range(41)) + [4095, 4096, 4097, 100000]
    rng = random.Random(5)
    blob, offs = bytearray(b"\x11"), []
    for n in lens:
        offs.append(len(blob))
        blob += rng.randbytes(n) + b"\x22" * rng.randrange(1, 4)
    d = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).cuda()
    off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    ln = torch.tensor(lens, dtype=torch.int64, device="cuda").to(torch.int32)
    xx = ctypes.util.find_library("xxhash")
    lib = C.CDLL(xx) if xx else None
    if lib:
        lib.XXH32.restype = C.c_uint32
    for seed in (0, 1):
        got = u32(compu_amd.xxh32_batch(d, off, ln, seed=seed))
        for i, n in enumerate(lens):
            piece = bytes(blob[offs[i]:offs[i] + n])
            assert int(got[i]) == R.xxh32(piece, seed), (n, seed)
            if lib:
                assert int(got[i]) == lib.XXH32(piece, n, seed)
    assert compu_amd.xxh32_batch(d, off[:0], ln[:0]).numel() == 0
