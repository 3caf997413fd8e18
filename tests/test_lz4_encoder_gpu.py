"""The LZ4 encoder on the GPU.  The kernel against the host form, byte for byte (chip_lz4_block_encode_host and
chip_lz4_frame_encode_host define the bytes): every built input of tests/lz4_enc_cases.py in ONE batch per finder group, at odd
offsets, a 0xA5 canary behind every unit's room, a 1 MiB unit among the small ones; the same unit 256 times; exact room and one byte
less per unit; frames of every option, decoded again by chip_decode_batch.  Then chip_encode_file(CHIP_FMT_LZ4): ONE frame equal to
the frame assembled here from the host blocks, read by the reference, by chip_lz4_parallel on its parallel path and by tar_open.
Without the feature every test fails at its first call (CHIP_E_INVALID)."""
import numpy as np
import pytest

import lz4_cases as K
import lz4_enc_cases as E
import lz4_ref as R

pytestmark = pytest.mark.gpu
PAD = 64


def _place(sizes, gap):
    """odd offsets for ranges of `sizes` bytes with `gap` bytes between them"""
    off, at = [], 1
    for s in sizes:
        off.append(at)
        at = (at + s + gap) | 1
    return np.array(off, np.int64), at


def _enc(torch, fmt, datas, level, strategy=0, caps=None):
    """chip_encode_batch_ex at odd in_off / out_off with a 0xA5 canary behind every unit's room -> (units or None, status, out_len)"""
    import compu_amd as c

    dev = torch.device("cuda:0")
    in_len = np.array([len(d) for d in datas], np.int64)
    in_off, total_in = _place(in_len, 3)
    buf = np.zeros((total_in + 8) // 4 * 4, np.uint8)
    for o, d in zip(in_off, datas):
        buf[o:o + len(d)] = np.frombuffer(d, np.uint8)
    caps = np.array([c.encode_bound(fmt, len(d)) for d in datas] if caps is None else caps, np.int64)
    out_off, total_out = _place(caps, PAD)
    d_out = torch.full((total_out + PAD,), 0xA5, dtype=torch.uint8, device=dev)
    out_len, status = c.encode_batch(fmt, level, torch.from_numpy(buf).to(dev), torch.from_numpy(in_off).to(dev),
                                     torch.from_numpy(in_len.astype(np.int32)).to(dev), d_out, torch.from_numpy(out_off).to(dev),
                                     torch.from_numpy(caps.astype(np.int32)).to(dev), strategy=strategy)
    torch.cuda.synchronize()
    out, ol, st = d_out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    units = []
    for i in range(len(datas)):
        assert (out[out_off[i] + caps[i]:out_off[i] + caps[i] + PAD] == 0xA5).all(), f"unit {i} wrote at or past its out_cap"
        assert (out[out_off[i] - 1] == 0xA5), f"unit {i} wrote in front of its room"
        units.append(bytes(out[out_off[i]:out_off[i] + ol[i]]) if st[i] == 2 else None)
    return units, st, ol


_HOST = {}


def host_blocks(level):
    """the host form's blocks of every input, made once per level and left unchanged"""
    import compu_amd as c

    if level not in _HOST:
        _HOST[level] = tuple(c.lz4_block_encode_host(d, level)[0] for _, d in E.inputs())
    return _HOST[level]


def _first_difference(a, b):
    if a is None:
        return "not finished"
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"{len(a)} bytes against {len(b)}, first difference at byte {k}"


@pytest.mark.parametrize("level", [1, 2, 4, 9])
def test_kernel_equals_host_on_every_input_in_one_batch(gpu, level):
    import compu_amd as c

    names, datas = zip(*E.inputs())
    assert max(len(d) for d in datas) == 1 << 20
    blocks, st, _ = _enc(gpu, c.FMT_LZ4_BLOCK, datas, level)
    assert (st == 2).all(), [n for n, s in zip(names, st) if s != 2]
    diff = [f"{n}: {_first_difference(b, h)}" for n, b, h in zip(names, blocks, host_blocks(level)) if b != h]
    assert not diff, "\n".join(diff)


@pytest.mark.parametrize("level", [1, 9])
def test_the_same_unit_256_times(gpu, level):
    """256 units for the persistent grid's waves, one behind the other on each: a race, or a table that was not cleared, shows as a
    copy that differs"""
    import compu_amd as c

    i = [n for n, _ in E.inputs()].index("alice64k")
    data, host = E.inputs()[i][1], host_blocks(level)[i]
    blocks, st, _ = _enc(gpu, c.FMT_LZ4_BLOCK, [data] * 256, level)
    assert (st == 2).all()
    odd = [k for k, b in enumerate(blocks) if b != host]
    assert not odd, f"copies {odd[:8]} differ from the host form: {_first_difference(blocks[odd[0]], host)}"


def test_exact_room_and_one_byte_less(gpu):
    import compu_amd as c

    names, datas = zip(*E.inputs())
    for level in (1, 9):
        host = host_blocks(level)
        jobs, caps = [], []
        for d, h in zip(datas, host):
            jobs += [d, d]
            caps += [len(h), len(h) - 1]
        blocks, st, ol = _enc(gpu, c.FMT_LZ4_BLOCK, jobs, level, caps=caps)
        for i, (n, h) in enumerate(zip(names, host)):
            assert st[2 * i] == 2 and blocks[2 * i] == h, (n, level)
            assert st[2 * i + 1] == 1 and ol[2 * i + 1] == 0, (n, level)


def test_host_memory_batch_takes_the_tags(gpu):
    """chip_encode_batch_host funnels into the same kernels: units in host memory, sliced over two streams, the host form's bytes"""
    import compu_amd as c

    level = 4
    picked = [(d, h) for (n, d), h in zip(E.inputs(), host_blocks(level)) if len(d) <= 70000][::3]
    for fmt in (c.FMT_LZ4_BLOCK, c.FMT_LZ4):
        lens = np.array([len(d) for d, _ in picked], np.uint32)
        offs = np.zeros(len(picked), np.uint64)
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        buf = np.zeros(int(lens.astype(np.uint64).sum()) + 8, np.uint8)
        buf[:int(lens.astype(np.uint64).sum())] = np.frombuffer(b"".join(d for d, _ in picked), np.uint8)
        caps = np.array([c.encode_bound(fmt, len(d)) for d, _ in picked], np.uint32)
        ooff = np.zeros(len(picked), np.uint64)
        ooff[1:] = np.cumsum((caps[:-1].astype(np.uint64) + 15) & ~np.uint64(15))
        out = np.zeros(int(ooff[-1] + caps[-1]) + 16, np.uint8)
        ol, st = c.encode_batch_host(fmt, level, buf, offs, lens, out, ooff, caps, slice_bytes=1 << 19)
        assert (st == 2).all()
        for i, (d, h) in enumerate(picked):
            got = bytes(out[int(ooff[i]):int(ooff[i]) + int(ol[i])])
            assert got == (h if fmt == c.FMT_LZ4_BLOCK else c.lz4_frame_encode_host(d, level)[0]), (fmt, i)


def _decode_frames(torch, frames, sizes):
    import compu_amd as c

    dev = torch.device("cuda:0")
    in_len = np.array([len(f) for f in frames], np.int64)
    in_off = np.zeros(len(frames), np.int64)
    in_off[1:] = np.cumsum((in_len + 3) // 4 * 4)[:-1]
    buf = np.zeros(int(in_off[-1] + in_len[-1]) // 4 * 4 + 8, np.uint8)
    for o, f in zip(in_off, frames):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    caps = np.array([max(s, 1) for s in sizes], np.int64)
    out_off = np.zeros(len(frames), np.int64)
    out_off[1:] = np.cumsum(caps)[:-1]
    d_out = torch.zeros(int(caps.sum()), dtype=torch.uint8, device=dev)
    ol, _iu, st = c.decode_batch(c.FMT_LZ4, torch.from_numpy(buf).to(dev), torch.from_numpy(in_off).to(dev), torch.from_numpy(in_len.astype(np.int32)).to(dev),
                                 d_out, torch.from_numpy(out_off).to(dev), torch.from_numpy(caps.astype(np.int32)).to(dev))
    torch.cuda.synchronize()
    out, ol, st = d_out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    return [bytes(out[out_off[i]:out_off[i] + ol[i]]) if st[i] == 2 else None for i in range(len(frames))]


def test_frames_of_every_option_equal_the_host_form_and_decode(gpu):
    import compu_amd as c

    names, datas = zip(*E.frame_inputs())
    for k, opts in enumerate(E.frame_options()):
        level = E.GROUP_LEVELS[k % 3]
        frames, st, _ = _enc(gpu, c.FMT_LZ4, datas, level, strategy=opts)
        assert (st == 2).all(), (opts, [n for n, s in zip(names, st) if s != 2])
        for n, d, f in zip(names, datas, frames):
            host, hs = c.lz4_frame_encode_host(d, level, opts)
            assert hs == 2 and f == host, f"{n}, options {opts:#x}, level {level}: {_first_difference(f, host)}"
        assert _decode_frames(gpu, frames, [len(d) for d in datas]) == list(datas), opts
    # exact room and one byte less, with every checksum
    opts, level = E.S_BCHK, 4
    full, _, _ = _enc(gpu, c.FMT_LZ4, datas, level, strategy=opts)
    jobs = [d for d in datas for _ in range(2)]
    caps = [len(f) - k for f in full for k in range(2)]
    frames, st, ol = _enc(gpu, c.FMT_LZ4, jobs, level, strategy=opts, caps=caps)
    for i, (n, f) in enumerate(zip(names, full)):
        assert st[2 * i] == 2 and frames[2 * i] == f, n
        assert st[2 * i + 1] == 1 and ol[2 * i + 1] == 0, n


def _file_want(data, unit, level, flags):
    """the ONE frame chip_encode_file writes, assembled from the host blocks (stored where not smaller)"""
    import compu_amd as c

    bid = {65536: 4, 262144: 5, 1048576: 6, 4194304: 7}[unit]
    flg = 0x40 | 0x20 | (0x10 if flags & c.W_LZ4_BLOCK_CHECKSUM else 0) | 0x08 | (0x04 if flags & c.W_LZ4_CONTENT_CHECKSUM else 0)
    desc = bytes([flg, bid << 4]) + len(data).to_bytes(8, "little")
    out = bytearray(R.MAGIC.to_bytes(4, "little") + desc + bytes([(R.xxh32(desc) >> 8) & 0xFF]))
    n_stored = 0
    for at in range(0, len(data), unit):
        piece = data[at:at + unit]
        blk, st = c.lz4_block_encode_host(piece, level)
        assert st == 2
        stored = len(blk) >= len(piece)
        n_stored += stored
        body = piece if stored else blk
        out += (len(body) | (0x80000000 if stored else 0)).to_bytes(4, "little") + body
        if flags & c.W_LZ4_BLOCK_CHECKSUM:
            out += R.xxh32(body).to_bytes(4, "little")
    out += b"\0\0\0\0"
    if flags & c.W_LZ4_CONTENT_CHECKSUM:
        out += R.xxh32(data).to_bytes(4, "little")
    return bytes(out), n_stored


def _to_device(torch, data):
    padded = np.zeros((len(data) + 3) // 4 * 4 + 4, np.uint8)
    padded[:len(data)] = np.frombuffer(data, np.uint8)
    return torch.from_numpy(padded).to(torch.device("cuda:0"))


def _file_inputs():
    big = K.text(70000, 1) + K.noise(140000, 2) + K.text(90000, 3)  # its third 64 KiB block is random: stored
    return [(b"", 0), (b"x", 0), (E.mix(65536, 1), 0), (E.mix(65537, 2), 65536), (big, 0), (E.mix(1 << 20, 3), 262144)]


@pytest.mark.parametrize("flags", [0, 2, 4, 6])
def test_encode_file_writes_the_one_frame_of_the_host_blocks(gpu, flags):
    import compu_amd as c

    stored_seen = 0
    for k, (data, unit_bytes) in enumerate(_file_inputs()):
        unit, level = unit_bytes or 65536, E.GROUP_LEVELS[k % 3]
        want, n_stored = _file_want(data, unit, level, flags)
        stored_seen += n_stored
        d_in = _to_device(gpu, data)
        out, summ = c.encode_file(c.FMT_LZ4, level, d_in, len(data), unit_bytes=unit_bytes, flags=flags)
        n_blocks = -(-len(data) // unit)
        assert summ.status == c.FileStatus.Ok and summ.out_len == len(want) and summ.n_units == n_blocks, (len(data), summ)
        got = out.cpu().numpy().tobytes()
        assert got == want, f"{len(data)} bytes, flags {flags}: {_first_difference(got, want)}"
        assert len(want) <= c.encode_file_bound(c.FMT_LZ4, len(data), unit_bytes, flags)
        assert R.frame_decode(got, len(data), checks=True) == (data, len(data), len(got), R.FINISHED)
        # the counterpart: a wave per block
        back, ps = c.lz4_parallel(_to_device(gpu, got), len(got))
        assert ps.status == 2 and back.cpu().numpy().tobytes() == data and ps.in_used == len(got)
        assert ps.path == (c.LZ4PAR_PARALLEL if n_blocks >= 2 else c.LZ4PAR_SERIAL), (len(data), ps)
        # room that is one byte short: the exact size, and nothing written
        short = gpu.full((len(want) - 1 + PAD,), 0xA5, dtype=gpu.uint8, device=d_in.device)
        none, s2 = c.encode_file(c.FMT_LZ4, level, d_in, len(data), unit_bytes=unit_bytes, flags=flags, out=short[:len(want) - 1])
        assert none is None and s2.status == c.FileStatus.NeedOutput and s2.out_len == len(want)
        assert (short == 0xA5).all()
        exact = gpu.full((len(want) + PAD,), 0xA5, dtype=gpu.uint8, device=d_in.device)
        out3, s3 = c.encode_file(c.FMT_LZ4, level, d_in, len(data), unit_bytes=unit_bytes, flags=flags, out=exact[:len(want)])
        assert s3.status == c.FileStatus.Ok and out3.cpu().numpy().tobytes() == want and (exact[len(want):] == 0xA5).all()
    assert stored_seen >= 1


def test_lz4_encode_decode_and_tar_lz4(gpu):
    import compu_amd as c

    for data in (b"", b"abc", E.alice(), E.mix(300000, 8)):
        for kw in ({}, {"level": 9, "content_checksum": True, "block_checksum": True}, {"block_bytes": 262144, "level": 4}):
            blob = c.lz4_encode(data, **kw)
            assert R.frame_decode(blob, len(data))[0] == data
            assert c.lz4_decode(blob).cpu().numpy().tobytes() == data
    items = [("docs/", b""), ("docs/alice29.txt", E.alice()), ("noise.bin", K.noise(100000, 5)), ("empty", b"")]
    image, _entries, summ = c.tar_write_items(items)
    assert summ.status == c.TarWriteStatus.Ok
    out, fs = c.encode_file(c.FMT_LZ4, 1, image, image.numel())
    assert fs.status == c.FileStatus.Ok and fs.n_units == -(-image.numel() // 65536)
    tar = c.tar_open(_to_device(gpu, out.cpu().numpy().tobytes()), fs.out_len)
    assert tar.names == [n.encode() for n, _ in items]
    for name, content in items:
        assert tar.member(name).cpu().numpy().tobytes() == content
