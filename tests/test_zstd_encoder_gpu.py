"""The zstd encoder on the GPU (encoder::Interface::zstd, src/encoder/zstd.rs): the reference's encoder tests
(tests/encoder.rs:195-203 should_encode_and_decode_zstd, :324-332 should_encode_with_empty_final_and_decode_zstd), batch round
trips through three decoders, the modes the frames use, room, byte identity of the paths, streaming, the status rules, options
and the compression ratio."""
import ctypes as C
import random

import numpy as np
import pytest

from conftest import golden
from test_encoder_gpu import _test_case, _test_case_empty_final
from test_inflate_gpu import _mk
from zstd_decoders import oracle_decode as _oracle_decode, zdec as _zdec

pytestmark = pytest.mark.gpu
FMT_ZSTD = 100


def _batch(torch, datas, level=3, strategy=0, caps=None, pad=64, with_len=False):
    """chip_encode_batch_ex(CHIP_FMT_ZSTD) with a 0xA5 canary behind every unit's range -> (frames, status), with_len: and out_len"""
    import compu_amd as c

    n = len(datas)
    in_len = np.array([len(d) for d in datas], np.int64)
    in_off = np.zeros(n, np.int64)
    in_off[1:] = np.cumsum((in_len + 3) // 4 * 4)[:-1]
    buf = np.zeros(max(int(in_off[-1] + in_len[-1]) + 4, 4) // 4 * 4 + 4, np.uint8)
    for i, d in enumerate(datas):
        buf[in_off[i] : in_off[i] + len(d)] = np.frombuffer(d, np.uint8)
    caps = np.array([c.encode_bound(FMT_ZSTD, len(d)) for d in datas] if caps is None else caps, np.int64)
    out_off = np.zeros(n, np.int64)
    out_off[1:] = np.cumsum(caps + pad)[:-1]
    total = int(out_off[-1] + caps[-1] + pad)
    dev = torch.device("cuda:0")
    d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    out_len, status = c.encode_batch(
        FMT_ZSTD, level, torch.from_numpy(buf).to(dev), torch.from_numpy(in_off).to(dev), torch.from_numpy(in_len.astype(np.int32)).to(dev),
        d_out, torch.from_numpy(out_off).to(dev), torch.from_numpy(caps.astype(np.int32)).to(dev), strategy=strategy)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    ol, st = out_len.cpu().numpy(), status.cpu().numpy()
    frames = []
    for i in range(n):
        tail = out[out_off[i] + caps[i] : out_off[i] + caps[i] + pad]
        assert (tail == 0xA5).all(), f"unit {i} wrote past its out_cap"
        frames.append(bytes(out[out_off[i] : out_off[i] + ol[i]]) if st[i] == 2 else None)
    return (frames, st, ol) if with_len else (frames, st)


def _gpu_decode(torch, frames, sizes):
    import compu_amd as c

    n = len(frames)
    in_len = np.array([len(f) for f in frames], np.int64)
    in_off = np.zeros(n, np.int64)
    in_off[1:] = np.cumsum((in_len + 3) // 4 * 4)[:-1]
    buf = np.zeros(int(in_off[-1] + in_len[-1]) // 4 * 4 + 8, np.uint8)
    for i, f in enumerate(frames):
        buf[in_off[i] : in_off[i] + len(f)] = np.frombuffer(f, np.uint8)
    caps = np.array([max(s, 1) for s in sizes], np.int64)
    out_off = np.zeros(n, np.int64)
    out_off[1:] = np.cumsum(caps)[:-1]
    dev = torch.device("cuda:0")
    d_out = torch.zeros(int(caps.sum()), dtype=torch.uint8, device=dev)
    ol, _iu, st = c.decode_batch(FMT_ZSTD, torch.from_numpy(buf).to(dev), torch.from_numpy(in_off).to(dev),
                                 torch.from_numpy(in_len.astype(np.int32)).to(dev), d_out, torch.from_numpy(out_off).to(dev),
                                 torch.from_numpy(caps.astype(np.int32)).to(dev))
    torch.cuda.synchronize()
    out, ol, st = d_out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    return [bytes(out[out_off[i] : out_off[i] + ol[i]]) if st[i] == 2 else None for i in range(n)]


# ---- a small frame parser: which modes a frame uses (RFC 8878) -------------------------------------------------------------------


def _parse(frame):
    """-> set of mode tags of a frame written by this encoder (checks the structure as it goes)"""
    tags = set()
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    single, has_ck, fcs_flag = (fhd >> 5) & 1, (fhd >> 2) & 1, fhd >> 6
    assert fhd & 3 == 0 and (fhd >> 3) & 1 == 0
    if has_ck:
        tags.add("checksum")
    p = 5 + (0 if single else 1)
    p += [1 if single else 0, 2, 4, 8][fcs_flag]
    while True:
        h = int.from_bytes(frame[p : p + 3], "little")
        last, btype, bsize = h & 1, (h >> 1) & 3, h >> 3
        p += 3
        tags.add(["raw_block", "rle_block", "compressed_block", "reserved"][btype])
        if btype == 0:
            p += bsize
        elif btype == 1:
            p += 1
        else:
            b = frame[p : p + bsize]
            p += bsize
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            if lt in (0, 1):
                tags.add("lit_raw" if lt == 0 else "lit_rle")
                hs = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                size = b[0] >> 3 if sf in (0, 2) else (b[0] >> 4) + (b[1] << 4) + ((b[2] << 12) if sf == 3 else 0)
                q = hs + (size if lt == 0 else 1)
            else:
                assert lt == 2, "treeless literals are not written"
                hs, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
                v = int.from_bytes(b[:hs], "little") >> 4
                csize = v >> bits
                tags.add("lit_1stream" if sf == 0 else "lit_4streams")
                tags.add("weights_direct" if b[hs] >= 128 else "weights_fse")
                q = hs + csize
            nseq = b[q]
            q += 1 if nseq < 128 else 2 if nseq < 255 else 3
            if nseq:
                modes = b[q]
                assert modes & 3 == 0
                for name, sh in (("LL", 6), ("OF", 4), ("ML", 2)):
                    m = (modes >> sh) & 3
                    assert m != 3, "Repeat_Mode is not written"
                    tags.add(f"{name}_{['predefined', 'rle', 'fse'][m]}")
        if last:
            break
    assert len(frame) == p + 4 * has_ck
    return tags


# ---- 1. the reference's tests -------------------------------------------------------------------------------------------------


def test_should_encode_and_decode_zstd_hip(gpu):
    import compu_amd as c

    for level in (3, 1, 19):
        encoder = c.encoder_interface.zstd_hip(c.ZstdEncoderOptions().level(level))
        decoder = c.decoder_interface.zstd_hip()
        assert encoder is not None and decoder is not None
        for name in ("10x10y", "alice29.txt"):
            data = golden(name)
            comp = _test_case(c, encoder, decoder, data, c.Detection.Zstd)
            assert _zdec(comp, len(data)) == data
            _test_case_empty_final(c, encoder, decoder, data)


def test_empty_final_flush_fits_the_reference_room(gpu):
    """tests/encoder.rs:124-138 with the 20-byte fixture: Process, then Flush into 20 bytes of room is Continue."""
    import compu_amd as c

    data = golden("10x10y")
    enc = c.encoder_interface.zstd_hip()
    out = bytearray(len(data))
    r = enc.encode(data, out, c.EncodeOp.Process, 0, len(out))
    assert r.status == c.EncodeStatus.Continue and r.output_remain == len(out) and r.input_remain == 0
    r = enc.encode(b"", out, c.EncodeOp.Flush, 0, len(out))
    assert r.status == c.EncodeStatus.Continue
    flushed = bytes(out[: len(out) - r.output_remain])
    assert flushed[4] == 0x04 and len(flushed) <= 20  # checksum flag, a Window_Descriptor, no content size
    assert _zdec(flushed, 100, complete=False) == data


# ---- 2. batch round trip ---------------------------------------------------------------------------------------------------------

SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 1023, 1024, 5000, 65535, 65536, 131071, 131072, 131073, 200000, 400000]


def test_batch_round_trip_three_decoders(gpu, alice):
    rnd = random.Random(5)
    settings = [(-5, 0), (1, 0), (3, 0), (6, 0), (9, 0), (19, 0), (22, 0), (3, 1), (3, 4), (1, 6), (5, 9)]
    for level, strategy in settings:
        datas = [_mk(rnd.randrange(5), rnd.choice(SIZES), rnd, alice) for _ in range(60)]
        if level == 3 and strategy == 0:
            datas.append((alice * 20)[: 3 << 20])  # a few MiB: 24 blocks of 128 KiB
        frames, st = _batch(gpu, datas, level, strategy)
        assert (st == 2).all(), (level, strategy, st)
        sizes = [len(d) for d in datas]
        for f, d in zip(frames, datas):
            assert _zdec(f, len(d)) == d
        assert _oracle_decode(frames, sizes) == datas
        assert _gpu_decode(gpu, frames, sizes) == datas


# ---- 3. modes --------------------------------------------------------------------------------------------------------------------


def test_every_mode_is_reached(gpu, alice):
    rnd = random.Random(7)
    corpus = [alice[:100000], alice[:900], b"a" * 5000, bytes(rnd.randrange(256) for _ in range(5000)), b"xyz" * 3000]
    corpus.append(bytes(rnd.choice(b"ab") for _ in range(3000)))
    corpus.append(bytes((rnd.randrange(4) + 200) for _ in range(4000)))  # literals >= 128: FSE-compressed weights
    corpus.append(bytes(min(255, int(rnd.expovariate(0.02))) for _ in range(60000)))
    corpus.append(bytes(rnd.randrange(2) * 255 for _ in range(2000)) + alice[:2000])
    # runs of 256 different bytes: every sequence has literal length 1 and the initial repeat offset 1 (LL and OF in RLE mode)
    corpus.append(b"".join(bytes([b]) * rnd.randrange(6, 40) for b in range(256)))
    # 8 bytes >= 128, then the same 16-byte token: literal length 8 and match length 16 everywhere (LL and ML in RLE mode)
    corpus.append(b"".join(bytes(rnd.randrange(128, 256) for _ in range(8)) + b"ABCDEFGHIJKLMNOP" for _ in range(2000)))
    # a first block of zeros ending in 200 bytes, then copies of those 200 bytes with one separator byte: RLE literals in the second
    s = bytes(rnd.randrange(8, 256) for _ in range(200))
    corpus.append(b"\0" * (131072 - len(s)) + s + (s + b"\x07") * 300 + b"\x07" * 9)
    corpus.append(bytes(range(256)) * 40)
    frames, st = _batch(gpu, corpus, 3)
    assert (st == 2).all()
    seen = set()
    for f, d in zip(frames, corpus):
        tags = _parse(f)
        assert "checksum" in tags
        assert _zdec(f, len(d)) == d
        seen |= tags
    want = {"raw_block", "rle_block", "compressed_block", "lit_raw", "lit_rle", "lit_1stream", "lit_4streams", "weights_direct", "weights_fse"}
    want |= {f"{k}_{m}" for k in ("LL", "OF", "ML") for m in ("predefined", "rle", "fse")}
    assert want <= seen, sorted(want - seen)


# ---- 4. room ---------------------------------------------------------------------------------------------------------------------


def test_too_little_room_is_need_output(gpu, alice):
    import compu_amd as c

    datas = [alice[:50000], alice[:1000], bytes(range(256)) * 4, b"", b"q" * 300]
    full, st = _batch(gpu, datas, 3)
    assert (st == 2).all()
    caps = [len(f) - 1 for f in full] + [len(full[0]) // 2, 0, 5]
    datas2 = datas + [alice[:50000], alice[:10], alice[:10]]
    frames, st = _batch(gpu, datas2, 3, caps=caps)
    assert (st == 1).all(), st
    assert c.encode_bound(FMT_ZSTD, 0) >= len(full[3])


# ---- 5. the same bytes from every path -------------------------------------------------------------------------------------------


def _stream_oneshot(c, data, level, strategy):
    enc = c.encoder_interface.zstd_hip(c.ZstdEncoderOptions().level(level).strategy(strategy))
    out = bytearray(c.encode_bound(FMT_ZSTD, len(data)))
    r = enc.encode(data, out, c.EncodeOp.Finish, 0, len(out))
    assert r.status == c.EncodeStatus.Finished and r.input_remain == 0
    enc.close()
    return bytes(out[: len(out) - r.output_remain])


def test_device_host_and_streaming_bytes_are_identical(gpu, alice):
    import compu_amd as c

    rnd = random.Random(9)
    for level, strategy in ((3, 0), (1, 0), (9, 0), (19, 6), (-3, 0)):
        datas = [_mk(rnd.randrange(5), rnd.choice([0, 1, 100, 5000, 65536, 200000, 1 << 20]), rnd, alice) for _ in range(8)]
        frames, st = _batch(gpu, datas, level, strategy)
        assert (st == 2).all()
        if strategy == 0:
            in_len = np.array([len(d) for d in datas], np.uint32)
            in_off = np.zeros(len(datas), np.uint64)
            in_off[1:] = np.cumsum(in_len.astype(np.uint64))[:-1]
            caps = np.array([c.encode_bound(FMT_ZSTD, len(d)) for d in datas], np.uint32)
            out_off = np.zeros(len(datas), np.uint64)
            out_off[1:] = np.cumsum(caps.astype(np.uint64))[:-1]
            hbuf = np.frombuffer(b"".join(datas) + b"\0" * 4, np.uint8).copy()
            hout = np.zeros(int(caps.sum()) + 1, np.uint8)
            ol, hst = c.encode_batch_host(FMT_ZSTD, level, hbuf, in_off, in_len, hout, out_off, caps)
            assert (hst == 2).all()
            for i, f in enumerate(frames):
                assert bytes(hout[out_off[i] : out_off[i] + ol[i]]) == f
        for d, f in zip(datas, frames):
            assert _stream_oneshot(c, d, level, strategy) == f


# ---- 6. streaming ----------------------------------------------------------------------------------------------------------------


def _stream_run(c, enc, data, rnd, flushes=True):
    out_all = bytearray()
    pos = 0
    while pos < len(data):
        k = rnd.choice([1, 100, 4096, 70000, 300000, 1 << 20])
        piece = data[pos : pos + k]
        op = c.EncodeOp.Flush if flushes and rnd.random() < 0.3 else c.EncodeOp.Process
        while True:
            room = rnd.choice([0, 1, 7, 1000, 65536, 1 << 20])
            buf = bytearray(room)
            r = enc.encode(piece, buf, op, 0, room)
            assert r.status != c.EncodeStatus.Error
            out_all += buf[: room - r.output_remain]
            piece = piece[len(piece) - r.input_remain :]
            if not piece and (op == c.EncodeOp.Process or r.status == c.EncodeStatus.Continue and r.output_remain > 0):
                break
        pos += k
        if op == c.EncodeOp.Flush:
            # everything so far is out and decodes
            assert _zdec(bytes(out_all), pos + 16, complete=False) == data[:pos]
    while True:
        room = rnd.choice([1, 13, 5000, 1 << 20])
        buf = bytearray(room)
        r = enc.encode(b"", buf, c.EncodeOp.Finish, 0, room)
        out_all += buf[: room - r.output_remain]
        if r.status == c.EncodeStatus.Finished:
            break
        assert r.status == c.EncodeStatus.NeedOutput
    return bytes(out_all)


def test_streaming_pieces_flushes_and_reset(gpu, alice):
    import compu_amd as c

    rnd = random.Random(13)
    body = bytearray()
    while len(body) < (3 << 20) + 12345:
        body += alice[rnd.randrange(0, 100000) :][: rnd.randrange(100, 20000)]
        body += bytes(rnd.randrange(256) for _ in range(rnd.randrange(0, 50)))
    data = bytes(body)
    enc = c.encoder_interface.zstd_hip()
    comp = _stream_run(c, enc, data, random.Random(1))
    assert _zdec(comp, len(data)) == data
    dec = c.decoder_interface.zstd_hip()
    out = c.Vec()
    r = dec.decode_vec_full(comp, out)
    assert r.status == c.DecodeStatus.Finished and bytes(out) == data
    # reset and reuse gives the bytes of a fresh encoder
    enc.reset()
    again = _stream_run(c, enc, data, random.Random(1))
    fresh = _stream_run(c, c.encoder_interface.zstd_hip(), data, random.Random(1))
    assert again == fresh
    assert _zdec(fresh, len(data)) == data


# ---- 7. status rules -------------------------------------------------------------------------------------------------------------


def test_status_rules_of_zstd_rs(gpu, alice):
    import compu_amd as c

    S = c.EncodeStatus
    enc = c.encoder_interface.zstd_hip()
    # Process that only buffers: nothing waits for delivery -> Continue, also with no room at all
    r = enc.encode(alice[:1000], bytearray(0), c.EncodeOp.Process, 0, 0)
    assert r.status == S.Continue and r.input_remain == 0
    # Flush without room: compressed bytes wait -> NeedOutput; Process with no room while they wait -> NeedOutput
    r = enc.encode(b"", bytearray(0), c.EncodeOp.Flush, 0, 0)
    assert r.status == S.NeedOutput
    r = enc.encode(b"", bytearray(0), c.EncodeOp.Process, 0, 0)
    assert r.status == S.NeedOutput
    # deliver them with room to spare: everything out and nothing buffered -> Continue
    buf = bytearray(5000)
    r = enc.encode(b"", buf, c.EncodeOp.Flush, 0, len(buf))
    assert r.status == S.Continue and r.output_remain > 0
    # a Finish that fills the output exactly before the frame is complete -> NeedOutput, then Finished
    r = enc.encode(alice[1000:3000], bytearray(3), c.EncodeOp.Finish, 0, 3)
    assert r.status == S.NeedOutput and r.output_remain == 0
    r = enc.encode(b"", buf, c.EncodeOp.Finish, 0, len(buf))
    assert r.status == S.Finished
    # the whole frame filling the output exactly: compu sees 0 first -> Finished
    enc.reset()
    whole = _stream_oneshot(c, alice[:5000], 3, 0)
    out = bytearray(len(whole))
    r = enc.encode(alice[:5000], out, c.EncodeOp.Finish, 0, len(out))
    assert r.status == S.Finished and r.output_remain == 0 and bytes(out) == whole


# ---- 8. options ------------------------------------------------------------------------------------------------------------------


def test_options_range_and_small_window(gpu, alice):
    import compu_amd as c
    from compu_amd.api import _ZstdEncoderOpts

    L = c.lib()
    for lvl, strat, wl in ((131073, 0, 27), (-131073, 0, 27), (3, 10, 27), (3, -1, 27), (3, 0, 9), (3, 0, 32)):
        assert not L.chip_encoder_new_zstd(C.byref(_ZstdEncoderOpts(lvl, strat, wl, -1))), (lvl, strat, wl)
    with pytest.raises(AssertionError):
        c.ZstdEncoderOptions().window_log(9)
    with pytest.raises(AssertionError):
        c.ZstdEncoderOptions().level(131073)
    bad = c.ZstdEncoderOptions()
    bad._strategy = 10
    assert c.encoder_interface.zstd_hip(bad) is None
    for lvl in (131072, -131072, 0, 23):
        e = c.encoder_interface.zstd_hip(c.ZstdEncoderOptions().level(lvl))
        assert e is not None
        assert _zdec(_test_case(c, e, c.decoder_interface.zstd_hip(), alice[:20000], c.Detection.Zstd), 20000) == alice[:20000]
    data = alice + alice[:50000]
    enc = c.encoder_interface.zstd_hip(c.ZstdEncoderOptions().window_log(10))
    for rnd_seed in (1, 2):
        comp = _stream_run(c, enc, data, random.Random(rnd_seed), flushes=rnd_seed == 2)
        enc.reset()
        assert _zdec(comp, len(data), window_log_max=10) == data
        dec = c.decoder_interface.zstd_hip(c.ZstdOptions().window_log(10))
        out = c.Vec()
        r = dec.decode_vec_full(comp, out)
        assert r.status == c.DecodeStatus.Finished and bytes(out) == data
    # one-shot under window_log(10): larger than the window, so not single-segment
    small = c.encoder_interface.zstd_hip(c.ZstdEncoderOptions().window_log(10))
    out = bytearray(c.encode_bound(FMT_ZSTD, 5000) + 3 * 5)
    r = small.encode(alice[:5000], out, c.EncodeOp.Finish, 0, len(out))
    assert r.status == c.EncodeStatus.Finished
    assert _zdec(bytes(out[: len(out) - r.output_remain]), 5000, window_log_max=10) == alice[:5000]


# ---- 9. ratio --------------------------------------------------------------------------------------------------------------------


def test_ratio_against_libzstd_level1(gpu, alice):
    import compu_amd as c
    from bench_support import synth

    for data, bar in ((alice, 65687), (synth.payloads(4, threads=4).tobytes(), 148387)):
        comp = _stream_run(c, c.encoder_interface.zstd_hip(), data, random.Random(3), flushes=False)
        assert _zdec(comp, len(data)) == data
        assert len(comp) <= bar, (len(comp), bar)
