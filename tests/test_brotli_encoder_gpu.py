"""The brotli encoder on the GPU (encoder::Interface::brotli_c, src/encoder/brotli_c.rs): the reference's encoder tests
(tests/encoder.rs should_encode_and_decode_brotli_c, should_encode_with_empty_final_and_decode_brotli_c), batch round trips through
libbrotlidec and the GPU decoder, kernel bytes against the host form of the same core, room, byte identity of the paths, streaming
with flushes and reset, the status rules, a 65 536-unit batch and the compression ratio."""
import random

import numpy as np
import pytest

import brotli_enc_host as H
import brotli_ref as B
from conftest import golden
from test_encoder_gpu import _test_case, _test_case_empty_final
from test_inflate_gpu import _mk

pytestmark = pytest.mark.gpu
FMT_BROTLI = 101
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 1023, 1024, 5000, 65535, 65536, 131071, 131072, 131073, 200000, 400000]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return H.build_driver(str(tmp_path_factory.mktemp("benc")))


def _batch(torch, datas, quality=0, mode=0, caps=None, pad=64):
    """chip_encode_batch_ex(CHIP_FMT_BROTLI) with a 0xA5 canary behind every unit's range -> (streams, status)"""
    import compu_amd as c

    n = len(datas)
    in_len = np.array([len(d) for d in datas], np.int64)
    in_off = np.zeros(n, np.int64)
    in_off[1:] = np.cumsum((in_len + 3) // 4 * 4)[:-1]
    buf = np.zeros(max(int(in_off[-1] + in_len[-1]) + 4, 4) // 4 * 4 + 4, np.uint8)
    for i, d in enumerate(datas):
        buf[in_off[i] : in_off[i] + len(d)] = np.frombuffer(d, np.uint8)
    caps = np.array([c.encode_bound(FMT_BROTLI, len(d)) for d in datas] if caps is None else caps, np.int64)
    out_off = np.zeros(n, np.int64)
    out_off[1:] = np.cumsum(caps + pad)[:-1]
    total = int(out_off[-1] + caps[-1] + pad)
    dev = torch.device("cuda:0")
    d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    out_len, status = c.encode_batch(
        FMT_BROTLI, quality, torch.from_numpy(buf).to(dev), torch.from_numpy(in_off).to(dev),
        torch.from_numpy(in_len.astype(np.int32)).to(dev), d_out, torch.from_numpy(out_off).to(dev),
        torch.from_numpy(caps.astype(np.int32)).to(dev), strategy=mode)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    ol, st = out_len.cpu().numpy(), status.cpu().numpy()
    streams = []
    for i in range(n):
        tail = out[out_off[i] + caps[i] : out_off[i] + caps[i] + pad]
        assert (tail == 0xA5).all(), f"unit {i} wrote past its out_cap"
        streams.append(bytes(out[out_off[i] : out_off[i] + ol[i]]) if st[i] == 2 else None)
    return streams, st


def _gpu_decode(torch, streams, sizes):
    import compu_amd as c

    n = len(streams)
    in_len = np.array([len(f) for f in streams], np.int64)
    in_off = np.zeros(n, np.int64)
    in_off[1:] = np.cumsum((in_len + 3) // 4 * 4)[:-1]
    buf = np.zeros(int(in_off[-1] + in_len[-1]) // 4 * 4 + 8, np.uint8)
    for i, f in enumerate(streams):
        buf[in_off[i] : in_off[i] + len(f)] = np.frombuffer(f, np.uint8)
    caps = np.array([max(s, 1) for s in sizes], np.int64)
    out_off = np.zeros(n, np.int64)
    out_off[1:] = np.cumsum(caps)[:-1]
    dev = torch.device("cuda:0")
    d_out = torch.zeros(int(caps.sum()), dtype=torch.uint8, device=dev)
    ol, _iu, st = c.decode_batch(FMT_BROTLI, torch.from_numpy(buf).to(dev), torch.from_numpy(in_off).to(dev),
                                 torch.from_numpy(in_len.astype(np.int32)).to(dev), d_out, torch.from_numpy(out_off).to(dev),
                                 torch.from_numpy(caps.astype(np.int32)).to(dev))
    torch.cuda.synchronize()
    out, ol, st = d_out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    return [bytes(out[out_off[i] : out_off[i] + ol[i]]) if st[i] == 2 else None for i in range(n)]


def _libdec(stream, data):
    st, out, used = B.decode(stream, len(data) + 16)
    assert st == B.FINISHED and used == len(stream)
    return out


# ---- 1. the reference's tests -------------------------------------------------------------------------------------------------


def test_should_encode_and_decode_brotli_hip(gpu):
    import compu_amd as c

    for opts in (c.BrotliOptions(), c.BrotliOptions().quality(1), c.BrotliOptions().quality(5)):
        encoder = c.encoder_interface.brotli_hip(opts)
        decoder = c.decoder_interface.brotli_hip()
        assert encoder is not None and decoder is not None
        for name in ("10x10y", "alice29.txt"):
            data = golden(name)
            comp = _test_case(c, encoder, decoder, data, c.Detection.Unknown)
            assert _libdec(comp, data) == data
            _test_case_empty_final(c, encoder, decoder, data)
        encoder.close()


def test_empty_final_flush_fits_the_reference_room(gpu):
    """tests/encoder.rs:124-138 with the 20-byte fixture: Process, then Flush into 20 bytes of room is Continue."""
    import compu_amd as c

    data = golden("10x10y")
    enc = c.encoder_interface.brotli_hip()
    out = bytearray(len(data))
    r = enc.encode(data, out, c.EncodeOp.Process, 0, len(out))
    assert r.status == c.EncodeStatus.Continue and r.output_remain == len(out) and r.input_remain == 0
    r = enc.encode(b"", out, c.EncodeOp.Flush, 0, len(out))
    assert r.status == c.EncodeStatus.Continue
    flushed = bytes(out[: len(out) - r.output_remain])
    st, got, used = B.decode(flushed, 100)
    assert st == B.NEED_INPUT and got == data and used == len(flushed)


# ---- 2. batch round trips, kernel bytes == host-core bytes -------------------------------------------------------------------------


def test_batch_round_trip_and_host_core_bytes(gpu, alice, driver):
    rnd = random.Random(5)
    for quality in (1, 3, 5, 11):
        datas = [_mk(k % 5, n, rnd, alice) for k, n in enumerate(SIZES)]
        datas += [_mk(rnd.randrange(5), rnd.randrange(0, 300000), rnd, alice) for _ in range(12)]
        streams, st = _batch(gpu, datas, quality)
        assert (st == 2).all(), st
        host = H.encode(driver, quality, 22, datas)
        for i, (d, s) in enumerate(zip(datas, streams)):
            assert s == host[i], f"quality {quality} unit {i}: kernel and host core differ"
            assert _libdec(s, d) == d
        assert _gpu_decode(gpu, streams, [len(d) for d in datas]) == datas


def test_too_little_room_is_need_output(gpu, alice):
    import compu_amd as c

    datas = [alice[:50000], alice[:1000], bytes(range(256)) * 4, b"", b"q" * 300]
    full, st = _batch(gpu, datas, 5)
    assert (st == 2).all()
    caps = [len(f) - 1 for f in full] + [len(full[0]) // 2, 0, 5]
    datas2 = datas + [alice[:50000], alice[:10], alice[:10]]
    _, st = _batch(gpu, datas2, 5, caps=caps)
    assert (st == 1).all(), st
    # incompressible units at out_cap = bound
    rnd = random.Random(2)
    inc = [rnd.randbytes(n) for n in (0, 1, 100, 65536, 131072, 131073, 400000)]
    streams, st = _batch(gpu, inc, 11, caps=[c.encode_bound(FMT_BROTLI, len(d)) for d in inc])
    assert (st == 2).all(), st
    for d, s in zip(inc, streams):
        assert _libdec(s, d) == d


# ---- 3. the same bytes from every path -------------------------------------------------------------------------------------------


def _stream_oneshot(c, data, quality, mode=0):
    opts = c.BrotliOptions()
    if quality:
        opts = opts.quality(quality)
    enc = c.encoder_interface.brotli_hip(opts.mode(mode) if mode else opts)
    out = bytearray(c.encode_bound(FMT_BROTLI, len(data)))
    r = enc.encode(data, out, c.EncodeOp.Finish, 0, len(out))
    assert r.status == c.EncodeStatus.Finished and r.input_remain == 0
    enc.close()
    return bytes(out[: len(out) - r.output_remain])


def test_device_host_and_streaming_bytes_are_identical(gpu, alice):
    import compu_amd as c

    rnd = random.Random(9)
    for quality, mode in ((0, 0), (1, 1), (5, 2), (9, 3), (11, 0)):
        datas = [_mk(rnd.randrange(5), rnd.choice([0, 1, 100, 5000, 65536, 200000, 1 << 20]), rnd, alice) for _ in range(8)]
        streams, st = _batch(gpu, datas, quality, mode)
        assert (st == 2).all()
        in_len = np.array([len(d) for d in datas], np.uint32)
        in_off = np.zeros(len(datas), np.uint64)
        in_off[1:] = np.cumsum(in_len.astype(np.uint64))[:-1]
        caps = np.array([c.encode_bound(FMT_BROTLI, len(d)) for d in datas], np.uint32)
        out_off = np.zeros(len(datas), np.uint64)
        out_off[1:] = np.cumsum(caps.astype(np.uint64))[:-1]
        hbuf = np.frombuffer(b"".join(datas) + b"\0" * 4, np.uint8).copy()
        hout = np.zeros(int(caps.sum()) + 1, np.uint8)
        ol, hst = c.encode_batch_host(FMT_BROTLI, quality, hbuf, in_off, in_len, hout, out_off, caps)
        assert (hst == 2).all()
        for i, s in enumerate(streams):
            assert bytes(hout[out_off[i] : out_off[i] + ol[i]]) == s
        for d, s in zip(datas, streams):
            assert _stream_oneshot(c, d, quality, mode) == s


# ---- 4. streaming ----------------------------------------------------------------------------------------------------------------


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
            got = room - r.output_remain
            out_all += buf[:got]
            # brotli_c.rs:63-84: NeedOutput exactly while compressed bytes wait
            if r.status == c.EncodeStatus.NeedOutput:
                assert r.output_remain == 0
            piece = piece[len(piece) - r.input_remain :]
            if not piece and (op == c.EncodeOp.Process or r.status == c.EncodeStatus.Continue):
                break
        pos += k
        if op == c.EncodeOp.Flush:
            # everything so far is out, and libbrotlidec in streaming mode returns exactly the input so far
            st, got, used = B.decode(bytes(out_all), pos + 16)
            assert st == B.NEED_INPUT and used == len(out_all) and got == data[:pos]
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
    enc = c.encoder_interface.brotli_hip(c.BrotliOptions().quality(5))
    comp = _stream_run(c, enc, data, random.Random(1))
    assert _libdec(comp, data) == data
    dec = c.decoder_interface.brotli_hip()
    out = c.Vec()
    r = dec.decode_vec_full(comp, out)
    assert r.status == c.DecodeStatus.Finished and bytes(out) == data
    # reset and reuse gives the bytes of a fresh encoder
    enc.reset()
    again = _stream_run(c, enc, data, random.Random(1))
    fresh = _stream_run(c, c.encoder_interface.brotli_hip(c.BrotliOptions().quality(5)), data, random.Random(1))
    assert again == fresh
    assert _libdec(fresh, data) == data


def test_status_rules_of_brotli_c_rs(gpu, alice):
    import compu_amd as c

    S = c.EncodeStatus
    enc = c.encoder_interface.brotli_hip()
    # Process that only buffers: nothing waits -> Continue, also with no room at all
    r = enc.encode(alice[:1000], bytearray(0), c.EncodeOp.Process, 0, 0)
    assert r.status == S.Continue and r.input_remain == 0
    # Flush without room: compressed bytes wait -> NeedOutput; so does Process while they wait
    r = enc.encode(b"", bytearray(0), c.EncodeOp.Flush, 0, 0)
    assert r.status == S.NeedOutput
    r = enc.encode(b"", bytearray(0), c.EncodeOp.Process, 0, 0)
    assert r.status == S.NeedOutput
    buf = bytearray(5000)
    r = enc.encode(b"", buf, c.EncodeOp.Flush, 0, len(buf))
    assert r.status == S.Continue and r.output_remain > 0
    # a Finish whose output does not fit -> NeedOutput, then Finished
    r = enc.encode(alice[1000:3000], bytearray(3), c.EncodeOp.Finish, 0, 3)
    assert r.status == S.NeedOutput and r.output_remain == 0
    r = enc.encode(b"", buf, c.EncodeOp.Finish, 0, len(buf))
    assert r.status == S.Finished
    # the whole stream filling the output exactly: nothing waits -> Finished
    enc.reset()
    whole = _stream_oneshot(c, alice[:5000], 0)
    out = bytearray(len(whole))
    r = enc.encode(alice[:5000], out, c.EncodeOp.Finish, 0, len(out))
    assert r.status == S.Finished and r.output_remain == 0 and bytes(out) == whole
    enc.close()


def test_options_range(gpu, alice):
    import compu_amd as c
    from compu_amd.api import _BrotliEncoderOpts
    import ctypes as C

    L = c.lib()
    for q, m, w in ((12, 0, 22), (5, 4, 22), (5, 0, 9), (5, 0, 25), (-1, 0, 22)):
        assert not L.chip_encoder_new_brotli(C.byref(_BrotliEncoderOpts(q, m, w, -1))), (q, m, w)
    h = L.chip_encoder_new_brotli(None)  # BrotliOptions::new()
    assert h
    L.chip_encoder_free(h)
    for lgwin in (10, 16, 24):
        enc = c.encoder_interface.brotli_hip(c.BrotliOptions().quality(5), lgwin=lgwin)
        out = bytearray(len(alice) + 100)
        r = enc.encode(alice, out, c.EncodeOp.Finish, 0, len(out))
        assert r.status == c.EncodeStatus.Finished
        comp = bytes(out[: len(out) - r.output_remain])
        assert H.first_metablock(comp)["wbits"] == lgwin
        assert _libdec(comp, alice) == alice
        enc.close()


# ---- 5. scale and ratio ----------------------------------------------------------------------------------------------------------


def test_batch_of_65536_units(gpu, driver):
    from bench_support import synth

    pay = synth.payloads(32).tobytes()
    rnd = np.random.default_rng(1)
    n = 65536
    sizes = rnd.integers(0, 4096, n)
    starts = rnd.integers(0, len(pay) - 4096, n)
    datas = [pay[s : s + k] for s, k in zip(starts, sizes)]
    streams, st = _batch(gpu, datas, 5)
    assert (st == 2).all()
    assert _gpu_decode(gpu, streams, [len(d) for d in datas]) == datas
    pick = list(range(0, n, 1024))
    for i in pick:
        assert _libdec(streams[i], datas[i]) == datas[i]
    host = H.encode(driver, 5, 22, [datas[i] for i in pick])
    assert host == [streams[i] for i in pick]


def test_ratio_against_libbrotlienc_quality1(gpu, alice):
    from bench_support import synth

    syn = synth.payloads(4).tobytes()
    for data in (alice, syn):
        ref = len(B.compress(data, quality=1))
        for quality in (5, 9, 11):
            s, = _batch(gpu, [data], quality)[0]
            assert len(s) <= 1.10 * ref, (quality, len(s), ref)
