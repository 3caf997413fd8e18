"""Brotli decode on the GPU (CHIP_FMT_BROTLI): the reference's decoder test (tests/decoder.rs:97-116, should_decode_brotli_c)
against the hip variant, and parity with the system's libbrotlidec (tests/brotli_ref.py) in batches and streams."""
import random

import numpy as np
import pytest

import brotli_ref as B
from conftest import golden
from test_decoder_gpu import DATA, _test_case
from test_inflate_gpu import _mk, run_batch

pytestmark = pytest.mark.gpu
FMT_BROTLI = 101


def _check_parity(got, ref, data_note=""):
    """one unit: (out, status, in_used) of the GPU against libbrotlidec's (status, out, in_used)"""
    out, st, used = got
    rst, rout, rused = ref
    assert st == rst, f"{data_note}: status {st} against libbrotlidec {rst}"
    if st == B.FINISHED:
        assert out == rout and used == rused, data_note
    elif st == B.NEED_OUTPUT:
        assert out[: len(rout)] == rout, data_note
    else:  # an error or truncation: what libbrotlidec flushed is a prefix of what the GPU decoded
        assert out[: len(rout)] == rout, data_note


def _batch(torch, parts, caps):
    outs, ol, iu, st = run_batch(torch, FMT_BROTLI, parts, caps)
    return [(outs[i], int(st[i]), int(iu[i])) for i in range(len(parts))]


def test_should_decode_brotli_hip(gpu):
    """tests/decoder.rs:97-105 with Interface::brotli_c replaced by the hip variant"""
    import compu_amd

    decoder = compu_amd.decoder_interface.brotli_hip()
    assert decoder is not None, "create brotli-hip decoder"
    for name in DATA:
        _test_case(compu_amd, decoder, golden(name), golden(name + ".compressed.br"))
    assert decoder.describe_error(compu_amd.DecodeError.no_error()) == "NO_ERROR"


def test_golden_batch(gpu):
    import torch

    parts = [golden(n + ".compressed.br") for n in DATA]
    datas = [golden(n) for n in DATA]
    got = _batch(torch, parts + [p + b"trailing" for p in parts], [len(d) for d in datas] * 2)
    for i, (out, st, used) in enumerate(got):
        assert st == B.FINISHED and out == datas[i % 2] and used == len(parts[i % 2])


def test_batch_parity_corpus(gpu, alice):
    import torch

    rnd = random.Random(7)
    datas, parts = [], []
    sizes = [0, 1, 2, 3, 17, 100, 1000, 4096, 20000, 65536, 100000, 400000]
    for it in range(160):
        n = sizes[it % len(sizes)] if it < 2 * len(sizes) else rnd.choice(sizes)
        data = _mk(rnd.randrange(5), n, rnd, alice)
        q = it % 12 if it < 24 else rnd.randrange(12)
        if n > 100000 and q >= 10:
            q = 9  # keeps the CPU side of the test short
        lgwin = rnd.choice([10, 12, 16, 18, 22, 24])
        mode = rnd.choice([B.MODE_GENERIC, B.MODE_TEXT, B.MODE_FONT])
        flush = rnd.choice([0, 0, 0, 777, 5000])
        datas.append(data)
        parts.append(B.compress(data, q, lgwin, mode, flush))
    caps = [len(d) + rnd.choice([0, 0, 5, 1000]) for d in datas]
    got = _batch(torch, parts, caps)
    for i in range(len(parts)):
        assert got[i][1] == B.FINISHED and got[i][0] == datas[i], f"unit {i}: status {got[i][1]}"
        assert got[i][2] == len(parts[i])
        _check_parity(got[i], B.decode(parts[i], caps[i]), f"unit {i}")


def test_many_trees_overflow_path(gpu, alice):
    """quality 11 on mixed text: many literal trees; units whose tables do not fit the small slot take the second launch"""
    import torch

    rnd = random.Random(3)
    datas = []
    for k in range(24):
        parts = [_mk(rnd.randrange(5), rnd.choice([200, 3000, 9000]), rnd, alice) for _ in range(20)]
        datas.append(b"".join(parts))
    comps = [B.compress(d, 11, 22, B.MODE_TEXT) for d in datas]
    got = _batch(torch, comps, [len(d) for d in datas])
    for i in range(len(datas)):
        assert got[i][1] == B.FINISHED and got[i][0] == datas[i], f"unit {i}"


def test_truncation_and_small_out_cap(gpu, alice):
    import torch

    streams = [B.compress(alice[:3000], 5, 16), B.compress(alice[:2000], 11, 22, B.MODE_TEXT), B.compress(b"x" * 500, 1, 10)]
    parts, caps, refs = [], [], []
    for s in streams:
        for cut in range(len(s)):
            parts.append(s[:cut])
            caps.append(4000)
    got = _batch(torch, parts, caps)
    for i, p in enumerate(parts):
        assert got[i][1] == B.NEED_INPUT, f"cut {len(p)}: {got[i][1]}"
        _check_parity(got[i], B.decode(p, caps[i]), f"cut {len(p)}")
    data = alice[:20000]
    s = B.compress(data, 9, 18, B.MODE_TEXT)
    caps = list(range(0, 300)) + list(range(300, len(data), 997))
    got = _batch(torch, [s] * len(caps), caps)
    for c, g in zip(caps, got):
        assert g[1] == B.NEED_OUTPUT and g[0] == data[:c], f"cap {c}"


def test_hand_built_streams(gpu):
    import torch

    cases = [
        (bytes([0x06]), B.FINISHED),           # WBITS 16, ISLAST + ISEMPTY
        (bytes([0x11, 0x01]), -13),            # the large-window marker: WINDOW_BITS
        (bytes([0x21]), B.NEED_INPUT),         # a header cut short
    ]
    # WBITS 16, a metadata metablock with MSKIPBYTES 0, then the bits of 0x00 0x06 read as a further header (libbrotlidec decides)
    cases.append((bytes([0x0c, 0x00, 0x06]), None))
    parts = [c for c, _ in cases]
    got = _batch(torch, parts, [64] * len(parts))
    for (p, want), g in zip(cases, got):
        ref = B.decode(p, 64)
        if want is not None:
            assert ref[0] == want
        _check_parity(g, ref, p.hex())


def test_bit_flips(gpu, alice):
    import torch

    rnd = random.Random(5)
    base = [B.compress(alice[:5000], q, 18, B.MODE_TEXT) for q in (0, 2, 5, 9, 11)]
    base.append(B.compress(bytes(rnd.randrange(256) for _ in range(3000)), 5, 16))  # uncompressed metablocks
    parts = []
    for s in base:
        for _ in range(400):
            b = bytearray(s)
            for _ in range(rnd.choice([1, 1, 2, 3])):
                k = rnd.randrange(len(b))
                b[k] ^= 1 << rnd.randrange(8)
            parts.append(bytes(b))
    cap = 6000
    got = _batch(torch, parts, [cap] * len(parts))
    for i, p in enumerate(parts):
        _check_parity(got[i], B.decode(p, cap), f"flip {i}")


def test_streaming_verdicts(gpu, alice):
    """Decoder::decode with every output size on small streams: the bytes and the final verdict equal libbrotlidec's"""
    import compu_amd

    dec = compu_amd.decoder_interface.brotli_hip()
    data = alice[:1500]
    s = B.compress(data, 9, 16, B.MODE_TEXT)
    for step in (1, 7, 64, 1000):
        dec.reset()
        out = bytearray()
        inp = s
        for _ in range(10000):
            buf = bytearray(step)
            r = dec.decode(inp, buf)
            inp = inp[len(inp) - r.input_remain:]
            out += buf[: step - r.output_remain]
            if r.status == compu_amd.DecodeStatus.Finished:
                break
            assert r.is_ok()
        assert bytes(out) == data
    dec.reset()
    bad = bytearray(s)
    bad[len(bad) // 2] ^= 0x10
    r = dec.decode(bytes(bad), bytearray(4000))
    ref = B.decode(bytes(bad), 4000)
    if ref[0] < 0:
        assert not r.is_ok() and r.status.as_raw() == ref[0]


def test_streaming_long_stream_bounded(gpu, alice):
    import compu_amd
    from bench_support import synth

    data = synth.payloads(256, unit_size=65536).tobytes()  # 16 MiB
    s = B.compress(data, 5, 24)
    dec = compu_amd.decoder_interface.brotli_hip()
    out = bytearray()
    peak = 0
    buf = bytearray(1 << 20)
    for k in range(0, len(s), 65536):
        piece = s[k:k + 65536]
        while True:
            r = dec.decode(piece, buf)
            out += buf[: len(buf) - r.output_remain]
            piece = piece[len(piece) - r.input_remain:]
            peak = max(peak, sum(dec.footprint()))
            if r.status != compu_amd.DecodeStatus.NeedOutput:
                break
        assert r.is_ok()
    while r.status != compu_amd.DecodeStatus.Finished:
        r = dec.decode(b"", buf)
        out += buf[: len(buf) - r.output_remain]
        assert r.is_ok()
    assert bytes(out) == data
    assert peak < 96 << 20, peak


def test_host_and_multi_paths(gpu, alice):
    import torch
    import compu_amd

    rnd = random.Random(9)
    datas = [_mk(rnd.randrange(5), rnd.choice([0, 100, 5000, 70000]), rnd, alice) for _ in range(64)]
    parts = [B.compress(d, rnd.randrange(12), 20) for d in datas]
    caps = [len(d) + 8 for d in datas]
    dev = _batch(torch, parts, caps)
    buf = b"".join(p + b"\0" * (-len(p) % 4) for p in parts)
    offs, o = [], 0
    for p in parts:
        offs.append(o)
        o += len(p) + (-len(p) % 4)
    in_buf = np.frombuffer(buf + b"\0" * 4, dtype=np.uint8).copy()
    in_off = np.array(offs, dtype=np.uint64)
    in_len = np.array([len(p) for p in parts], dtype=np.uint32)
    out_cap = np.array(caps, dtype=np.uint32)
    out_off = np.zeros(len(parts), dtype=np.uint64)
    out_off[1:] = np.cumsum(out_cap[:-1].astype(np.uint64))
    for fn in (compu_amd.decode_batch_host, compu_amd.decode_batch_multi):
        out_buf = np.zeros(int(out_cap.sum()) + 16, dtype=np.uint8)
        ol, iu, st = fn(FMT_BROTLI, in_buf, in_off, in_len, out_buf, out_off, out_cap)
        for i in range(len(parts)):
            assert int(st[i]) == dev[i][1] == B.FINISHED
            assert bytes(out_buf[int(out_off[i]): int(out_off[i]) + int(ol[i])]) == dev[i][0] == datas[i]
