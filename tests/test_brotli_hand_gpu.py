"""Brotli on the GPU against libbrotlidec: hand-built streams (tests/brotli_cases.py), the result of every streaming call, a long
stream through the bounded streaming decoder, and a full-size batch."""
import random

import numpy as np
import pytest

import brotli_cases as K
import brotli_ref as B
from test_brotli_gpu import _batch, _check_parity
from test_inflate_gpu import _mk

pytestmark = pytest.mark.gpu


def _gpu_calls(dec, data, cap, max_calls=100000):
    """the same loop as brotli_ref.stream_calls through Decoder::decode of brotli_hip()"""
    import compu_amd

    dec.reset()
    calls, rest = [], data
    for _ in range(max_calls):
        buf = bytearray(cap)
        r = dec.decode(rest, buf)
        rest = rest[len(rest) - r.input_remain:]
        st = r.status.as_raw() if not r.is_ok() else int(r.status)
        calls.append((st, bytes(buf[: cap - r.output_remain]), r.input_remain))
        if st == B.FINISHED or st < 0 or (st == B.NEED_INPUT and not rest):
            break
        assert st != compu_amd.DecodeStatus.NeedInput or rest
    return calls


@pytest.fixture(scope="module")
def cases():
    return K.all_cases()


def test_hand_built_batch(gpu, cases):
    import torch

    parts = [c for _, c, _ in cases] + [bytes([0x11, 0x01]), bytes([0x06])]
    outs = [o for _, _, o in cases] + [b"", b""]
    got = _batch(torch, parts, [len(o) + 16 for o in outs])
    for i, p in enumerate(parts):
        ref = B.decode(p, len(outs[i]) + 16)
        name = cases[i][0] if i < len(cases) else p.hex()
        _check_parity(got[i], ref, name)
        if i < len(cases):
            assert got[i][1] == B.FINISHED and got[i][0] == outs[i], name
    assert got[-2][1] == -13  # the large-window marker: WINDOW_BITS
    # the many-trees unit beside units that fit the first pass, several times over: the overflow list takes every copy
    many = cases[0][1]
    small = [B.compress(outs[1][:k], 5, 16) for k in (0, 100, 5000)]
    mix = [many, small[0], many, small[1], small[2], many]
    got = _batch(torch, mix, [len(outs[0])] + [6000] * 4 + [len(outs[0])])
    for p, g in zip(mix, got):
        assert g[1] == B.FINISHED and g[0] == B.decode(p, 6000)[1]


def test_hand_built_streaming(gpu, cases):
    import compu_amd

    dec = compu_amd.decoder_interface.brotli_hip()
    for name, comp, out in cases:
        for cap in (1 << 20, 997):
            assert _gpu_calls(dec, comp, cap) == B.stream_calls(comp, cap), (name, cap)
    dev, pinned = dec.footprint()[1], dec.footprint()[0]
    assert dev < 4 << 20 and pinned < 1 << 20, (dev, pinned)  # the worst-case table slot is counted


def test_streaming_verdicts_every_capacity(gpu, alice):
    """per call (status, bytes handed on, input_remain) against libbrotlidec at every output capacity up to the stream's size,
    on streams that decode and on damaged ones"""
    import compu_amd

    dec = compu_amd.decoder_interface.brotli_hip()
    good = [B.compress(alice[:300], 5, 16, B.MODE_TEXT), B.compress(b"ab" * 100, 0, 10) + b"tail"]
    rnd = random.Random(4)
    bad = []
    for s in (B.compress(alice[:400], 9, 16), B.compress(alice[:400], 2, 16)):
        for _ in range(6):
            b = bytearray(s)
            b[rnd.randrange(2, len(b))] ^= 1 << rnd.randrange(8)
            bad.append(bytes(b))
    for s in good + bad:
        caps = range(1, len(B.decode(s, 100000)[1]) + 2) if s in good else range(1, 420, 7)
        for cap in caps:
            want = B.stream_calls(s, cap)
            got = _gpu_calls(dec, s, cap)
            # input is taken whole: while the stream goes on input_remain is 0; libbrotlidec may leave input unread while its
            # ring buffer and the caller's output are full; statuses and bytes agree call for call
            assert [(st, o) for st, o, _ in got] == [(st, o) for st, o, _ in want], (s.hex(), cap)
            if want[-1][0] == B.FINISHED:
                assert got[-1][2] == want[-1][2]
            # once the end of the stream is known, the bytes behind it are given back on every call
            trailing = want[-1][2] if want[-1][0] == B.FINISHED else 0
            assert all(r in (0, trailing) for st, _, r in got if st in (B.NEED_OUTPUT, B.NEED_INPUT))


def test_streaming_64mib_lgwin24_bounded(gpu):
    """a 64 MiB stream with a 16 MiB window in 64 KiB pieces: output behind the window is dropped between calls and the
    footprint stays near window + piece"""
    import compu_amd
    from bench_support import synth

    base = synth.payloads(4)  # 256 KiB; each 256 KiB block repeats it with small changes, so most of the stream is long matches
    rnd = np.random.default_rng(1)
    blocks = []
    for k in range(256):
        b = base.copy()
        idx = rnd.integers(0, len(b), 1000)
        b[idx] = rnd.integers(0, 256, len(idx), dtype=np.uint8)
        blocks.append(b.tobytes())
    data = b"".join(blocks)
    # a run goes on from the last metablock boundary, so a call costs O(metablock + piece): the stream is flushed every MiB
    s = B.compress(data, 5, 24, flush_every=1 << 20)
    dec = compu_amd.decoder_interface.brotli_hip()
    h = bytearray()
    peak = 0
    buf = bytearray(1 << 20)
    r = None
    for k in range(0, len(s), 65536):
        piece = s[k:k + 65536]
        while True:
            r = dec.decode(piece, buf)
            h += buf[: len(buf) - r.output_remain]
            piece = piece[len(piece) - r.input_remain:]
            peak = max(peak, sum(dec.footprint()))
            if r.status != compu_amd.DecodeStatus.NeedOutput:
                break
        assert r.is_ok()
    while r.status != compu_amd.DecodeStatus.Finished:
        r = dec.decode(b"", buf)
        h += buf[: len(buf) - r.output_remain]
        peak = max(peak, sum(dec.footprint()))
        assert r.is_ok()
    assert bytes(h) == data
    # window 16 MiB + what one run decodes past its checkpoint + the table slots; far below the 64 MiB of output
    assert peak < 40 << 20, peak


def test_full_size_batch_q5(gpu):
    """65 536 x 64 KiB bench_support.synth units at quality 5 in one batch, every unit against its payload"""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from bench_support import synth
    import compu_amd

    n, unit = 65536, 65536
    pay = synth.payloads(n)
    mv = memoryview(pay)
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(lambda i: B.compress(bytes(mv[i * unit:(i + 1) * unit]), 5, 22), range(n)))
    lens = np.array([len(p) for p in parts], np.int32)
    padded = [p + b"\0" * (-len(p) % 4) for p in parts]
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(np.array([len(p) for p in padded[:-1]], np.int64))
    buf = np.frombuffer(b"".join(padded) + b"\0" * 4, np.uint8).copy()
    dev = torch.device("cuda:0")
    d_out = torch.zeros(n * unit, dtype=torch.uint8, device=dev)
    ol, iu, st = compu_amd.decode_batch(compu_amd.FMT_BROTLI, torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev),
                                        torch.from_numpy(lens).to(dev), d_out, torch.arange(n, dtype=torch.int64, device=dev) * unit,
                                        torch.full((n,), unit, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert bool((st == B.FINISHED).all()) and bool((ol == unit).all())
    assert torch.equal(iu.cpu(), torch.from_numpy(lens))
    assert torch.equal(d_out, torch.from_numpy(pay).to(dev))
