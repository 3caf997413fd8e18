"""Life cycle of the launch slots of the four caches that tests/test_inflate_gpu.py does not reach: the dynamic
deflate levels, the zstd encoder, the brotli encoder and the brotli decoder.  Every test is the call sequence of an ordinary
caller -- trim between batches, batches of growing size on one stream, streaming objects made and freed -- and checks the
results the way the codec's own test file does."""
import functools
import zlib

import numpy as np
import pytest

import brotli_ref as B
from conftest import golden
from test_brotli_encoder_gpu import _batch as _brotli_enc_batch, _libdec
from test_inflate_gpu import run_batch
from test_zstd_encoder_gpu import _batch as _zstd_enc_batch, _zdec

pytestmark = pytest.mark.gpu
FMT_ZSTD, FMT_BROTLI, FMT_ZLIB = 100, 101, 15
UNIT = 4096
GROWN = 300  # more than 1.25 x a slot of one wave, fewer than the resident waves of any of the kernels


@functools.lru_cache(maxsize=None)
def _payloads():
    from bench_support import synth

    pay = synth.payloads(GROWN, unit_size=UNIT).tobytes()
    return tuple(pay[i * UNIT : (i + 1) * UNIT] for i in range(GROWN))


@functools.lru_cache(maxsize=None)
def _brotli_streams():
    return tuple(B.compress(d, 5, 22) for d in _payloads())


def _deflate_level6(torch, n):
    """chip_encode_batch(zlib, level 6: deflate_dyn2_kernel): the oracle's bytes, and zlib decodes them to the payload"""
    import compu_amd as c
    from oracle import oracle as O

    datas = _payloads()[:n]
    lens = np.full(n, UNIT, np.int32)
    offs = np.arange(n, dtype=np.int64) * UNIT
    buf = np.frombuffer(b"".join(datas), np.uint8).copy()
    cap = c.encode_bound(FMT_ZLIB, UNIT)
    caps = np.full(n, cap, np.int32)
    ooff = np.arange(n, dtype=np.int64) * (cap + 7)
    dev = "cuda:0"
    d_out = torch.full((n * (cap + 7) + 8,), 0xA5, dtype=torch.uint8, device=dev)
    out_len, status = c.encode_batch(FMT_ZLIB, 6, torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev),
                                     d_out, torch.from_numpy(ooff).to(dev), torch.from_numpy(caps).to(dev))
    torch.cuda.synchronize()
    h, ol, st = d_out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    comps = []
    for i, d in enumerate(datas):
        assert st[i] == 2, (i, st[i])
        assert (h[ooff[i] + cap : ooff[i] + cap + 7] == 0xA5).all()
        comp = bytes(h[ooff[i] : ooff[i] + ol[i]])
        ref, _ir, _or, est = O.DeflateEncoder(FMT_ZLIB, 6).encode(d, cap + 64, O.OP_FINISH)
        assert est == O.ENC_FINISHED and comp == ref, i
        assert zlib.decompress(comp, FMT_ZLIB) == d
        comps.append(comp)
    return comps


def _zstd_encode(torch, n):
    """chip_encode_batch(zstd): libzstd decodes every frame to the payload"""
    datas = _payloads()[:n]
    frames, st = _zstd_enc_batch(torch, list(datas))
    assert (st == 2).all(), st
    for f, d in zip(frames, datas):
        assert _zdec(f, len(d)) == d
    return frames


def _brotli_encode(torch, n):
    """chip_encode_batch(brotli): libbrotlidec decodes every stream to the payload"""
    datas = _payloads()[:n]
    streams, st = _brotli_enc_batch(torch, list(datas), 5)
    assert (st == 2).all(), st
    for s, d in zip(streams, datas):
        assert _libdec(s, d) == d
    return streams


def _brotli_decode(torch, n):
    """chip_decode_batch(brotli) of libbrotlienc's streams: the payload, the whole input used"""
    datas, parts = _payloads()[:n], _brotli_streams()[:n]
    outs, _ol, iu, st = run_batch(torch, FMT_BROTLI, list(parts), [UNIT] * n)
    for i in range(n):
        assert int(st[i]) == B.FINISHED and outs[i] == datas[i] and int(iu[i]) == len(parts[i]), i
    return outs


CODECS = pytest.mark.parametrize("run", [_deflate_level6, _zstd_encode, _brotli_encode, _brotli_decode], ids=lambda f: f.__name__.strip("_"))


@CODECS
def test_trim_run_trim_run(gpu, run):
    """chip_trim() releases the slot of a non-default stream; the next batch there allocates it again: same, correct, results"""
    import compu_amd as c

    torch = gpu
    stream = torch.cuda.Stream()
    results = []
    for _ in range(2):
        c.trim()
        with torch.cuda.stream(stream):
            results.append(run(torch, 8))
    assert results[0] == results[1]


@CODECS
def test_slot_grows_on_one_stream(gpu, run):
    """1 unit, 300 units, 1 unit on one stream: the slot of one wave is replaced by a larger one (sized by the headroom rule,
    not by the resident-wave cap) and then serves the small batch again"""
    torch = gpu
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        first = run(torch, 1)
        grown = run(torch, GROWN)
        again = run(torch, 1)
    assert len(grown) == GROWN and grown[0] == first[0]
    assert again == first


def test_streaming_objects_release_and_reallocate_their_slots(gpu):
    """A streaming zstd encoder and a streaming brotli decoder, made, used and freed twice: the second pair, on streams of its
    own, gives the same bytes, and the brotli decoder's device footprint is the same -- the first pair's slots went with their
    streams and a fresh slot is sized for one wave.  After chip_trim() with both objects alive each does a second stream."""
    import compu_amd as c

    alice = golden("alice29.txt")
    data, data2 = alice[:65536], alice[65536:131072]
    comp, comp2 = B.compress(data, 5, 22), B.compress(data2, 5, 22)

    def encode(enc, d):
        out = c.Vec()
        r = enc.encode_vec_full(d, out, c.EncodeOp.Finish)
        assert r.status == c.EncodeStatus.Finished and r.input_remain == 0
        frame = bytes(out)
        assert _zdec(frame, len(d)) == d
        return frame

    def decode(dec, s, d):
        out = c.Vec()
        r = dec.decode_vec_full(s, out)
        assert r.status == c.DecodeStatus.Finished and r.input_remain == 0
        assert bytes(out) == d
        return bytes(out)

    rounds = []
    for k in range(2):
        enc, dec = c.encoder_interface.zstd_hip(), c.decoder_interface.brotli_hip()
        assert enc is not None and dec is not None
        rounds.append((encode(enc, data), decode(dec, comp, data), dec.footprint()[1]))
        if k == 0:
            enc.close()
            dec.close()
    assert rounds[0] == rounds[1]
    c.trim()
    assert enc.reset() and dec.reset()
    encode(enc, data2)
    decode(dec, comp2, data2)
    enc.close()
    dec.close()
