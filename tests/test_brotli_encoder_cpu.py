"""The brotli encoder without a GPU: its core (compu_amd/csrc/brotli_enc_core.h, the same source the kernel runs) built for the host
and checked with the system's libbrotlidec, the stream forms it writes, the output bound, argument checks of the batch entry point
and the mirrors."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import brotli_enc_host as H
import brotli_ref as B
from conftest import ROOT, golden

FMT_BROTLI = 101
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 1023, 65535, 65536, 131071, 131072, 131073, 400000]
QUALITIES = [1, 3, 5, 11]  # one per match finder group


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return H.build_driver(str(tmp_path_factory.mktemp("benc")))


def _payloads():
    alice = golden("alice29.txt")
    tenx = golden("10x10y")
    rnd = np.random.default_rng(7).integers(0, 256, 400000, dtype=np.uint8).tobytes()
    from bench_support import synth

    syn = synth.payloads(7).tobytes()
    return {"alice": (alice * 3)[:400000], "10x10y": (tenx * 40000)[:400000], "random": rnd, "one": b"\x61" * 400000, "synth": syn}


@pytest.fixture(scope="module")
def payloads():
    return _payloads()


def _roundtrip(stream, data):
    st, out, used = B.decode(stream, len(data) + 16)
    assert st == B.FINISHED, (st, len(data))
    assert used == len(stream)
    assert out == data


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("lgwin", [10, 16, 22])
def test_round_trips_through_libbrotlidec(driver, payloads, quality, lgwin):
    jobs = [p[:n] for p in payloads.values() for n in SIZES]
    for data, s in zip(jobs, H.encode(driver, quality, lgwin, jobs)):
        assert s is not None
        _roundtrip(s, data)
        assert H.first_metablock(s)["wbits"] == lgwin


def test_other_window_sizes(driver, payloads):
    data = payloads["alice"][:200000]
    for lgwin in [11, 15, 17, 18, 24]:
        s, = H.encode(driver, 5, lgwin, [data])
        _roundtrip(s, data)
        assert H.first_metablock(s)["wbits"] == lgwin


def test_default_header_is_not_detected(driver):
    # WBITS 22: the low nibble of the first byte is 0xB, which Detection::detect answers Unknown for (tests/encoder.rs:181)
    s, = H.encode(driver, 11, 22, [b"hello brotli"])
    assert s[0] & 0xF == 0xB
    import compu_amd

    assert compu_amd.lib().chip_detect(s, len(s)) == compu_amd.Detection.Unknown


def test_empty_input_is_wbits_and_an_empty_last_metablock(driver):
    s, = H.encode(driver, 11, 22, [b""])
    assert s == bytes([0x0B | (3 << 4)])
    _roundtrip(s, b"")


def test_stream_forms(driver, payloads):
    alice = payloads["alice"][:100000]
    forms, ring_checked = set(), []
    for q in QUALITIES:
        for name, data in (("alice", alice), ("10x10y", payloads["10x10y"][:5000]), ("ab", b"abababababababab" * 50 + b"xyz"),
                           ("synth", payloads["synth"][:65536])):
            m = H.first_metablock(H.encode(driver, q, 22, [data])[0])
            assert "lit" in m, (q, name)
            assert m["npostfix"] == 0 and m["ndirect"] == 0 and m["cmode"] == 0
            forms |= {m["lit"][0], m["ic"][0], m["dist"][0]}
            if q >= 2 and name == "alice":
                # ring hits: short distance codes 0..3, or implicit distances in cells 0..127 beyond the one symbol there that the
                # metablock's closing literal-only command may use
                assert sum(1 for x in m["ic"][1][:128] if x) >= 2 or any(m["dist"][1][:4]), q
                ring_checked.append(q)
    assert ring_checked == [3, 5, 11]
    assert forms == {"simple", "complex"}
    # incompressible data: the first metablock is uncompressed
    m = H.first_metablock(H.encode(driver, 5, 22, [payloads["random"][:100000]])[0])
    assert m.get("uncompressed") and m["mlen"] == 100000
    # over 128 KiB: metablocks of 128 KiB
    m = H.first_metablock(H.encode(driver, 5, 22, [payloads["alice"][:300000]])[0])
    assert m["mlen"] == 128 << 10


def test_flushed_segments_decode_as_one_stream(driver, payloads):
    rnd = random.Random(3)
    for q in QUALITIES:
        for name in ("alice", "synth", "10x10y", "random"):
            data = payloads[name][: rnd.choice([1000, 70000, 300000])]
            cuts = sorted(rnd.sample(range(len(data) + 1), 5))
            segs = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
            s, = H.encode(driver, q, 22, [segs])
            _roundtrip(s, data)
    # an empty first segment (a Flush before any input) and empty segments between
    data = payloads["alice"][:50000]
    s, = H.encode(driver, 5, 22, [[b"", data[:100], b"", data[100:], b""]])
    _roundtrip(s, data)


def test_segments_carry_the_distance_ring(driver):
    # the first segment ends with a match at distance 300, the second one holds one match at distance 300: with the ring carried it
    # is a ring hit (distance symbol 0, the only one in the second segment's distance code), with a fresh ring an explicit distance
    rnd = random.Random(4)
    x, y = rnd.randbytes(300), rnd.randbytes(300)
    segs = [y + y, x + x]
    s, = H.encode(driver, 5, 22, [segs])
    _roundtrip(s, y + y + x + x)
    first, = H.encode(driver, 5, 22, [[segs[0], b""]])  # the first segment, then a closing byte
    m = H.first_metablock(s[len(first) - 1:], wbits=False)
    dist = m["dist"][1]
    assert dist[0] and not any(dist[1:]), dist[:20]
    fresh, = H.encode(driver, 5, 22, [[segs[1]]])  # the same segment with a fresh ring takes an explicit distance
    assert not H.first_metablock(fresh)["dist"][1][0]


def test_encode_bound_covers_incompressible_data(driver, payloads):
    import compu_amd

    rnd = payloads["random"]
    sizes = [0, 1, 2, 100, 65535, 65536, 131071, 131072, 131073, 262144, 400000]
    for q in (1, 11):
        for data, s in zip([rnd[:n] for n in sizes], H.encode(driver, q, 22, [rnd[:n] for n in sizes])):
            assert len(s) <= compu_amd.encode_bound(FMT_BROTLI, len(data)), (q, len(data), len(s))
            _roundtrip(s, data)
    for n in [0, 1, 1 << 17, (1 << 17) + 1, 1 << 20, 5_000_000]:
        mb = max(1, -(-n // (128 << 10)))
        assert compu_amd.encode_bound(FMT_BROTLI, n) >= n + 3 * mb + 2


def test_batch_rejects_out_of_range_quality_mode_and_level():
    import compu_amd

    L = compu_amd.lib()
    one = C.c_void_p(8)  # never dereferenced: the arguments are checked first
    for level, mode in ((12, 0), (3, 4), (-1, 0), (5, -1)):
        rc = L.chip_encode_batch_ex(FMT_BROTLI, level, mode, 1, one, one, one, one, one, one, one, one, None)
        assert rc == -101, (level, mode, rc)


def test_mirrors():
    import compu_amd

    assert compu_amd.FMT_BROTLI == FMT_BROTLI
    assert [int(m) for m in compu_amd.BrotliEncoderMode] == [1, 2, 3]
    o = compu_amd.BrotliOptions()
    assert (o._quality, o._mode) == (0, 0)
    o = compu_amd.BrotliOptions().quality(5).mode(compu_amd.BrotliEncoderMode.Font)
    assert (o._quality, o._mode) == (5, 3)
    for bad in (0, 12):
        with pytest.raises(AssertionError):
            compu_amd.BrotliOptions().quality(bad)
    hdr = open(os.path.join(ROOT, "include", "compu_hip.h")).read()
    assert "chip_brotli_encoder_opts" in hdr and "chip_encoder_new_brotli" in hdr
    hpp = open(os.path.join(ROOT, "compu_amd", "host", "compu.hpp")).read()
    assert "BrotliEncoderMode" in hpp and "chip_encoder_new_brotli" in hpp and "Generic = 1" in hpp
    rs = open(os.path.join(ROOT, "integration", "src", "hip_sys.rs")).read()
    assert "pub struct chip_brotli_encoder_opts" in rs and "chip_encoder_new_brotli" in rs
    glue = open(os.path.join(ROOT, "integration", "src", "encoder", "hip.rs")).read()
    assert "pub fn brotli_hip(opts: BrotliOptions) -> Option<Encoder>" in glue
    assert "opts.inner" in glue
