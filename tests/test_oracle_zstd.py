"""Pins the CPU oracle (oracle/oracle_zstd.c): the reference's zstd fixtures through the phases of
tests/decoder.rs:21-77 (should_decode_zstd :119-128), and the system libzstd on generated frames."""
import random

import pytest

import zstd_ref
from conftest import golden
from oracle import oracle as O

Z = zstd_ref.load()
needs_libzstd = pytest.mark.skipif(Z is None, reason="no system libzstd to cross-check against")


@pytest.mark.parametrize("name", ["10x10y", "alice29.txt"])
def test_reference_zstd_fixtures(name):
    data, comp = golden(name), golden(name + ".compressed.zstd")
    d = O.ZstdDecoder()
    assert d.decode(comp, len(data)) == (data, 0, 0, O.FINISHED, 0)  # tests/decoder.rs:25-31
    d.reset()
    out1, ir, orr, st, err = d.decode(comp, 1)  # :34-36
    assert (st, orr, err) == (O.NEED_OUTPUT, 0, 0)
    out2, ir, orr, st, err = d.decode(comp[len(comp) - ir :], len(data) - 1)  # :40-44
    assert (out1 + out2, st) == (data, O.FINISHED)
    d.reset()
    pos, acc = 0, b""
    while True:  # :47-63
        got, ir, orr, st, err = d.decode(comp[pos:], 4096)
        assert not err
        acc += got
        pos = len(comp) - ir
        if st == O.FINISHED:
            break
    assert acc == data
    assert O.lib().orc_zstd_strerror(0) == b"No error detected"  # :74-76
    # checksum and corruption classes of SURVEY.md sec. 8b
    bad = bytearray(comp)
    bad[-1] ^= 1
    assert O.ZstdDecoder().decode(bytes(bad), len(data) + 10)[4] == -22
    assert O.ZstdDecoder().decode(b"\x00\x01\x02\x03\x04", 10)[4] == -10


def test_xxh64_known_answers():
    # published XXH64 test vectors (seed 0)
    assert O.xxh64(b"") == 0xEF46DB3751D8E999
    assert O.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert O.xxh64(b"abc") == 0x44BC2CF5AD770999
    assert O.xxh64(b"Nobody inspects the spammish repetition") == 0xFBCEA83C8A378BF1


def _mk(kind, n, rnd, alice):
    if kind == 0:
        return rnd.randbytes(n)
    if kind == 1:
        s = rnd.randrange(0, max(1, len(alice) - n))
        return alice[s : s + n]
    if kind == 2:
        return bytes(rnd.choice(b"ab") for _ in range(n))
    if kind == 3:
        return b"\0" * n
    return bytes(min(255, int(rnd.expovariate(0.05))) for _ in range(n))


@needs_libzstd
def test_generated_frames_roundtrip_chunked(alice):
    rnd = random.Random(4)
    for it in range(150):
        n = rnd.choice([0, 1, 2, 10, 100, 1000, 5000, 65536, 70000, 150000, 300000])
        data = _mk(rnd.randrange(5), n, rnd, alice)
        comp = zstd_ref.compress(Z, data, rnd.choice([1, 3, 5, 9, 15, 19, -1]), rnd.random() < 0.7, rnd.random() < 0.8)
        d, pos, out = O.ZstdDecoder(), 0, b""
        chunk, ocap = rnd.choice([3, 100, 4096, 10**9]), rnd.choice([100, 4096, 10**6])
        stream = comp + b"zz"
        while True:
            piece = stream[pos : pos + chunk]
            got, ir, orr, st, err = d.decode(piece, ocap)
            assert not err
            out += got
            pos += len(piece) - ir
            if st == O.FINISHED:
                break
        assert out == data and pos == len(comp)


@needs_libzstd
def test_truncated_and_corrupt_frames_vs_libzstd(alice):
    """Truncations must agree exactly with ZSTD_decompressStream (incl. raw blocks streaming through).
    Bit flips must agree except where the system libzstd (1.4.x) is laxer than RFC 8878: it clamps an
    over-read of the last Huffman symbol and does not insist that bitstreams end exactly, so it may
    reach the checksum (or finish) where the oracle already reports corruption; and the order in
    which two simultaneous faults are reported may differ."""
    rnd = random.Random(6)
    lenient = 0
    for it in range(1200):
        n = rnd.choice([50, 500, 5000, 70000])
        data = _mk(rnd.choice([1, 2, 4, 0]), n, rnd, alice)
        comp = bytearray(zstd_ref.compress(Z, data, rnd.choice([1, 3, 9]), rnd.random() < 0.7, rnd.random() < 0.8))
        mode = rnd.randrange(3)
        if mode == 0:
            comp[rnd.randrange(len(comp))] ^= 1 << rnd.randrange(8)
        elif mode == 1:
            comp = comp[: rnd.randrange(len(comp))]
        zo, zir, zor, zst, zerr = zstd_ref.stream_decode_once(Z, bytes(comp), n + 100)
        out, ir, orr, st, err = O.ZstdDecoder().decode(bytes(comp), n + 100)
        if mode != 0:
            assert (out, st, err) == (zo, zst, zerr), (it, mode)
            continue
        if (st, err) == (zst, zerr):
            assert st is None or out == zo
        else:
            assert err in (-20, -70) or zerr in (-20, -70), (it, st, err, zst, zerr)
            lenient += 1
    assert lenient < 30


@needs_libzstd
def test_status_at_every_capacity_is_the_systems_libzstd():
    """One ZSTD_decompressStream call of the system's libzstd, mapped as src/decoder/zstd.rs:113-135 maps it, against the oracle: valid,
    truncated, checksum-damaged and bit-flipped frames (with and without a content size) at output capacities around the block and
    frame sizes.  Pins two rules of the status mapping: an error return leaves output.pos 0, so compu reports the error
    -- also behind whole blocks that fill the range exactly -- unless the range is empty; and nothing of a block that fails is handed
    on.  The bit-flipped frames on which libzstd 1.4.x is laxer than RFC 8878 (its two-symbol Huffman decoder skips a pair's bits
    for the last symbol of a stream and clamps an over-read; the order of its 'destination too small' and 'corrupted' verdicts) are
    counted, not hidden: a few in a hundred flipped frames (0.7 % over 1,440 of them), never different bytes on a frame both accept.
    Where the verdicts agree, so does output_remain, and so does input_remain except on NeedOutput: there libzstd stops reading
    at the block it cannot flush yet, while the decoders here take all the input they are given (compu hands the rest back
    either way, so the next call sees the same bytes)."""
    rnd = random.Random(7)
    total = flips = 0
    lax = set()
    for trial in range(12):
        n = rnd.choice([300000, 70000, 1000, 131072, 262144, 5000])
        data = bytes(rnd.randrange(256) if rnd.random() < 0.3 else 65 + rnd.randrange(3) for _ in range(n))
        for cs in (True, False):
            comp = bytearray(zstd_ref.compress(Z, data, rnd.choice([1, 3, 9]), True, cs))
            variants = [("good", comp, False), ("checksum", bytearray(comp[:-1]) + bytes([comp[-1] ^ 1]), False), ("cut", comp[:-50] if len(comp) > 60 else comp[:-3], False),
                        ("half", comp[: len(comp) // 2], False)]
            for _ in range(6):
                m = bytearray(comp)
                m[rnd.randrange(4, len(m))] ^= 1 << rnd.randrange(8)
                variants.append(("flip", m, True))
                flips += 1
            for name, c, flipped in variants:
                for cap in (0, 10, n // 2, n - 1, n, n + 1, 131072, 262144):
                    out, inr, outr, st, err = zstd_ref.stream_decode_once(Z, bytes(c), cap)
                    got = O.ZstdDecoder(0).decode(bytes(c), cap)
                    total += 1
                    same = st == got[3] and (st is not None or err == got[4]) and (st is None or out == got[0])
                    if same:  # ... and the output left over, and the input too (an error return leaves both where the caller set them)
                        assert outr == got[2] and (st == 1 or inr == got[1]), (name, n, cs, cap, st, err, inr, outr, got[1:])
                    else:
                        assert flipped, (name, n, cs, cap, st, err, got[1:])  # only bit flips may differ ...
                        assert got[3] is None and got[4] in (-20, -70), (name, cap, st, err, got[1:])  # ... and only where the oracle is the stricter one
                        lax.add(bytes(c))
    assert len(lax) * 25 < flips, (len(lax), flips, total)


def _stream_verdict(decoder, frame, piece, ocap):
    """-> (output, error code or 0) of feeding `frame` in pieces of `piece` bytes with `ocap` bytes of output room per call"""
    pos, out = 0, b""
    for _ in range(200000):
        chunk = frame[pos : pos + piece]
        got, ir, orr, st, err = decoder.decode(chunk, ocap)
        if err:
            return out, err
        out += got
        pos += len(chunk) - ir
        if st == O.FINISHED:
            return out, 0
    raise AssertionError("no end")


def test_an_offset_beyond_the_window_is_corruption_however_the_stream_is_sliced():
    """the verdict on a match that reaches behind the frame's window, but not behind its start, must not depend
    on how much history the decoder still holds.  Frames written by hand (tests/zstd_ref.py::craft_offset_frame: raw blocks, then
    one sequence with a chosen offset; window 1 KiB): offsets up to the window decode, anything farther is -20 -- whole, in small
    pieces, with small output ranges.  (libzstd 1.4.8 copies whatever its ring holds there, without an error: measured when this
    test was written -- offset 2000 of 2000 bytes returned other bytes than the frame's first three.)"""
    for blocks, offset, ok in ((2, 1000, True), (2, 1024, True), (2, 1025, False), (2, 1500, False), (2, 2000, False), (2, 2001, False), (1, 900, True), (1, 1001, False)):
        frame, data = zstd_ref.craft_offset_frame(blocks, 1000, offset)
        want = data + data[len(data) - offset : len(data) - offset + 3] if ok else None
        for piece, ocap in ((10**9, 10**6), (7, 10**6), (10**9, 100), (300, 333)):
            out, err = _stream_verdict(O.ZstdDecoder(), frame, piece, ocap)
            assert (err == 0) == ok and (not ok or out == want) and (ok or err == -20), (blocks, offset, piece, ocap, err)
