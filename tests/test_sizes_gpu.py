"""chip_decode_batch_sizes on the GPU (DEFLATE / zlib / gzip / auto, zstd, routed batches): the hand-built cases against the oracle, generated payloads
against chip_decode_batch on the same device buffer, damaged streams (the size pass, then a decode into exactly the room it
named), no memory taken per unit, every result entry written, and a size pass racing a decode on one stream."""
import os
import random
import threading
import zlib

import numpy as np
import pytest

import deflate_cases as K
import sizes_ref as R
from test_inflate_gpu import _mk, _pack, oracle_batch, run_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON64, POISON32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def run_sizes(torch, fmt, parts, d_in=None):
    """The size pass over `parts` in one launch; the three result arrays are poisoned first and every entry must be written.
    Returns (out_size, in_used, status) on the host."""
    import compu_amd

    buf, offs, lens = _pack(parts)
    n = len(parts)
    if d_in is None:
        d_in = torch.from_numpy(buf).to(DEV)
    size = torch.full((n,), POISON64, dtype=torch.int64, device=DEV)
    used = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    st = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    compu_amd.decode_batch_sizes(fmt, d_in, torch.from_numpy(offs).to(DEV), torch.from_numpy(lens).to(DEV), size, used, st)
    torch.cuda.synchronize()
    size, used, st = size.cpu().numpy(), used.cpu().numpy(), st.cpu().numpy()
    assert (size != POISON64).all() and (used != POISON32).all() and (st != POISON32).all(), "a result entry was not written"
    return size, used, st


def test_hand_built_deflate_cases(gpu):
    """All 523 cases, each as a unit of its own format: status and size are the oracle's at ample capacity, in_used is the oracle's
    on CHIP_FINISHED and chip_decode_batch's otherwise.  The two cases whose only fault is the check value read CHIP_FINISHED with
    the true length (rule 2 / 4 of include/compu_hip.h)."""
    cases = K.all_cases()
    assert len(cases) == 523
    by_fmt = {}
    for c in cases:
        by_fmt.setdefault(K.MODES[c.fmt], []).append(c)
    exempt = set()
    for fmt, cs in by_fmt.items():
        parts = [c.data for c in cs]
        size, used, st = run_sizes(gpu, fmt, parts)
        _outs, d_ol, d_iu, d_st = run_batch(gpu, fmt, parts, [len(c.content) + 64 for c in cs])
        for j, c in enumerate(cs):
            e_st, e_size, e_used = R.expected(c)
            where = (c.name, int(st[j]), int(size[j]), int(used[j]), e_st, e_size, e_used, int(d_st[j]), int(d_iu[j]))
            print(*where)
            assert (int(st[j]), int(size[j])) == (e_st, e_size), where
            if R.by_rule_exempt(c):
                exempt.add(c.name)
                assert int(d_st[j]) == -3 and int(d_ol[j]) == e_size, where  # the decode that follows reports it
            else:
                assert (int(d_st[j]), int(d_ol[j])) == (e_st, e_size), where  # (the yardstick agrees with the oracle here)
            assert int(used[j]) == (e_used if e_st == R.FINISHED else int(d_iu[j])), where
    assert exempt == R.DEFLATE_EXCEPTIONS == {"zlib_adler", "gzip_crc"}
    # the wrapped cases again through CHIP_FMT_DETECT: each unit answers as in a batch of its own format (units the router does not
    # send to the inflate kernel -- headers Detection does not know -- are answered by the router, as in a routed decode)
    import compu_amd
    wrapped = [c for c in cases if c.fmt in ("zlib", "gzip", "auto")]
    parts = [c.data for c in wrapped]
    size, used, st = run_sizes(gpu, 0, parts)
    a_size, a_used, a_st = run_sizes(gpu, K.MODES["auto"], parts)
    _o, d_ol, d_iu, d_st = run_batch(gpu, 0, parts, [len(c.content) + 64 for c in wrapped])
    routed = 0
    for j, c in enumerate(wrapped):
        kind = compu_amd.Detection.detect(c.data)
        where = (c.name, int(st[j]), int(size[j]), int(used[j]))
        if kind in (compu_amd.Detection.Gzip, compu_amd.Detection.Zlib):
            routed += 1
            assert (int(st[j]), int(size[j]), int(used[j])) == (int(a_st[j]), int(a_size[j]), int(a_used[j])), where
        else:
            assert (int(st[j]), int(size[j]), int(used[j])) == (int(d_st[j]), int(d_ol[j]), int(d_iu[j])), where
            assert int(st[j]) in (0, 4), where
    assert routed >= 0.8 * len(wrapped)


def test_hand_built_zstd_cases(gpu):
    """All of tests/zstd_cases.py: status and size are the oracle's at ample capacity, in_used the oracle's on CHIP_FINISHED and
    chip_decode_batch's otherwise.  Exempt by rule (named in sizes_ref.ZSTD_EXCEPTIONS): a fault in the content of a Huffman literal
    stream, or in the checksum -- CHIP_FINISHED here and the error in the decode that follows, which still never lacks room, unless the
    fault's consequence is met by a check the pass does make (Frame_Content_Size against the counted length)."""
    import zstd_cases as Z

    cases = Z.all_cases()
    parts = [c.frame for c in cases]
    size, used, st = run_sizes(gpu, 100, parts)
    caps = [(len(c.want) if isinstance(c.want, bytes) else R.ZSTD_ERR_CAP) + 4096 for c in cases]
    _o, d_ol, d_iu, d_st = run_batch(gpu, 100, parts, caps, check_tail=False)
    _o, x_ol, x_iu, x_st = run_batch(gpu, 100, parts, [max(int(s), 1) for s in size], check_tail=False)
    exempt, kinds, differs = set(), set(), set()
    for j, c in enumerate(cases):
        e = R.zstd_expected(c)
        where = (c.name, int(st[j]), int(size[j]), int(used[j]), e, int(d_st[j]), int(d_ol[j]), int(d_iu[j]), int(x_st[j]))
        print(*where)
        if e is None:
            exempt.add(c.name)
            # the pass cannot see the fault itself; it either finishes, or meets the fault's consequence in a check it does make
            # (the literals' stated size no longer adds up to Frame_Content_Size) -- then with the decoder's verdict
            assert int(st[j]) in (2, c.want) and int(d_st[j]) == c.want, where
            if int(st[j]) == 2:
                assert int(x_st[j]) == c.want, where  # rule 3: the decode that follows reports it, and never lacks room
            if c.name == "checksum_wrong":
                assert int(size[j]) == int(d_ol[j]), where  # the true length: every block decoded
            continue
        e_st, e_size, e_used = e
        assert int(st[j]) == e_st == int(d_st[j]), where
        if e_st < 0 and int(d_ol[j]) != e_size:
            # An erroring frame: the oracle (libzstd's streaming interface) hands on nothing of a frame whose error it meets, the batch
            # decoder's out_len counts the whole blocks in front of the error (include/compu_hip.h).  Rule 2 of the contract names the
            # decoder's out_len as the length "counted in front of it", so that is the yardstick here; the status is the oracle's.
            differs.add(c.name)
            assert e_size <= int(d_ol[j]), where
            assert int(size[j]) == int(d_ol[j]), where
        else:
            assert int(size[j]) == e_size, where
        assert int(used[j]) == (e_used if e_st == 2 else int(d_iu[j])), where
        if e_st == 2:
            assert int(x_st[j]) == 2 and int(x_ol[j]) == e_size, where
            kinds |= c.tags
    assert exempt == R.ZSTD_EXCEPTIONS
    print("erroring frames whose counted length is the decoder's, not the oracle's:", sorted(differs))
    for t in ("window_nofcs", "single_fcs4", "rep_across_blocks", "rle_ll", "rep_ll_after_fse"):
        assert t in kinds, t
    byname = {c.name: j for j, c in enumerate(cases)}
    assert int(st[byname["fcs_off_by_1_True"]]) == -20


def test_generated_zstd_frames_match_the_decode(gpu, alice):
    """Rule 1 for zstd: system libzstd with and without Frame_Content_Size, with and without checksum, this library's zstd encoder,
    skippable frames, trailing bytes, sizes 0 .. 400 000 and multi-megabyte multi-block frames."""
    import compu_amd
    import zstd_ref
    from bench_support import synth

    z = zstd_ref.load()
    assert z is not None
    rnd = random.Random(31)
    pay = synth.payloads(8).tobytes()
    parts, want = [], []
    for n in [0, 1, 2, 10, 100, 1000, 5000, 65536, 70000, 131072, 131073, 140000, 400000]:
        for level in (1, 3, 9, 19):
            for fcs in (True, False):
                s = rnd.randrange(0, len(pay) - n + 1)
                data = pay[s : s + n] if rnd.random() < 0.6 else _mk(rnd.randrange(5), n, rnd, alice * 3)
                parts.append(zstd_ref.compress(z, data, level, rnd.random() < 0.7, fcs) + (b"tail" if rnd.random() < 0.2 else b""))
                want.append(len(data))
    parts.append(b"\x50\x2a\x4d\x18\x03\x00\x00\x00abc")
    want.append(0)
    for k, data in enumerate([pay * 6, os.urandom(3 << 20), b"\0" * (40 << 20), (alice * 30)[: 5 << 20]]):
        parts.append(zstd_ref.compress(z, data, [3, 1, 9, 1][k], True, k % 2 == 0))
        want.append(len(data))
    size, used, st = run_sizes(gpu, 100, parts)
    _o, ol, iu, dst = run_batch(gpu, 100, parts, [max(w, 1) for w in want], check_tail=False)
    for j in range(len(parts)):
        where = (j, int(st[j]), int(size[j]), int(used[j]), int(dst[j]), int(ol[j]), int(iu[j]), want[j])
        assert int(dst[j]) == 2 and int(ol[j]) == want[j], where
        assert (int(st[j]), int(size[j]), int(used[j])) == (2, int(ol[j]), int(iu[j])), where
    # this library's zstd encoder (frames with Frame_Content_Size and checksum)
    n = 96
    upay = synth.payloads(n)
    lens_in = gpu.from_numpy(np.array([rnd.choice([0, 1, 100, 5000, 65536]) for _ in range(n)], np.int32)).to(DEV)
    d_pay = gpu.from_numpy(upay).to(DEV)
    offs = gpu.arange(n, dtype=gpu.int64, device=DEV) * synth.UNIT
    bound = (int(compu_amd.encode_bound(100, synth.UNIT)) + 79) & ~15
    for level in (1, 3, 9, 19):
        d_comp = gpu.zeros(n * bound, dtype=gpu.uint8, device=DEV)
        coff = gpu.arange(n, dtype=gpu.int64, device=DEV) * bound
        clen, est = compu_amd.encode_batch(100, level, d_pay, offs, lens_in, d_comp, coff, gpu.full((n,), bound, dtype=gpu.int32, device=DEV))
        gpu.cuda.synchronize()
        assert bool((est == 2).all())
        s_size, s_used, s_st = compu_amd.decode_batch_sizes(100, d_comp, coff, clen)
        d_out = gpu.zeros(n * synth.UNIT, dtype=gpu.uint8, device=DEV)
        ol, iu, dst = compu_amd.decode_batch(100, d_comp, coff, clen, d_out, offs, gpu.full((n,), synth.UNIT, dtype=gpu.int32, device=DEV))
        gpu.cuda.synchronize()
        assert bool((dst == 2).all()) and bool((ol == lens_in).all()), level
        assert bool((s_st == 2).all()) and gpu.equal(s_size, ol.to(gpu.int64)) and gpu.equal(s_used, iu), level


@pytest.mark.timeout(1500)
def test_full_launch_size_mixed(gpu):
    """65 536 gzip + zstd units x 64 KiB through CHIP_FMT_DETECT (the layout of test_full_size_batches_match_the_oracle)."""
    import compu_amd
    from bench_support import synth

    n = 65536
    threads = min(32, len(os.sched_getaffinity(0)))
    pay = synth.payloads(n, threads=threads)
    packed, offs, lens = synth.mixed_units(pay, n, threads=threads)
    del pay
    is_gz = packed[offs.astype(np.int64)] == 0x1F
    assert n // 3 < int(is_gz.sum()) < 2 * n // 3
    size = gpu.full((n,), POISON64, dtype=gpu.int64, device=DEV)
    used = gpu.full((n,), POISON32, dtype=gpu.int32, device=DEV)
    st = gpu.full((n,), POISON32, dtype=gpu.int32, device=DEV)
    d_len = gpu.from_numpy(lens.astype(np.int32)).to(DEV)
    compu_amd.decode_batch_sizes(0, gpu.from_numpy(packed).to(DEV), gpu.from_numpy(offs.astype(np.int64)).to(DEV), d_len, size, used, st)
    gpu.cuda.synchronize()
    assert bool((st == 2).all()) and bool((size == synth.UNIT).all()) and gpu.equal(used, d_len)


def test_damaged_zstd_frames_size_then_decode(gpu, alice):
    """>= 700 damaged zstd frames (bit flips and truncations over libzstd's output, as test_truncated_and_corrupt_frames_match_oracle
    makes them): the size pass, then chip_decode_batch with out_cap = out_size.  Rules 3 and 1, and a verdict other than CHIP_FINISHED
    is never followed by a finished decode."""
    import zstd_ref
    from test_zstd_gpu import oracle_zstd_batch

    z = zstd_ref.load()
    rnd = random.Random(41)
    parts, ns = [], []
    for it in range(900):
        n = rnd.choice([50, 500, 5000, 70000, 140000])
        data = _mk(rnd.choice([1, 2, 4, 0]), n, rnd, alice)
        comp = bytearray(zstd_ref.compress(z, data, rnd.choice([1, 3, 9]), rnd.random() < 0.7, rnd.random() < 0.6))
        mode = rnd.randrange(3)
        if mode == 0:
            comp[rnd.randrange(len(comp))] ^= 1 << rnd.randrange(8)
        elif mode == 1:
            comp = comp[: rnd.randrange(len(comp))]
        parts.append(bytes(comp))
        ns.append(n)
    size, used, st = run_sizes(gpu, 100, parts)
    assert (size < (1 << 31)).all()
    ample = [max(int(s), n) + 4096 for s, n in zip(size, ns)]
    _o, e_ol, e_iu, e_st = run_batch(gpu, 100, parts, [max(int(s), 1) for s in size], check_tail=False)
    _o, a_ol, a_iu, a_st = run_batch(gpu, 100, parts, ample, check_tail=False)
    ref = oracle_zstd_batch(parts, ample)
    rule4 = 0
    for j in range(len(parts)):
        where = (j, int(st[j]), int(size[j]), int(used[j]), int(e_st[j]), int(e_ol[j]), int(a_st[j]), int(a_ol[j]), int(a_iu[j]), ref[j][2], len(ref[j][0]))
        if int(st[j]) == 2:
            assert int(e_st[j]) != 1 or int(size[j]) == 0, where  # rule 3 (a unit of size 0 was given one byte of room)
            if int(a_st[j]) != 2:
                rule4 += 1
                assert int(a_st[j]) < 0 and int(e_st[j]) == int(a_st[j]), where
        else:
            assert int(e_st[j]) != 2 and int(a_st[j]) != 2, where
        if int(a_st[j]) == 2:  # rule 1
            assert (int(st[j]), int(size[j]), int(used[j])) == (2, int(a_ol[j]), int(a_iu[j])), where
            assert ref[j][2] == 2 and len(ref[j][0]) == int(a_ol[j]), where
    print(f"rule 4 (finished here, an error in the decode): {rule4} of {len(parts)} frames")


def _decode_same(torch, fmt, parts, caps):
    outs, ol, iu, st = run_batch(torch, fmt, parts, caps)
    return ol, iu, st


def test_generated_payloads_match_the_decode(gpu, alice):
    """Rule 1: whatever chip_decode_batch finishes, the size pass finishes with the same length and input count -- system zlib at
    levels 1, 6, 9 as raw / zlib / gzip streams, this library's encoders, sizes 0 .. 400 000 and a few multi-megabyte
    multi-block units (one of them stored blocks only, one a run that decodes to 1000 times its input)."""
    import compu_amd
    from bench_support import synth

    rnd = random.Random(23)
    pay = synth.payloads(8).tobytes()  # 512 KiB of the benchmark's payload
    sizes = [0, 1, 2, 3, 17, 64, 257, 258, 259, 1000, 4095, 32767, 32768, 32769, 65535, 65536, 65537, 100000, 250000, 400000]
    for fmt, wbits in ((-15, -15), (15, 15), (31, 31), (47, 15), (47, 31)):
        parts, want = [], []
        for n in sizes:
            for level in (1, 6, 9):
                s = rnd.randrange(0, len(pay) - n + 1)
                data = pay[s : s + n] if rnd.random() < 0.7 else _mk(rnd.choice([1, 2, 3, 4]), n, rnd, alice * 3)
                co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, rnd.choice([0, 0, 4]))
                parts.append(co.compress(data) + co.flush() + (b"tail" if rnd.random() < 0.2 else b""))
                want.append(len(data))
        if fmt == -15:
            big = [pay * 6, os.urandom(3 << 20), b"\0" * (40 << 20), (alice * 30)[: 5 << 20]]
            for k, data in enumerate(big):
                co = zlib.compressobj([6, 0, 9, 1][k], zlib.DEFLATED, -15)
                parts.append(co.compress(data) + co.flush())
                want.append(len(data))
        size, used, st = run_sizes(gpu, fmt, parts)
        ol, iu, dst = _decode_same(gpu, fmt, parts, want)
        for j in range(len(parts)):
            where = (fmt, j, int(st[j]), int(size[j]), int(used[j]), int(dst[j]), int(ol[j]), int(iu[j]), want[j])
            assert int(dst[j]) == 2 and int(ol[j]) == want[j], where
            assert (int(st[j]), int(size[j]), int(used[j])) == (2, int(ol[j]), int(iu[j])), where
    # this library's encoders: every level group, every wrapper
    n = 96
    upay = synth.payloads(n)
    lens_in = np.array([rnd.choice([0, 1, 100, 5000, 65536]) for _ in range(n)], np.int32)
    d_pay = gpu.from_numpy(upay).to(DEV)
    offs = gpu.arange(n, dtype=gpu.int64, device=DEV) * synth.UNIT
    for fmt in (-15, 15, 31):
        for level in (0, 1, 3, 6, 9):
            bound = int(compu_amd.encode_bound(fmt, synth.UNIT)) + 64
            bound = (bound + 15) & ~15
            d_comp = gpu.zeros(n * bound, dtype=gpu.uint8, device=DEV)
            coff = gpu.arange(n, dtype=gpu.int64, device=DEV) * bound
            clen, est = compu_amd.encode_batch(fmt, level, d_pay, offs, gpu.from_numpy(lens_in).to(DEV), d_comp, coff,
                                               gpu.full((n,), bound, dtype=gpu.int32, device=DEV))
            gpu.cuda.synchronize()
            assert bool((est == 2).all())
            size = gpu.full((n,), POISON64, dtype=gpu.int64, device=DEV)
            s_used, s_st = gpu.zeros(n, dtype=gpu.int32, device=DEV), gpu.zeros(n, dtype=gpu.int32, device=DEV)
            compu_amd.decode_batch_sizes(fmt, d_comp, coff, clen, size, s_used, s_st)
            d_out = gpu.zeros(n * synth.UNIT, dtype=gpu.uint8, device=DEV)
            ol, iu, dst = compu_amd.decode_batch(fmt, d_comp, coff, clen, d_out, offs, gpu.full((n,), synth.UNIT, dtype=gpu.int32, device=DEV))
            gpu.cuda.synchronize()
            assert bool((dst == 2).all()) and bool((ol == gpu.from_numpy(lens_in).to(DEV)).all()), (fmt, level)
            assert bool((s_st == 2).all()) and gpu.equal(size, ol.to(gpu.int64)) and gpu.equal(s_used, iu), (fmt, level)


@pytest.mark.timeout(1500)
def test_full_launch_size_dynamic(gpu):
    """65 536 dynamic-Huffman units x 64 KiB (the benchmark's launch size, as test_full_size_batches_match_the_oracle builds it):
    every unit finishes with 65 536 bytes and its whole input, on a stream that has never decoded (the size pass allocates the
    scratch slot itself)."""
    import compu_amd
    from bench_support import synth

    n = 65536
    threads = min(32, len(os.sched_getaffinity(0)))
    pay = synth.payloads(n, threads=threads)
    packed, offs, lens = synth.deflate_units(pay, n, kind="dynamic", threads=threads)
    del pay
    compu_amd.trim()
    size = gpu.full((n,), POISON64, dtype=gpu.int64, device=DEV)
    used = gpu.full((n,), POISON32, dtype=gpu.int32, device=DEV)
    st = gpu.full((n,), POISON32, dtype=gpu.int32, device=DEV)
    d_len = gpu.from_numpy(lens.astype(np.int32)).to(DEV)
    compu_amd.decode_batch_sizes(-15, gpu.from_numpy(packed).to(DEV), gpu.from_numpy(offs.astype(np.int64)).to(DEV), d_len, size, used, st)
    gpu.cuda.synchronize()
    assert bool((st == 2).all()) and bool((size == synth.UNIT).all()) and gpu.equal(used, d_len)


def _damaged(rnd, alice, count):
    """bit flips, truncations and trailing bytes over zlib's output, as test_truncated_corrupt_and_small_caps_match_oracle makes them"""
    parts, ns = [], []
    for it in range(count):
        n = rnd.choice([50, 500, 5000, 30000, 70000])
        data = _mk(rnd.choice([1, 2, 4]), n, rnd, alice)
        wbits = rnd.choice([-15, -15, 15, 31])
        co = zlib.compressobj(rnd.choice([0, 1, 6, 9]), zlib.DEFLATED, wbits, 8, rnd.choice([0, 4]))
        comp = bytearray(co.compress(data) + co.flush())
        mode = rnd.randrange(4)
        if mode in (0, 3):
            for _ in range(1 if mode == 0 else 3):
                comp[rnd.randrange(len(comp))] ^= 1 << rnd.randrange(8)
        elif mode == 1:
            comp = comp[: rnd.randrange(len(comp))]
        else:
            comp += rnd.randbytes(rnd.randrange(1, 9))
        parts.append((wbits, bytes(comp)))
        ns.append(n)
    return parts, ns


def test_damaged_streams_size_then_decode(gpu, alice):
    """>= 700 damaged DEFLATE streams: the size pass, then chip_decode_batch with out_cap = out_size.  Rule 3 (never
    CHIP_NEED_OUTPUT behind a CHIP_FINISHED), rule 1 against a decode with ample room, a verdict other than CHIP_FINISHED is never
    followed by a finished decode, and the verdict and length are the oracle's wherever the fault is not the check value."""
    rnd = random.Random(77)
    units, ns = _damaged(rnd, alice, 900)
    rule4 = total = 0
    for fmt in (-15, 15, 31):
        idx = [i for i, (w, _) in enumerate(units) if w == fmt]
        parts = [units[i][1] for i in idx]
        size, used, st = run_sizes(gpu, fmt, parts)
        assert (size < (1 << 31)).all()  # nothing in this corpus is beyond a 32-bit capacity
        exact = [int(s) for s in size]
        ample = [max(int(s), ns[i]) + 1024 for s, i in zip(size, idx)]
        e_ol, e_iu, e_st = _decode_same(gpu, fmt, parts, exact)
        a_ol, a_iu, a_st = _decode_same(gpu, fmt, parts, ample)
        ref = oracle_batch(fmt, parts, ample)
        for j in range(len(parts)):
            where = (fmt, j, int(st[j]), int(size[j]), int(used[j]), int(e_st[j]), int(e_ol[j]), int(a_st[j]), int(a_ol[j]), int(a_iu[j]), ref[j][2], len(ref[j][0]))
            total += 1
            assert int(a_st[j]) != 1, where  # (the ample room was ample)
            if int(st[j]) == 2:
                assert int(e_st[j]) != 1, where                                  # rule 3
                assert int(e_st[j]) == int(a_st[j]) and int(e_ol[j]) == int(a_ol[j]), where
                if int(a_st[j]) != 2:                                            # rule 4: only the check value can be wrong
                    rule4 += 1
                    assert int(a_st[j]) == -3 and int(a_ol[j]) == int(size[j]) and fmt != -15, where
            else:
                assert int(e_st[j]) != 2 and int(a_st[j]) != 2, where
                assert (int(st[j]), int(size[j]), int(used[j])) == (int(a_st[j]), int(a_ol[j]), int(a_iu[j])), where  # rule 2
            if int(a_st[j]) == 2:                                                # rule 1
                assert (int(st[j]), int(size[j]), int(used[j])) == (2, int(a_ol[j]), int(a_iu[j])), where
            if len(parts[j]):  # (an empty unit is CHIP_NEED_INPUT to the batch calls, Z_BUF_ERROR to zlib)
                assert int(a_st[j]) == ref[j][2] and int(a_ol[j]) == len(ref[j][0]), where
    assert total >= 700
    print(f"rule 4 (finished here, data check fails in the decode): {rule4} of {total} units")


def test_no_memory_per_unit_and_every_entry_written(gpu):
    """A second size pass of the same size on the same stream takes no device memory (hipMemGetInfo differs by 0): the pass owns
    nothing but the per-wave scratch slot of (device, stream)."""
    import compu_amd
    from bench_support import synth

    n = 4096
    pay = synth.payloads(n)
    packed, offs, lens = synth.deflate_units(pay, n, kind="dynamic")
    d_in = gpu.from_numpy(packed).to(DEV)
    d_off, d_len = gpu.from_numpy(offs.astype(np.int64)).to(DEV), gpu.from_numpy(lens.astype(np.int32)).to(DEV)
    res = [(gpu.full((n,), POISON64, dtype=gpu.int64, device=DEV), gpu.full((n,), POISON32, dtype=gpu.int32, device=DEV),
            gpu.full((n,), POISON32, dtype=gpu.int32, device=DEV)) for _ in range(2)]
    compu_amd.decode_batch_sizes(-15, d_in, d_off, d_len, *res[0])
    gpu.cuda.synchronize()
    free0 = gpu.cuda.mem_get_info()[0]
    compu_amd.decode_batch_sizes(-15, d_in, d_off, d_len, *res[1])
    gpu.cuda.synchronize()
    assert gpu.cuda.mem_get_info()[0] - free0 == 0
    for size, used, st in res:
        assert bool((st == 2).all()) and bool((size == synth.UNIT).all()) and gpu.equal(used, d_len)


@pytest.mark.parametrize("fmt", [-15, 0])
def test_size_pass_and_decode_from_two_host_threads_on_one_stream(gpu, fmt):
    """One host thread sizes, one decodes, same stream, batches of different sizes, starting from no scratch at all: both use the
    token scratch slot of (device, stream) -- and, routed (fmt 0, the shape of
    test_concurrent_routed_batches_of_different_sizes_on_one_stream), its index lists and counters -- so slot lookup (and growth),
    counter reset, router and launches are one critical section."""
    import compu_amd
    from bench_support import synth

    sizes = [320, 1100]
    jobs = []
    for k, n in enumerate(sizes):
        pay = synth.payloads(n, first_unit=1000 * k)
        if fmt == 0:
            packed, offs, lens = synth.mixed_units(pay, n, first_unit=1000 * k)
        else:
            packed, offs, lens = synth.deflate_units(pay, n, kind="dynamic")
        jobs.append(dict(n=n, want=gpu.from_numpy(pay).to(DEV), d_in=gpu.from_numpy(packed).to(DEV), d_off=gpu.from_numpy(offs.astype(np.int64)).to(DEV),
                         d_len=gpu.from_numpy(lens.astype(np.int32)).to(DEV), ooff=gpu.arange(n, dtype=gpu.int64, device=DEV) * 65536,
                         caps=gpu.full((n,), 65536, dtype=gpu.int32, device=DEV), out=gpu.zeros(n * 65536, dtype=gpu.uint8, device=DEV)))
    res = [None, None]

    def size_work():
        j = jobs[1]
        for _ in range(25):
            res[0] = compu_amd.decode_batch_sizes(fmt, j["d_in"], j["d_off"], j["d_len"])

    def decode_work():
        j = jobs[0]
        for _ in range(25):
            res[1] = compu_amd.decode_batch(fmt, j["d_in"], j["d_off"], j["d_len"], j["out"], j["ooff"], j["caps"])

    compu_amd.trim()
    ts = [threading.Thread(target=size_work), threading.Thread(target=decode_work)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    gpu.cuda.synchronize()
    size, used, st = res[0]
    assert bool((st == 2).all()) and bool((size == 65536).all()) and gpu.equal(used, jobs[1]["d_len"])
    ol, iu, st = res[1]
    assert bool((st == 2).all()) and bool((ol == 65536).all()) and gpu.equal(iu, jobs[0]["d_len"])
    assert gpu.equal(jobs[0]["out"], jobs[0]["want"])
