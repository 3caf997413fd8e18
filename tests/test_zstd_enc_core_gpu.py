"""The zstd encoder kernel against its host core, byte for byte.  zstd_enc_core.h says that encode_segment_wave (zstd_enc.hip) is the
kernel form of zenc::compress_segment, "same steps, same bytes": tests/zstd_enc_host.py builds the host form of encode_unit with g++,
and these tests hold the kernel's frames against it -- on the built inputs of tests/zstd_enc_cases.py (each proven by the frame
reader to reach its threshold, on the kernel's frame too), on the generated corpus of test_zstd_encoder_gpu.py, on 256 copies of one
unit in one launch, with room that is exactly enough, and through the streaming encoder.  A kernel fault that still yields a valid
frame (a missing barrier, a stale repeat offset, a lost histogram count) changes the bytes and fails here."""
import random

import pytest

import zstd_enc_cases as K
import zstd_enc_host as H
import zstd_frame_reader as R
from test_inflate_gpu import _mk
from test_zstd_encoder_gpu import SIZES, _batch, _gpu_decode
from zstd_decoders import oracle_decode as _oracle_decode, zdec as _zdec

pytestmark = pytest.mark.gpu
BLOCK = 128 << 10


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return H.build_driver(str(tmp_path_factory.mktemp("zenc")))


def _differences(names, kernel, host, group):
    return [f"{n} (group {group}): {R.first_difference(k, h)}" for n, k, h in zip(names, kernel, host) if k != h]


# levels -7 .. 19 with the default strategy: groups 0 (skip_shift 2, 5, 8), 1, 2, 3; then Fast and BtLazy2 by name
@pytest.mark.parametrize("level,strategy", [(-7, 0), (-3, 0), (1, 0), (3, 0), (6, 0), (19, 0), (3, 1), (1, 6)])
def test_kernel_equals_host_core_on_the_built_cases(gpu, driver, level, strategy):
    cases = K.all_cases()
    names, datas = [c[0] for c in cases], [c[1] for c in cases]
    group, skip_shift = H.group_of(level, strategy)
    assert group == {(-7, 0): 0, (-3, 0): 0, (1, 0): 0, (3, 0): 1, (6, 0): 2, (19, 0): 3, (3, 1): 0, (1, 6): 3}[(level, strategy)]
    frames, st = _batch(gpu, datas, level, strategy)
    assert (st == 2).all(), [n for n, s in zip(names, st) if s != 2]
    host = H.encode_level(driver, level, strategy, datas)
    sizes = [len(d) for d in datas]
    # every decoder first: a frame that is damaged is reported as that, not as a difference
    for n, f, d in zip(names, frames, datas):
        assert _zdec(f, len(d)) == d, n
    assert _oracle_decode(frames, sizes) == datas
    assert _gpu_decode(gpu, frames, sizes) == datas
    diff = _differences(names, frames, host, group)
    assert not diff, "\n".join(diff)
    for (name, data, groups, condition), f in zip(cases, frames):
        if K.holds_in(groups, group, skip_shift):
            info = R.read_frame(f)
            assert info["content"] == data and condition(info), f"{name} does not reach its threshold in the kernel's frame (group {group})"


_CORPUS = []


def _corpus(alice):
    if not _CORPUS:
        rnd = random.Random(21)
        _CORPUS.extend((f"kind {kind}, {n} bytes", _mk(kind, n, rnd, alice)) for kind in range(5) for n in SIZES)
    return _CORPUS


@pytest.mark.parametrize("level", [-7, 1, 3, 6, 19])
def test_kernel_equals_host_core_on_the_generated_corpus(gpu, driver, alice, level):
    names, datas = zip(*_corpus(alice))
    frames, st = _batch(gpu, list(datas), level)
    assert (st == 2).all()
    host = H.encode_level(driver, level, 0, list(datas))
    diff = _differences(names, frames, host, H.group_of(level)[0])
    assert not diff, "\n".join(diff)


@pytest.mark.parametrize("case,level", [("nseq_full_block", 1), ("depth_alice", 6), ("depth_alice", 19)])
def test_the_same_unit_256_times(gpu, driver, case, level):
    """256 waves encode the same block side by side: a race shows as a copy that differs"""
    data = next(c[1] for c in K.all_cases() if c[0] == case)
    assert len(data) == BLOCK
    frames, st = _batch(gpu, [data] * 256, level)
    assert (st == 2).all()
    host, = H.encode_level(driver, level, 0, [data])
    odd = [i for i, f in enumerate(frames) if f != host]
    assert not odd, f"copies {odd[:8]} of {case} differ from the host core: {R.first_difference(frames[odd[0]], host)}"


def test_exact_room(gpu):
    """room of exactly the frame's length finishes with the same bytes; one byte less, or half, is NeedOutput with nothing written
    past the capacity (the 0xA5 canary of _batch) and no length reported"""
    cases = K.all_cases()
    names, datas = [c[0] for c in cases], [c[1] for c in cases]
    for level in (3, 6):
        full, st = _batch(gpu, datas, level)
        assert (st == 2).all()
        jobs, caps = [], []
        for d, f in zip(datas, full):
            jobs += [d, d, d]
            caps += [len(f), len(f) - 1, len(f) // 2]
        frames, st, out_len = _batch(gpu, jobs, level, caps=caps, with_len=True)
        for i, (n, f) in enumerate(zip(names, full)):
            assert st[3 * i] == 2 and frames[3 * i] == f, (n, level)
            assert st[3 * i + 1] == 1 and st[3 * i + 2] == 1, (n, level, st[3 * i:3 * i + 3])
            assert out_len[3 * i + 1] == 0 and out_len[3 * i + 2] == 0, (n, level)


def _run_script(c, enc, script):
    """the calls of `script` with ample room -> the bytes delivered"""
    ops = {H.PROCESS: c.EncodeOp.Process, H.FLUSH: c.EncodeOp.Flush, H.FINISH: c.EncodeOp.Finish}
    out = bytearray()
    for i, (piece, op) in enumerate(script):
        room = len(piece) + (3 << 20)
        buf = bytearray(room)
        r = enc.encode(piece, buf, ops[op], 0, room)
        assert r.input_remain == 0 and r.output_remain > 0
        assert r.status == (c.EncodeStatus.Finished if op == H.FINISH else c.EncodeStatus.Continue), (i, r.status)
        out += buf[: room - r.output_remain]
    return bytes(out)


@pytest.mark.parametrize("window_log", [10, 17, 27])
def test_streaming_equals_host_core(gpu, driver, window_log):
    import compu_amd as c

    for level, strategy in ((3, 0), (-7, 0), (12, 0), (3, 7)):
        # the scripts of a MiB (the segment cut) run under the default window only; the small ones at every setting; at level 3
        # every script runs again after reset()
        big = level == 3 and window_log == 27
        scripts = [(n, s) for n, s in K.stream_scripts() if big or sum(len(p) for p, _op in s) < 450000]
        jobs = [H.segments_of(s) for _n, s in scripts]
        host = H.encode_level(driver, level, strategy, jobs, params=H.stream_params(window_log))
        enc = c.encoder_interface.zstd_hip(c.ZstdEncoderOptions().level(level).strategy(strategy).window_log(window_log))
        for (name, script), segs, h in zip(scripts, jobs, host):
            got = _run_script(c, enc, script)
            data = b"".join(segs)
            assert _zdec(got, len(data), window_log_max=max(10, min(window_log, 20))) == data, (name, level)
            where = f"{name}, level {level}, strategy {strategy}, window_log {window_log}"
            assert got == h, f"{where}: {R.first_difference(got, h) if len(data) < 450000 else 'frames differ'}"
            enc.reset()
            if level == 3:
                assert _run_script(c, enc, script) == h, f"{where}: after reset()"
                enc.reset()
        enc.close()
