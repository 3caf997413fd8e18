"""The zstd encoder core (compu_amd/csrc/zstd_enc_core.h) without a GPU: built for the host (tests/zstd_enc_host.py) and run on the
built inputs of tests/zstd_enc_cases.py.  Every frame decodes with the system libzstd and the oracle, the frame reader proves that
each input reaches the threshold it was built for, streams of several segments decode under the window they declare, and room that
is exactly enough is enough while one byte less is not."""
import pytest

import zstd_enc_cases as K
import zstd_enc_host as H
import zstd_frame_reader as R
from zstd_decoders import oracle_decode as _oracle_decode, zdec as _zdec

SETTINGS = [(0, 8), (0, 2), (1, 8), (2, 8), (3, 8)]  # (group, skip_shift): skip_shift only matters in group 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return H.build_driver(str(tmp_path_factory.mktemp("zenc")))


def test_mirrors_of_the_api():
    assert H.group_of(-7) == (0, 2) and H.group_of(-3) == (0, 5) and H.group_of(1) == (0, 8) and H.group_of(0) == (1, 8)
    assert H.group_of(3) == (1, 8) and H.group_of(6) == (2, 8) and H.group_of(12) == (2, 8) and H.group_of(13) == (3, 8)
    assert H.group_of(19) == (3, 8) and H.group_of(40) == (3, 8) and H.group_of(3, 1) == (0, 8) and H.group_of(1, 6) == (3, 8)
    assert H.group_of(-9, 4) == (2, 2)
    assert H.batch_params() == (27, 27, True) and H.stream_params(10) == (10, 10, True) and H.stream_params(31) == (27, 20, True)
    M = H.SEGMENT
    a = bytes(M + 5)
    assert [len(s) for s in H.segments_of([(a, H.FINISH)])] == [M, 5]
    assert [len(s) for s in H.segments_of([(a[:M], H.FINISH)])] == [M]
    assert [len(s) for s in H.segments_of([(a[:M], H.PROCESS), (b"", H.FINISH)])] == [M, 0]
    assert [len(s) for s in H.segments_of([(a[:M], H.FLUSH), (b"", H.FLUSH), (b"x", H.FINISH)])] == [M, 1]
    assert [len(s) for s in H.segments_of([(b"", H.FLUSH), (b"", H.FLUSH), (b"", H.FINISH)])] == [0, 0]
    assert [len(s) for s in H.segments_of([(a[:M - 1], H.PROCESS), (a[:3], H.PROCESS), (b"", H.FINISH)])] == [M, 2]


@pytest.mark.parametrize("group,skip_shift", SETTINGS)
def test_built_cases_decode_and_reach_their_thresholds(driver, group, skip_shift):
    cases = [c for c in K.all_cases() if K.holds_in(c[2], group, skip_shift)]
    assert len(cases) > 60
    datas = [c[1] for c in cases]
    frames = H.encode(driver, group, skip_shift, *H.batch_params(), datas)
    assert all(f is not None for f in frames)
    assert _oracle_decode(frames, [len(d) for d in datas]) == datas
    for (name, data, _groups, condition), f in zip(cases, frames):
        assert _zdec(f, len(data)) == data, name
        info = R.read_frame(f)
        assert info["content"] == data and info["checksum"], name
        assert condition(info), f"{name} no longer reaches its threshold in group {group}: {_brief(info)}"


def _brief(info):
    keys = ("type", "size", "lit_type", "size_format", "lit_regen", "lit_comp", "streams", "tree", "n_weights", "longest_code", "nseq",
            "nseq_bytes", "modes")
    return [{k: b[k] for k in keys if k in b} for b in info["blocks"]][:4]


def test_case_names_are_unique_and_inputs_small():
    names = [c[0] for c in K.all_cases()]
    assert len(set(names)) == len(names)
    assert all(len(c[1]) <= 400000 and c[2] for c in K.all_cases())


@pytest.mark.parametrize("window_log", [10, 17, 20, 27])
def test_streams_of_segments_decode_under_their_window(driver, window_log):
    params = H.stream_params(window_log)
    for group, skip_shift in SETTINGS:
        # the scripts of a MiB in one group only: the reader takes seconds on them
        scripts = [(n, s) for n, s in K.stream_scripts() if group == 2 or sum(len(p) for p, _op in s) < 450000]
        jobs = [H.segments_of(s) for _name, s in scripts]
        frames = H.encode(driver, group, skip_shift, *params, jobs)
        for (name, _s), segs, f in zip(scripts, jobs, frames):
            data = b"".join(segs)
            assert f is not None, name
            assert _zdec(f, len(data), window_log_max=max(10, min(window_log, 20))) == data, (name, group)
            info = R.read_frame(f)
            assert info["content"] == data, (name, group)
            oneshot = len(segs) == 1 and len(data) <= 1 << min(window_log, 27)
            assert info["single"] == oneshot, (name, group)
            if not oneshot:
                assert info["window_log"] == min(window_log, 20) and info["fcs"] is None, (name, group)
                assert all(b["regen"] <= 1 << min(window_log, 17) for b in info["blocks"]), (name, group)
                offs = [o for b in info["blocks"] for o in b.get("offsets", [])]
                assert all(o <= 1 << min(window_log, 20) for o in offs), (name, group)


ROOM_CASES = ["nseq_full_block", "nseq_32512", "ml_full_block_and_more", "zeros_131073", "one_zeros_131072", "permutations_8192",
              "permutations_512_and_copy", "depth_expo", "weights_129_fse", "lit_raw_4096_chunked", "lit_1025_chunked", "lit_16384_chunked", "lit_rle_4096",
              "repeat_codes", "raw_block_between_repeat_codes", "tiny_0", "tiny_1", "tiny_15", "fcs_256"]


@pytest.mark.parametrize("group", [0, 2])
def test_exact_room_is_enough_and_one_byte_less_is_not(driver, group):
    by_name = {c[0]: c[1] for c in K.all_cases()}
    datas = [by_name[n] for n in ROOM_CASES]
    full = H.encode(driver, group, 8, *H.batch_params(), datas)
    jobs, caps = [], []
    for d, f in zip(datas, full):
        jobs += [d, d, d]
        caps += [len(f), len(f) - 1, len(f) // 2]
    got = H.encode(driver, group, 8, *H.batch_params(), jobs, caps)  # asserts the canary behind every capacity
    for i, (name, f) in enumerate(zip(ROOM_CASES, full)):
        assert got[3 * i] == f, name
        assert got[3 * i + 1] is None and got[3 * i + 2] is None, name
