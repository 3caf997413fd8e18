"""chip_inflate_parallel_next without a GPU: the argument refusals, which answer before a device is looked for, and the condition the
GPU tests rely on -- for the listed inputs and slabs the model of tests/inflate_stream_ref.py finishes with every call on the
parallel path, and the finder names only true block boundaries in every slab (so the chain of each call is the model's)."""
import ctypes as C

import pytest

import inflate_parallel_ref as R
import inflate_stream_cases as SC
import inflate_stream_ref as SR


def test_argument_refusals_need_no_device():
    import compu_amd
    from compu_amd.api import _InflateCursor, _InflateNextSummary

    call = compu_amd.lib().chip_inflate_parallel_next
    cur, summ = _InflateCursor(), _InflateNextSummary()
    p = C.c_void_p(4096)  # never read: every call below is refused at its arguments
    good = [31, C.byref(cur), p, p, 1000, p, 1000, 0, C.byref(summ), None]

    def refused(k, v):
        a = list(good)
        a[k] = v
        return call(*a)

    assert refused(0, 12345) == -101 and refused(0, 0) == -101 and refused(0, 100) == -101  # a format that is none of the four
    assert refused(4, (1 << 29) - 63) == -101  # len above CHIP_GZPLAN_WINDOW
    assert refused(6, 0xFFFFFFF1) == -101  # out_cap above 2^32 - 16
    assert refused(1, None) == -101 and refused(2, None) == -101 and refused(8, None) == -101  # cursor, window, summary
    assert refused(3, None) == -101 and refused(5, None) == -101  # a NULL buffer with a length
    assert refused(7, 255) == -101 and refused(7, (1 << 29) - 63) == -101  # chunk_bytes out of range
    for field, v in (("bit", 8), ("phase", 5), ("wrap", 3), ("hist", 1)):  # a cursor no call has left
        bad = _InflateCursor()
        setattr(bad, field, v)
        assert refused(1, C.byref(bad)) == -101, field
    assert (cur.in_total, cur.out_total, cur.phase) == (0, 0, 0)


def test_header_declares_the_cursor_and_the_summary():
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "compu_hip.h")).read()
    assert "CHIP_CUR_HEADER = 0, CHIP_CUR_BLOCKS = 1, CHIP_CUR_TRAILER = 2, CHIP_CUR_DONE = 3, CHIP_CUR_ERROR = 4" in text
    from compu_amd.api import _InflateCursor, _InflateNextSummary

    assert C.sizeof(_InflateCursor) == 40 and C.sizeof(_InflateNextSummary) == 56


@pytest.mark.parametrize("name,fmt,data,first_bit,chunk_bytes,slabs", SC.parallel_inputs(), ids=[c[0] for c in SC.parallel_inputs()])
def test_every_call_of_the_listed_inputs_is_parallel(name, fmt, data, first_bit, chunk_bytes, slabs):
    bits, out_at, content = SR.boundaries(data, first_bit, SC.TRAILER[fmt])
    true = set(bits)
    for slab in slabs:
        calls, _ = SR.calls(data, first_bit, chunk_bytes, slab, trailer=SC.TRAILER[fmt])
        assert calls[-1].status == SR.FINISHED and sum(c.out_len for c in calls) == len(content)
        blocks = [c for c in calls if c.out_len or c.starts]
        assert all(c.path == SR.PARALLEL and len(c.starts) >= 2 for c in blocks), (slab, calls)
        for c in blocks:
            assert {s + 8 * c.pos for s in c.starts} <= true, (slab, c)  # no false start: links == the starts the chain can reach
            assert c.end in true
        print(name, slab, len(calls), "calls")


def test_the_serial_inputs_have_no_start_in_any_slab():
    for name, data, content, chunk_bytes, slabs in SC.serial_inputs():
        for slab in slabs:
            calls, walked = SR.calls(data, 0, chunk_bytes, slab)
            assert walked == content and calls[-1].status == SR.FINISHED
            assert all(not c.starts and c.path == SR.SERIAL for c in calls if name != "chunk-edges"), (name, slab)
            assert all(c.out_len > 0 or c.status == SR.FINISHED or c.slab < slab for c in calls), (name, slab, calls)


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """compu_amd/csrc/check_combine.h -- the combination of the check values and the cursor's arithmetic -- in a stand-alone program
    built with the address and undefined-behaviour sanitizers, against zlib"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_check_combine")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(root, "tests", "cpp", "test_check_combine.cpp"), "-lz"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test result: ok" in out.stdout, out.stdout + out.stderr
