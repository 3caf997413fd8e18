"""The block finder on the host (include/compu_hip.h, "one large stream: block starts"): chip_inflate_find_starts_host against the
Python restatement of the candidate rule (tests/inflate_parallel_ref.py) and against the true block boundaries of the inputs, and
the argument checks of both finder calls, which answer before a device is looked for.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import inflate_index_cases as IC
import inflate_parallel_cases as PC
import inflate_parallel_ref as R

E_INVALID = -101
GZPLAN_WINDOW = (1 << 29) - 64


def _host(data, first_bit, chunk_bytes, **kw):
    import compu_amd

    return compu_amd.inflate_find_starts_host(data, first_bit, chunk_bytes, **kw)


@pytest.mark.parametrize("chunk_bytes", PC.CHUNKS)
def test_host_finder_equals_the_reference(chunk_bytes):
    """counted and filled, on every input; a fill that is cut short keeps the first entries and touches nothing behind them"""
    for name, data, first_bit in PC.finder_inputs(chunk_bytes):
        want = R.find_starts(data, first_bit, chunk_bytes)
        starts, n = _host(data, first_bit, chunk_bytes)
        assert (n, starts.tolist()) == (len(want), want), name
        _, counted = _host(data, first_bit, chunk_bytes, max_starts=0)
        assert counted == len(want), name
        if len(want) >= 2:
            import compu_amd

            buf = np.frombuffer(data, np.uint8)
            part, n2 = np.full(len(want), 0xA5A5A5A5A5A5A5A5, np.uint64), C.c_uint64(0)
            rc = compu_amd.lib().chip_inflate_find_starts_host(buf.ctypes.data, buf.size, first_bit, chunk_bytes, len(want) - 1, part.ctypes.data,
                                                               C.byref(n2))
            assert rc == 0 and n2.value == len(want), name
            assert part[:-1].tolist() == want[:-1] and int(part[-1]) == 0xA5A5A5A5A5A5A5A5, name


@pytest.mark.parametrize("chunk_bytes", PC.CHUNKS)
def test_starts_of_a_file_are_its_real_boundaries(chunk_bytes):
    """alice29.txt at memLevel 2: every chunk that holds the boundary of a non-final dynamic block starts at the first of them, and
    no other position of the file is taken for a header; nearly every chunk has one"""
    for fmt in IC.WRAPPERS:
        data, first_bit = PC.alice(fmt)
        bounds, content = R.walk_cached(data, first_bit)
        assert content == IC.file_content("alice") and len(bounds) > 100
        want = R.true_starts(bounds, first_bit, chunk_bytes, len(data))
        starts, n = _host(data, first_bit, chunk_bytes)
        assert starts.tolist() == want, fmt
        n_chunks = -(-len(data) // chunk_bytes)
        assert n >= (n_chunks - 1) * 9 // 10, (fmt, n, n_chunks)


@pytest.mark.parametrize("chunk_bytes", PC.CHUNKS)
def test_boundaries_on_a_chunks_first_and_last_bit(chunk_bytes):
    s, (first, last) = PC.chunk_edges(chunk_bytes)
    starts, _ = _host(s.data, 0, chunk_bytes)
    assert starts.tolist() == [first, last]
    # starts lie behind first_bit: the stream's first block is never one
    assert _host(s.data, first, chunk_bytes)[0].tolist() == [last]


@pytest.mark.parametrize("chunk_bytes", PC.CHUNKS)
def test_header_cut_by_the_end_of_the_buffer(chunk_bytes):
    s, (first, last) = PC.chunk_edges(chunk_bytes)
    got = {name: _host(data, 0, chunk_bytes)[0].tolist() for name, data in PC.cut_header(chunk_bytes)}
    assert got == {"cut-in-header": [first], "cut-behind-header": [first, last], "cut-in-fields": [first]}


@pytest.mark.parametrize("chunk_bytes", PC.CHUNKS)
def test_decoy_is_a_start_and_no_boundary(chunk_bytes):
    """a candidate is not a promise: the stored payload that spells a header is its chunk's start"""
    s, at = PC.decoy(chunk_bytes)
    starts, _ = _host(s.data, 0, chunk_bytes)
    assert starts[0] == at and at not in [b[0] for b in s.blocks]
    real = [b for b, t, f, *_ in s.blocks if t == 2 and not f and b >= 16 * chunk_bytes]
    assert set(starts[1:].tolist()) <= set(real)


def test_fixed_stored_and_final_blocks_are_no_candidates():
    s = IC.phases("raw")
    starts, _ = _host(s.data, 0, 256)
    dynamic = {b for b, t, f, *_ in s.blocks if t == 2 and not f}
    assert set(starts.tolist()) <= dynamic and len(starts) >= 2
    for b, t, f, *_ in s.blocks:
        assert R.is_candidate(s.data, b) == (t == 2 and not f), (b, t, f)


def test_parallel_refusals_need_no_device():
    import compu_amd
    from compu_amd.api import _InflateParallelSummary

    lib = compu_amd.lib()
    raw = _InflateParallelSummary()
    s, p, arr = C.byref(raw), 0x1000, 0x2000  # (addresses that are only looked at: a refusal comes before any device)
    call = lib.chip_inflate_parallel
    assert call(12345, p, 100, p, 100, 0, 0, None, None, None, None, s, None) == E_INVALID          # a format that is none of the four
    assert call(31, p, 100, p, 100, 0, 0, None, None, None, None, None, None) == E_INVALID          # no summary
    assert call(31, None, 100, p, 100, 0, 0, None, None, None, None, s, None) == E_INVALID          # no input
    assert call(31, p + 2, 100, p, 100, 0, 0, None, None, None, None, s, None) == E_INVALID         # input not 4-byte aligned
    assert call(31, p, 100, None, 100, 0, 0, None, None, None, None, s, None) == E_INVALID          # room without a buffer
    assert call(31, p, GZPLAN_WINDOW + 1, p, 100, 0, 0, None, None, None, None, s, None) == E_INVALID
    assert call(31, p, 100, p, (1 << 32) - 15, 0, 0, None, None, None, None, s, None) == E_INVALID  # room above 2^32 - 16
    for missing in range(4):                                                                        # a null array with max_points > 0
        arrays = [arr, arr, arr, arr]
        arrays[missing] = None
        assert call(31, p, 100, p, 100, 0, 1, *arrays, s, None) == E_INVALID
    for chunk in (1, 255, GZPLAN_WINDOW + 1):
        assert call(31, p, 100, p, 100, chunk, 0, None, None, None, None, s, None) == E_INVALID


def test_refusals_need_no_device():
    import compu_amd

    lib = compu_amd.lib()
    buf = np.zeros(4096, np.uint8)
    out, n = np.zeros(8, np.uint64), C.c_uint64(0)
    p, o, nn = buf.ctypes.data, out.ctypes.data, C.byref(n)
    for host in (True, False):
        def call(*a):
            return lib.chip_inflate_find_starts_host(*a) if host else lib.chip_inflate_find_starts(*a, None)

        assert call(p, 4096, 0, 512, 8, o, None) == E_INVALID                    # n NULL
        assert call(None, 4096, 0, 512, 8, o, nn) == E_INVALID                   # no buffer
        assert call(p, 4096, 0, 512, 8, None, nn) == E_INVALID                   # no array for max > 0
        assert call(p, 4096, 0, 255, 8, o, nn) == E_INVALID                      # chunk_bytes below 256
        assert call(p, 4096, 0, 0, 8, o, nn) == E_INVALID
        assert call(p, 4096, 0, GZPLAN_WINDOW + 1, 8, o, nn) == E_INVALID        # chunk_bytes above a unit's limit
        assert call(p, GZPLAN_WINDOW + 1, 0, 512, 8, o, nn) == E_INVALID         # len above a unit's limit
        assert call(p, 4096, 8 * 4096 + 1, 512, 8, o, nn) == E_INVALID           # first_bit behind the buffer
    # what is fine: an empty buffer, a buffer of one chunk, counting with null arrays
    n.value = 7
    assert lib.chip_inflate_find_starts_host(None, 0, 0, 512, 0, None, nn) == 0 and n.value == 0
    n.value = 7
    assert lib.chip_inflate_find_starts_host(p, 512, 0, 512, 0, None, nn) == 0 and n.value == 0
    n.value = 7
    assert lib.chip_inflate_find_starts(p, 512, 0, 512, 0, None, nn, None) == 0 and n.value == 0  # one chunk: no launch
