"""The block finder on the device: chip_inflate_find_starts answers what chip_inflate_find_starts_host answers (which
tests/test_inflate_parallel_cpu.py holds against the definition), counted, filled and cut short, from one chunk to thousands."""
import numpy as np
import pytest
import torch

import compu_amd
import inflate_index_cases as IC
import inflate_parallel_cases as PC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A


def _device(data, pad=0):
    """the bytes at offset `pad` of a device tensor, some bytes of another value behind them"""
    t = torch.full((pad + len(data) + 64,), 0x24, dtype=torch.uint8, device="cuda")  # 0x24 = 00100100: candidates' first bits
    t[pad:pad + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t[pad:]


def _filled(buf, length, first_bit, chunk_bytes, room, ask):
    """chip_inflate_find_starts into a poisoned array of `room` entries with max = ask -> (array, n)"""
    import ctypes as C

    starts = torch.full((room,), POISON, dtype=torch.int64, device="cuda")
    n = C.c_uint64(0)
    rc = compu_amd.lib().chip_inflate_find_starts(buf.data_ptr(), length, first_bit, chunk_bytes, ask, starts.data_ptr(), C.byref(n), None)
    assert rc == 0
    return starts.cpu().numpy().astype(np.uint64), n.value


@pytest.mark.parametrize("chunk_bytes", PC.CHUNKS)
def test_device_finder_equals_the_host_finder(chunk_bytes):
    for name, data, first_bit in PC.finder_inputs(chunk_bytes):
        want, n = compu_amd.inflate_find_starts_host(data, first_bit, chunk_bytes)
        buf = _device(data, pad=3 if name.startswith("phases") else 0)  # (no alignment is asked of the buffer)
        got, gn = compu_amd.inflate_find_starts(buf, len(data), first_bit, chunk_bytes)
        assert gn == n and got.cpu().numpy().astype(np.uint64).tolist() == want.tolist(), name
        # counted with null arrays; filled with room to spare and cut short: nothing behind the answer is touched
        assert compu_amd.inflate_find_starts(buf, len(data), first_bit, chunk_bytes, max_starts=0)[1] == n, name
        arr, gn = _filled(buf, len(data), first_bit, chunk_bytes, n + 5, n + 5)
        assert gn == n and arr[:n].tolist() == want.tolist() and (arr[n:] == POISON).all(), name
        if n >= 2:
            arr, gn = _filled(buf, len(data), first_bit, chunk_bytes, n + 5, n - 1)
            assert gn == n and arr[:n - 1].tolist() == want[:n - 1].tolist() and (arr[n - 1:] == POISON).all(), name


@pytest.mark.parametrize("chunk_bytes", (256, 16384))
def test_thousands_of_chunks(chunk_bytes):
    """the 2.5 MiB payload at level 6 (1.3 MB): more chunks than one trip of the compaction takes, and chunks without a start"""
    data = IC.compressed("bench", 6, "gzip")
    want, n = compu_amd.inflate_find_starts_host(data, 80, chunk_bytes)
    got, gn = compu_amd.inflate_find_starts(_device(data), len(data), 80, chunk_bytes)
    n_chunks = -(-len(data) // chunk_bytes)
    assert gn == n and got.cpu().numpy().astype(np.uint64).tolist() == want.tolist()
    assert 0 < n < n_chunks - 1 if chunk_bytes == 256 else n >= (n_chunks - 1) // 2


def test_short_buffers_and_a_late_first_bit():
    data, first_bit = PC.alice("gzip")
    buf = _device(data)
    for length in (0, 1, 2, 255, 256, 257, 511, 512, 513):
        want, n = compu_amd.inflate_find_starts_host(data[:length], 0, 256)
        got, gn = compu_amd.inflate_find_starts(buf, length, 0, 256)
        assert gn == n and got.cpu().numpy().astype(np.uint64).tolist() == want.tolist(), length
    late = 8 * 5000 + 3  # chunks in front of first_bit have no start, the chunk that holds it only behind it
    want, n = compu_amd.inflate_find_starts_host(data, late, 512)
    got, gn = compu_amd.inflate_find_starts(buf, len(data), late, 512)
    assert n > 0 and want[0] > late and gn == n and got.cpu().numpy().astype(np.uint64).tolist() == want.tolist()
