"""chip_pack_units on the GPU: the packed bytes, the offsets and the total against numpy at every pair of source and destination
alignments, at the lengths around the 16-byte chunk, the 1 KiB round and the 4 KiB tile, for a unit of many tiles and a tile of
many units, with sources in any order, with gaps and shared; nothing written in front of the destination, behind `total`, or at
all when the room is a byte short.  The destination sits in a poisoned tensor with 64 guard bytes on each side.  Without the
feature every test here fails at the missing symbol."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD, POISON, POISON64 = 64, 0xEE, 0x7E7E7E7E7E7E7E7E


def pack(torch, src_bytes, offs, lens, src_mis=0, dst_mis=0, cap=None, want_off=True, slack=40):
    """chip_pack_units of the ranges src_bytes[offs[i] .. + lens[i]) -- the source placed `src_mis` bytes behind a 16-byte aligned
    address, the destination `dst_mis` behind one, with room for `cap` bytes (None: the total) and `slack` bytes behind the room --
    checked against numpy: (rc, total) and the destination bytes, which hold the packed ranges when they fit and poison wherever
    nothing may be written."""
    import compu_amd

    lib = compu_amd.lib()
    n = len(lens)
    assert len(offs) == n and all(0 <= o and o + l <= len(src_bytes) for o, l in zip(offs, lens)), "a range outside the source"
    want = b"".join(bytes(src_bytes[o:o + l]) for o, l in zip(offs, lens))
    total_want = len(want)
    cap = total_want if cap is None else cap
    d_src = torch.full((GUARD + src_mis + len(src_bytes) + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    if len(src_bytes):
        d_src[GUARD + src_mis:GUARD + src_mis + len(src_bytes)] = torch.from_numpy(np.frombuffer(bytes(src_bytes), np.uint8).copy()).cuda()
    d_dst = torch.full((GUARD + dst_mis + max(cap, total_want) + slack + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    d_off = torch.from_numpy(np.asarray(offs, np.int64).reshape(n)).cuda()
    d_len = torch.from_numpy(np.asarray(lens, np.uint32).reshape(n).view(np.int32)).cuda()
    d_doff = torch.full((n + 2,), POISON64, dtype=torch.int64, device="cuda")
    total = C.c_uint64(12345)
    p = lambda t, at=0: C.c_void_p(t.data_ptr() + at)  # noqa: E731
    rc = lib.chip_pack_units(n, p(d_src, GUARD + src_mis), p(d_off), p(d_len), p(d_dst, GUARD + dst_mis), cap, p(d_doff) if want_off else None,
                             C.byref(total), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and total.value == total_want
    got_off = d_doff.cpu().numpy()
    if want_off:
        assert got_off[:n].tolist() == list(itertools.accumulate([0] + list(lens)))[:n]
        assert (got_off[n:] == POISON64).all()
    else:
        assert (got_off == POISON64).all()
    got = d_dst.cpu().numpy()
    at = GUARD + dst_mis
    assert (got[:at] == POISON).all(), "bytes in front of the destination were written"
    if total_want <= cap:
        assert got[at:at + total_want].tobytes() == want
        assert (got[at + total_want:] == POISON).all(), "bytes behind the total were written"
    else:
        assert (got == POISON).all(), "the destination was written although the units do not fit"
    return total.value


def source(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def test_every_pair_of_alignments(gpu):
    """units of 0..48 bytes at src_off = 64 * k + j: every source misalignment j against every destination misalignment"""
    src = source(64 * 49 + 64)
    lens = list(range(49))
    for j in range(16):
        offs = [64 * k + j for k in range(49)]
        for dst_mis in range(16):
            assert pack(gpu, src, offs, lens, src_mis=0, dst_mis=dst_mis) == sum(lens)
    # the same ranges with the source base itself misaligned
    for src_mis in (1, 7, 15):
        assert pack(gpu, src, [64 * k for k in range(49)], lens, src_mis=src_mis, dst_mis=3) == sum(lens)


BOUNDARY = [0, 1, 15, 16, 17, 1023, 1024, 1025, 65539]


@pytest.mark.parametrize("dst_mis", [0, 5])
def test_boundary_lengths(gpu, dst_mis):
    src = source(sum(BOUNDARY) + 100 * len(BOUNDARY))
    offs = np.concatenate(([0], np.cumsum(BOUNDARY)))[:-1].tolist()
    pack(gpu, src, offs, BOUNDARY, src_mis=3, dst_mis=dst_mis)
    # the same batch, the source ranges in reverse order and with gaps of 1..99 bytes between them
    roffs, at = [], 0
    for i, ln in enumerate(reversed(BOUNDARY)):
        at += 11 * i + 1
        roffs.append(at)
        at += ln
    pack(gpu, src, roffs[::-1], BOUNDARY, src_mis=0, dst_mis=dst_mis)
    # one source range used by two units, and two ranges that overlap
    pack(gpu, src, [100, 100, 90, 0], [1025, 1025, 60000, 17], src_mis=9, dst_mis=dst_mis)


def test_one_unit_of_many_tiles(gpu):
    n = 5 * (1 << 20) + 7
    pack(gpu, source(n + 13), [13], [n], src_mis=6, dst_mis=11)


def test_many_units_in_one_tile(gpu):
    src = source(80000)
    lens = [1] * 3000 + [70000]
    offs = [(7 * i) % 3000 for i in range(3000)] + [3001]
    for dst_mis in (0, 9):
        pack(gpu, src, offs, lens, dst_mis=dst_mis)
    # empty units between the others: at the start, in the middle of a tile, at a tile's edge, at the end
    lens = [0, 0, 4090, 0, 6, 0, 0, 100, 0]
    pack(gpu, src, [50 * i for i in range(len(lens))], lens)


def test_an_all_empty_batch(gpu):
    assert pack(gpu, source(128), list(range(100)), [0] * 100, cap=0) == 0
    assert pack(gpu, source(64), [0] * 100, [0] * 100, cap=32) == 0
    assert pack(gpu, b"", [], [], cap=16) == 0  # no unit: the device is not touched


def test_dst_off_may_be_null(gpu):
    src = source(70000)
    assert pack(gpu, src, [5, 100, 30], [1000, 65539, 17], dst_mis=2, want_off=False) == 66556


@pytest.mark.parametrize("lens", [[1], [16], [4096], [0, 1025, 65539, 15]], ids=["1", "16", "4096", "mixed"])
def test_no_room_writes_nothing(gpu, lens):
    src = source(sum(lens) + 64)
    offs = np.concatenate(([0], np.cumsum(lens)))[:-1].tolist()
    total = sum(lens)
    for dst_mis in (0, 13):
        assert pack(gpu, src, offs, lens, dst_mis=dst_mis, cap=total - 1) == total  # rc 0, total and dst_off right, dst untouched
        assert pack(gpu, src, offs, lens, dst_mis=dst_mis, cap=total) == total  # exact bytes, the byte behind untouched
        assert pack(gpu, src, offs, lens, dst_mis=dst_mis, cap=total + 1) == total


def test_the_python_face(gpu):
    import compu_amd

    src = gpu.from_numpy(np.frombuffer(source(5000), np.uint8).copy()).cuda()
    off = gpu.tensor([4000, 0, 77], dtype=gpu.int64, device="cuda")
    ln = gpu.tensor([1000, 33, 0], dtype=gpu.int32, device="cuda")
    dst, dst_off, total = compu_amd.pack_units(src, off, ln)
    host = src.cpu().numpy()
    assert total == 1033 and dst.numel() == 1033 and dst_off.tolist() == [0, 1000, 1033]
    assert dst.cpu().numpy().tobytes() == host[4000:5000].tobytes() + host[:33].tobytes()
    small = gpu.full((1032,), POISON, dtype=gpu.uint8, device="cuda")
    _, _, total = compu_amd.pack_units(src, off, ln, dst=small)
    assert total == 1033 and (small.cpu().numpy() == POISON).all()
