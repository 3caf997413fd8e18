"""chip_zstd_parallel_next on the GPU: one zstd frame decoded slab by slab from a carried cursor.  Every call
decodes into a poisoned room whose bytes behind out_len must stay as they were.  The bytes are the writer's content (or the payload
libzstd compressed) whatever the slabs; where a frame fits a unit, bytes, total and final status are also those of the one-unit
chip_decode_batch on the whole frame.  Without the feature every test here fails at the missing symbol."""
import ctypes as C
import functools
import io
import random

import numpy as np
import pytest

import test_zstd_parallel_decode_gpu as T
import zstd_parallel_cases as P
import zstd_writer as W
from zstd_writer import new_offset as N

pytestmark = pytest.mark.gpu

FINISHED, NEED_OUTPUT, NEED_INPUT = 2, 1, 0
POISON, SLACK = 0xC7, 64
BLOCK_ROOM = 131072


class Dec:
    """One frame in device memory (at an odd address: a slab needs no alignment) and a cursor over it."""

    def __init__(self, torch, frame, checksum=True, wlog=0, cursor=None, pos=0):
        import compu_amd

        self.torch, self.frame, self.checksum, self.wlog = torch, bytes(frame), checksum, wlog
        self.d = torch.full((len(frame) + 9,), 0xA5, dtype=torch.uint8, device="cuda")
        if frame:
            self.d[1:1 + len(frame)] = torch.frombuffer(bytearray(frame), dtype=torch.uint8).cuda()
        self.cur = cursor if cursor is not None else compu_amd.ZstdCursor()
        self.pos, self.out, self.calls = pos, bytearray(), []

    def call(self, end, room=BLOCK_ROOM, grow_state=True):
        """one call over frame[pos:end] into `room` poisoned bytes"""
        import compu_amd

        torch = self.torch
        out = torch.full((room + SLACK,), POISON, dtype=torch.uint8, device="cuda")
        s = compu_amd.zstd_parallel_next(self.cur, self.d[1 + self.pos:1 + end], out[:room], self.wlog, self.checksum, grow_state=grow_state)
        got = out.cpu().numpy()
        assert s.out_len <= room and (got[s.out_len:] == POISON).all(), "bytes behind out_len were written"
        self.out += got[:s.out_len].tobytes()
        self.pos += s.in_used
        self.calls.append(s)
        return s

    def next_block_end(self):
        """where the block at the cursor ends (the frame's end for the last block, so that its checksum comes along; the first
        call takes the frame header with its block)"""
        import compu_amd

        at = self.pos
        if self.cur.phase == 0:
            at += P.py_blocks(self.frame)[1][6]
        if self.cur.phase > 1 or at >= len(self.frame):
            return len(self.frame)
        blocks, summ = compu_amd.zstd_slab_blocks_host(self.frame[at:at + BLOCK_ROOM + 8], 1 << 21)
        if not len(blocks) or blocks[0]["flags"] & 1:
            return len(self.frame)
        return at + 3 + (1 if blocks[0]["type"] == 1 else int(blocks[0]["size"]))

    def block_by_block(self, room=BLOCK_ROOM, max_calls=100000):
        for _ in range(max_calls):
            s = self.call(self.next_block_end(), room)
            if s.status not in (NEED_INPUT, NEED_OUTPUT) or (s.in_used == 0 and s.out_len == 0):
                return s
        raise AssertionError("the decode does not end")

    def by_slabs(self, slab, room=BLOCK_ROOM, max_calls=100000):
        """fixed slab lengths from wherever the cursor stands: blocks are cut and read twice; the slab doubles on no progress"""
        for _ in range(max_calls):
            end = min(len(self.frame), self.pos + slab)
            s = self.call(end, room)
            if s.status not in (NEED_INPUT, NEED_OUTPUT):
                return s
            if s.in_used == 0 and s.out_len == 0:
                if s.status == NEED_OUTPUT:
                    room = max(room, s.need_out)
                elif end == len(self.frame):
                    return s
                else:
                    slab *= 2
        raise AssertionError("the decode does not end")


def three_ways(torch, frame, content, checksum=True, slab=None):
    """(a) one block per call, (b) slabs that end inside blocks, (c) one slab; all three are the content"""
    a = Dec(torch, frame, checksum)
    s = a.block_by_block()
    assert (s.status, bytes(a.out), a.pos, a.cur.phase) == (FINISHED, content, len(frame), 3), ("block by block", s)
    assert a.cur.out_total == len(content) and a.cur.in_total == len(frame)
    blocks = P.py_blocks(frame)[0]
    mid = slab or max(7, max(r[1] for r in blocks) // 2 + 5)  # about half the largest block: every larger block is cut at least once
    b = Dec(torch, frame, checksum)
    s = b.by_slabs(mid)
    assert (s.status, bytes(b.out), b.pos) == (FINISHED, content, len(frame)), ("slabs", mid, s)
    c = Dec(torch, frame, checksum)
    s = c.call(len(frame), max(len(content), 1))
    assert (s.status, bytes(c.out), s.in_used, s.out_len, s.n_blocks) == (FINISHED, content, len(frame), len(content), len(blocks)), ("one slab", s)
    return a, b, c


def parallel_frames():
    """the frames test_zstd_parallel_decode_gpu.py decodes on the parallel path"""
    out = []
    frame, content = T.three_blocks(random.Random(1), checksum=True).finish()
    out.append(("three_blocks_with_matches", frame, content))
    out += [(c.name, c.frame, c.content) for c in T.CASES if c.name in T.MUST_BE_PARALLEL]
    for ov in (1, 2, 3):
        for ll in (0, 4):
            rnd = random.Random(10 * ov + ll)
            f = W.Frame(checksum=True)
            f.raw(rnd.randbytes(100))
            f.compressed(P._rb(rnd, 10), [(2, 5, N(10)), (1, 4, N(20)), (3, 6, N(33))])
            f.rle(0x11, 7)
            f.compressed(P._rb(rnd, 12), [(ll, 5, ov), (2, 6, 1), (0, 4, 2), (1, 7, 3)], last=True)
            out.append((f"repeat_history_ov{ov}_ll{ll}",) + f.finish())
    rnd = random.Random(3)
    f = W.Frame(checksum=True)
    f.raw(rnd.randbytes(64))
    f.compressed(P._rb(rnd, 4), [(2, 5, N(5))])
    f.compressed(P._rb(rnd, 3), [(0, 3, 3)] * 9 + [(1, 4, 1), (0, 3, 2), (0, 5, 3)], last=True)
    out.append(("rep0_minus_1_clamp",) + f.finish())
    f = W.Frame(fcs=None, window=(7, 0), checksum=True)
    f.raw(b"start of a long run: a")
    f.compressed(b"", [(0, 65539 + 23456, N(1))], modes=("pre", "pre", ("rle", 52)), last=True)
    out.append(("offset_1_run_of_88995",) + f.finish())
    rnd = random.Random(4)
    f = W.Frame(fcs=None, window=(0, 0))
    f.raw(rnd.randbytes(100))
    for k in range(40):
        f.compressed(b"", [(0, 100, N(100))], last=k == 39)
    out.append(("forty_copying_blocks",) + f.finish())
    rnd = random.Random(13)
    for last in ("raw", "compressed"):
        f = W.Frame(fcs=None, window=(7, 0), checksum=True)
        f.raw(rnd.randbytes(9000)).rle(0x5A, 70000).compressed(P._rb(rnd, 10), [(2, 50, N(9000)), (3, 400, N(75000))]).rle(7, 0).raw(b"")
        f.compressed(P._rb(rnd, 700), [(300, 2000, N(60000))], lit="huf", streams=4)
        if last == "raw":
            f.raw(b"", last=True)
        else:
            f.compressed(b"", [], lit="rle", last=True)
        out.append((f"mixed_empty_last_{last}",) + f.finish())
    return out + carry_frames()


def carry_frames():
    """what only a carried definer decodes: one block that defines all four kinds, five blocks that define nothing, then the reuse;
    and a definer that a later block replaces"""
    rnd = random.Random(77)
    out = []
    f = W.Frame(fcs=None, window=(2, 0), checksum=True)
    f.raw(rnd.randbytes(500))
    seqs = P._seqs(rnd, 30, 400)
    c = W.seq_codes(seqs)
    lits = bytes(range(60, 90)) + P._rb(rnd, sum(s[0] for s in seqs) + 40, 60, 90)
    fse = (("fse", W.fit(c[0], 6), 6), ("fse", W.fit(c[1], 5), 5), ("fse", W.fit(c[2], 6), 6))
    f.compressed(lits, seqs, lit="huf", streams=1, modes=fse)  # defines Huffman, LL, OF and ML
    f.raw(rnd.randbytes(30)).rle(0x33, 50).compressed(rnd.randbytes(20), []).raw(b"").rle(1, 9)  # five blocks that define nothing
    f.compressed(P._rb(rnd, sum(s[0] for s in seqs) + 9, 60, 90), seqs[::-1], lit="treeless", streams=1, modes=("rep", "rep", "rep"))
    f.compressed(P._rb(rnd, sum(s[0] for s in seqs) + 3, 60, 90), seqs, lit="treeless", streams=4, modes=("rep", "pre", "rep"), last=True)
    out.append(("all_four_kinds_then_five_idle_blocks",) + f.finish())
    f = W.Frame(fcs=None, window=(2, 0), checksum=True)
    f.raw(rnd.randbytes(500))
    f.compressed(lits, seqs, lit="huf", streams=1, modes=fse)
    f.compressed(P._rb(rnd, sum(s[0] for s in seqs) + 9, 60, 90), seqs, lit="treeless", streams=1, modes=("rep", "rep", "rep"))
    seqs2 = P._seqs(rnd, 25, 300)
    c2 = W.seq_codes(seqs2)
    lits2 = bytes(range(100, 120)) + P._rb(rnd, sum(s[0] for s in seqs2) + 50, 100, 120)
    f.compressed(lits2, seqs2, lit="huf", streams=1, modes=(("fse", W.fit(c2[0], 6), 6), "pre", ("fse", W.fit(c2[2], 7), 7)))  # replaces all four
    f.compressed(P._rb(rnd, sum(s[0] for s in seqs2) + 5, 100, 120), seqs2[::-1], lit="treeless", streams=1, modes=("rep", "rep", "rep"), last=True)
    out.append(("a_definer_replaced_in_a_later_slab",) + f.finish())
    return out


FRAMES = parallel_frames()


@pytest.mark.parametrize("name,frame,content", FRAMES, ids=[f[0] for f in FRAMES])
def test_slab_cuts(gpu, name, frame, content):
    want = T.batch(gpu, frame, len(content))
    assert want[3] == FINISHED and want[0] == content
    a, b, c = three_ways(gpu, frame, content)
    got, summ = T.par(gpu, frame, len(content))  # chip_zstd_parallel: the same bytes and total
    assert (got, summ.total_out, summ.in_used) == (bytes(c.out), len(c.out), c.pos)
    three_ways(gpu, frame, content, checksum=False)


def test_one_block_per_call_reads_carried_definers(gpu):
    """with one block per call every treeless block and every Repeat mode has its source in the carry"""
    for name, frame, content in carry_frames():
        rows = P.py_blocks(frame)[0]
        reuses = sum(1 for r in rows if r[5] == 2 and (r[7] == 3 or (r[4] and 3 in r[8])))
        assert reuses >= 2, name
        d = Dec(gpu, frame)
        assert d.block_by_block().status == FINISHED and bytes(d.out) == content
        assert all(s.n_blocks <= 1 for s in d.calls)
        assert all(d.cur.raw.carry_len[k] > 3 for k in range(4)), name


# ---- the window ----
def test_offsets_of_exactly_hist_and_exactly_the_window_and_one_more(gpu):
    rnd = random.Random(80)
    # hist < window: 600 bytes delivered, 10 literals in front of the match
    for off, ok in ((610, True), (611, False)):
        f = W.Frame(fcs=None, window=(0, 0))
        f.raw(rnd.randbytes(300)).raw(rnd.randbytes(300))
        f.compressed(P._rb(rnd, 10), [(10, 5, N(off))], invalid=1)
        f.raw(b"tail", last=True)
        frame, content = f.finish()
        d = Dec(gpu, frame)
        s = d.block_by_block()
        if ok:
            assert s.status == FINISHED and bytes(d.out) == content
        else:
            assert (s.status, bytes(d.out), s.out_len, d.cur.phase, d.cur.error) == (-20, content[:600], 0, 4, -20)
            assert d.call(len(frame)).status == -20 and bytes(d.out) == content[:600]  # sticky
        d = Dec(gpu, frame)  # the same verdict with the blocks in one slab: the blocks in front are delivered
        s = d.call(len(frame), 4096)
        assert (s.status, bytes(d.out)) == ((FINISHED, content) if ok else (-20, content[:600]))
    # hist == window: 1200 bytes delivered under a 1 KiB window
    for off, ok in ((1024, True), (1025, False)):
        f = W.Frame(fcs=None, window=(0, 0))
        for _ in range(4):
            f.raw(rnd.randbytes(300))
        f.compressed(P._rb(rnd, 10), [(0, 7, N(off)), (10, 5, N(off))], last=True)
        frame, content = f.finish()
        d = Dec(gpu, frame)
        s = d.block_by_block()
        assert (s.status, bytes(d.out)) == ((FINISHED, content) if ok else (-20, content[:1200]))
        assert (T.batch(gpu, frame, len(content) + 8)[3] == FINISHED) == ok


def test_a_single_segment_frame_and_a_run_whose_source_byte_lies_in_the_window(gpu):
    rnd = random.Random(81)
    f = W.Frame(checksum=True)  # Single_Segment: the window is the content size
    f.raw(rnd.randbytes(290) + b"a")
    f.compressed(b"", [(0, 500, N(1))])  # a run at offset 1 from the last byte of the block in front
    f.compressed(P._rb(rnd, 20), [(5, 40, N(796)), (10, 30, N(300))], last=True)  # to the frame's first byte
    frame, content = f.finish()
    assert content[291:791] == b"a" * 500
    three_ways(gpu, frame, content)
    assert T.batch(gpu, frame, len(content))[0] == content


def test_the_ring_wraps_several_times(gpu):
    rnd = random.Random(82)
    f = W.Frame(fcs=None, window=(0, 0), checksum=True)
    f.raw(rnd.randbytes(310))
    for k in range(28):  # 28 blocks of about 300 bytes under a 1 KiB window: more than 7 KiB
        avail = min(len(f.content), 1024)
        seqs = [(rnd.randrange(0, 9), rnd.randrange(20, 90), N(rnd.choice([avail, avail - 1, 1, rnd.randrange(1, avail)]))) for _ in range(5)]
        f.compressed(P._rb(rnd, sum(s[0] for s in seqs) + 7), seqs, last=k == 27)
    frame, content = f.finish()
    assert len(content) > 7 * 1024
    a, b, c = three_ways(gpu, frame, content)
    assert a.cur.hist == 1024 and a.cur.ring == len(content) % 1024 and a.cur.state.numel() == a.cur.window_size + 524352
    ring = a.cur.state[524352:].cpu().numpy().tobytes()  # content byte j lies at j mod window
    assert all(ring[j % 1024] == content[j] for j in range(len(content) - 1024, len(content)))
    assert T.batch(gpu, frame, len(content))[0] == content


# ---- room and input ----
def test_room_one_byte_short_slab_shorter_than_its_block_and_a_state_too_small(gpu, monkeypatch):
    import compu_amd

    ends, block = [], W.Frame._block  # the writer's content cut points: the content's length behind each block it writes

    def noting(self, *args):
        ends.append(len(self.content))
        return block(self, *args)

    monkeypatch.setattr(W.Frame, "_block", noting)
    frame, content = T.three_blocks(random.Random(83), checksum=True, fcs=None, window=(0, 0)).finish()
    monkeypatch.undo()
    assert len(ends) == 3 and ends[2] == len(content)
    n0, n1 = ends[0], ends[1] - ends[0]  # what the first and the second block decode to
    cuts = [r[0] for r in P.py_blocks(frame)[0]]
    d = Dec(gpu, frame)
    s = d.call(cuts[1], grow_state=False)  # header and first block, a state without a window
    assert (s.status, s.in_used, s.out_len, s.need_state, d.cur.phase) == (NEED_OUTPUT, cuts[0], 0, 524352 + 1024, 1)
    s = d.call(cuts[1], grow_state=False)  # again, now at BLOCKS: the same answer, no progress
    assert (s.status, s.in_used, s.out_len, s.need_state) == (NEED_OUTPUT, 0, 0, 524352 + 1024)
    d.cur.state = gpu.zeros(524352 + 1024, dtype=gpu.uint8, device="cuda")
    first = d.cur.copy()
    s = d.call(cuts[1] - 1)  # one byte short of the block
    assert (s.status, s.in_used, s.out_len) == (NEED_INPUT, 0, 0) and bytes(d.cur.raw) == bytes(first.raw)
    s = d.call(cuts[1], n0 - 1)
    assert (s.status, s.in_used, s.out_len, s.need_out) == (NEED_OUTPUT, 0, 0, n0) and bytes(d.cur.raw) == bytes(first.raw), s
    s = d.call(len(frame), n0)  # room for exactly one block: it is delivered, the next one says what it needs
    assert (s.status, s.in_used, s.out_len, s.n_blocks) == (NEED_OUTPUT, cuts[1] - cuts[0], n0, 1) and s.need_out == n1
    s = d.by_slabs(len(frame), 4096)
    assert s.status == FINISHED and bytes(d.out) == content


def test_the_frame_header_and_the_checksum_cut_across_two_slabs(gpu):
    frame, content = T.three_blocks(random.Random(84), checksum=True, fcs=8).finish()
    d = Dec(gpu, frame)
    for n in (0, 3, 4, 5, 12):  # (magic, descriptor and 8 bytes of content size)
        s = d.call(n)
        assert (s.status, s.in_used, s.out_len, d.cur.phase) == (NEED_INPUT, 0, 0, 0), n
    s = d.call(13)
    assert (s.status, s.in_used, d.cur.phase, d.cur.content_size) == (NEED_INPUT, 13, 1, len(content))
    s = d.call(len(frame) - 2, 4096)  # every block, half the checksum
    assert (s.status, s.out_len, d.pos, d.cur.phase) == (NEED_INPUT, len(content), len(frame) - 4, 2) and bytes(d.out) == content
    s = d.call(len(frame) - 1)
    assert (s.status, s.in_used, s.out_len, d.cur.phase) == (NEED_INPUT, 0, 0, 2)
    d.cur.state = d.cur.state[:16].clone()  # behind the last block neither the carry nor the window is read: the state may have gone
    s = d.call(len(frame))
    assert (s.status, s.in_used, s.out_len, s.need_state, d.cur.phase, d.pos) == (FINISHED, 4, 0, 0, 3, len(frame))
    assert d.call(len(frame)).status == FINISHED and d.pos == len(frame)  # a finished cursor stays finished
    # bytes behind the frame are not its business
    d = Dec(gpu, frame + b"\xff" * 9)
    s = d.call(len(frame) + 9, 4096)
    assert (s.status, s.in_used, bytes(d.out)) == (FINISHED, len(frame), content)


# ---- errors ----
def damaged_frames():
    out = []
    for bad in T.BAD:
        out.append((f"three_blocks_{bad}",) + T.three_blocks(random.Random(6), bad=bad).finish())
    rnd = random.Random(7)
    f = W.Frame()
    f.compressed(P._rb(rnd, 60), [(20, 30, N(15))])
    f.compressed(P._rb(rnd, 50, 60, 70), [(15, 40, N(90))], lit="huf", lit_regen=49)
    f.compressed(P._rb(rnd, 40), [(10, 50, N(150))], last=True)
    out.append(("short_huffman_regen",) + f.finish())
    for name, mid in T._fse_damages():
        out.append((name,) + T.around(random.Random(15), b"ab", [(1, 5, N(9))], **mid))
    for name, tree in (("rest_not_pow2", bytes([127 + 2, 0x31])), ("all_zero", bytes([127 + 2, 0x00])), ("weight_12", bytes([127 + 3, 0xC1, 0x10]))):
        rnd = random.Random(16)
        out.append((f"huffman_tree_{name}",) + T.around(rnd, P._rb(rnd, 100, 97, 100), [], lit="huf", weights=[0] * 97 + [2, 1, 1], tree_bytes=tree))
    for streams in (1, 4):
        for key, val in (("lit_extra", 5), ("lit_drop", 2)):
            rnd = random.Random(17)
            out.append((f"huffman_streams_{streams}_{key}",) + T.around(rnd, P._rb(rnd, 300, 60, 70), [(3, 9, N(40)), (1, 5, 2), (0, 30, N(20))], lit="huf",
                                                                      streams=streams, **{key: val}))
    for what in ("fse", "huffman"):  # a damaged description that a later block replays
        rnd = random.Random(18)
        f = W.Frame()
        f.raw(rnd.randbytes(200))
        if what == "fse":
            f.compressed(b"ab", [(1, 5, N(9))], modes=(("fse", [2] * 16, 5), "pre", "pre"), al_field={"ll": 10}, invalid=1)
            f.compressed(b"cd", [(1, 5, N(9))], modes=("rep", "pre", "pre"), last=True)
        else:
            f.compressed(P._rb(rnd, 100, 97, 100), [], lit="huf", weights=[0] * 97 + [2, 1, 1], tree_bytes=bytes([127 + 2, 0x00]))
            f.compressed(P._rb(rnd, 50, 97, 100), [(3, 4, N(20))], lit="treeless", last=True)
        out.append((f"replayed_damage_{what}",) + f.finish())
    out += [(c.name, c.frame, c.content) for c in P.source_cases() if "without_source" in c.name]
    return out


DAMAGED = damaged_frames()


@pytest.mark.parametrize("name,frame,content", DAMAGED, ids=[d[0] for d in DAMAGED])
def test_a_damaged_block_is_the_batchs_status_with_the_blocks_in_front_delivered(gpu, name, frame, content):
    want = T.batch(gpu, frame, len(content) + 64)
    assert want[3] < 0
    for how in ("block_by_block", "one_slab"):
        d = Dec(gpu, frame)
        s = d.block_by_block() if how == "block_by_block" else d.call(len(frame), len(content) + 64)
        print(name, how, "batch", want[1:], "next", s)
        assert s.status == want[3], how
        assert bytes(d.out) == want[0] and d.cur.phase == 4 and d.cur.error == want[3], how
        again = d.call(len(frame))
        assert (again.status, again.out_len, again.in_used) == (want[3], 0, 0), how  # sticky


def test_a_wrong_checksum_and_a_content_size_off_by_one(gpu):
    frame, content = T.three_blocks(random.Random(9), checksum=True).finish(checksum_value=0x12345678)
    for how in ("block_by_block", "one_slab"):
        d = Dec(gpu, frame)
        s = d.block_by_block() if how == "block_by_block" else d.call(len(frame), 4096)
        assert (s.status, bytes(d.out), d.cur.phase, d.pos) == (-22, content, 4, len(frame))  # found behind all content
        d = Dec(gpu, frame, checksum=False)
        s = d.block_by_block() if how == "block_by_block" else d.call(len(frame), 4096)
        assert (s.status, bytes(d.out), d.pos) == (FINISHED, content, len(frame))
    assert T.batch(gpu, frame, len(content))[3] == -22
    n = len(T.three_blocks(random.Random(9)).finish()[1])
    for delta in (1, -1):
        f = T.three_blocks(random.Random(9), fcs=4, window=(0, 0), fcs_value=n + delta)
        frame, content = f.finish()
        cuts = [r[0] for r in P.py_blocks(frame)[0]]
        for how in ("block_by_block", "one_slab"):
            d = Dec(gpu, frame)
            s = d.block_by_block() if how == "block_by_block" else d.call(len(frame), 4096)
            assert s.status == -20 and d.cur.phase == 4, (delta, how)
            assert bytes(d.out) == content[:len(d.out)] and d.pos == cuts[2], (delta, how)  # the two blocks in front of the last one


def test_single_bit_flips_of_a_three_block_libzstd_frame(gpu, alice):
    import zstd_ref

    z = zstd_ref.load()
    data = (alice * 3)[:300000]
    frame = zstd_ref.compress(z, data, 3, True, True)
    assert len(P.py_blocks(frame)[0]) == 3
    rnd = random.Random(85)
    disagree = []
    for k in range(300):
        bit = rnd.randrange(len(frame) * 8) if k >= 60 else rnd.randrange(20 * 8)  # (a fifth of them in the frame header and the first block's headers)
        bad = bytearray(frame)
        bad[bit >> 3] ^= 1 << (bit & 7)
        want = T.batch(gpu, bytes(bad), len(data) + 64)
        d = Dec(gpu, bytes(bad))
        s = d.block_by_block()
        if (s.status < 0) != (want[3] < 0) or (s.status == FINISHED and want[3] == FINISHED and bytes(d.out) != want[0]):
            disagree.append((bit, want[1:], s))
    assert not disagree, disagree[:5]


# ---- 64-bit totals ----
def test_totals_beyond_2_pow_32(gpu):
    import compu_amd

    rnd = random.Random(86)
    window, before = 1 << 17, (1 << 32) - 70000
    hist = rnd.randbytes(window)
    f = W.Frame(fcs=None, window=(7, 0))
    f.content = bytearray(hist)  # what the writer's matches may reach
    f.raw(rnd.randbytes(60000))
    f.compressed(P._rb(rnd, 300), [(100, 9000, N(131072)), (50, 20000, N(100000)), (20, 700, N(3))])
    f.rle(0x42, 49000)
    rest = 140000 - (len(f.content) - window)
    f.raw(rnd.randbytes(rest), last=True)
    blocks, content = bytes(f.blocks), bytes(f.content[window:])
    assert len(content) == 140000
    ring = np.zeros(window, np.uint8)
    ring[(before - window + np.arange(window)) % window] = np.frombuffer(hist, np.uint8)  # content byte j lies at j mod window

    def cursor(content_size, in_total):
        cur = compu_amd.ZstdCursor()
        cur.phase, cur.window_size, cur.content_size, cur.out_total, cur.in_total = 1, window, content_size, before, in_total
        cur.hist, cur.ring = window, before % window
        cur.raw.rep[0], cur.raw.rep[1], cur.raw.rep[2] = 1, 4, 8
        cur.state = gpu.zeros(524352 + window, dtype=gpu.uint8, device="cuda")
        cur.state[524352:] = gpu.from_numpy(ring).cuda()
        return cur

    for in_total in (6, (1 << 32) + 12345):
        for slab in (len(blocks), 50000):
            d = Dec(gpu, blocks, cursor=cursor((1 << 32) + 70000, in_total))
            s = d.by_slabs(slab)
            assert (s.status, bytes(d.out)) == (FINISHED, content), (in_total, slab, s)
            assert (d.cur.out_total, d.cur.in_total, d.cur.phase) == ((1 << 32) + 70000, in_total + len(blocks), 3)
        d = Dec(gpu, blocks, cursor=cursor(70000, in_total))  # the content size lower by 2^32
        s = d.by_slabs(len(blocks))
        assert s.status == -20 and d.cur.phase == 4 and len(d.out) == 0
        d = Dec(gpu, blocks, cursor=cursor((1 << 32) + 70001, in_total))
        s = d.by_slabs(50000)
        assert s.status == -20 and bytes(d.out) == content[:len(d.out)] and len(d.out) == 140000 - rest


# ---- libzstd frames ----
@functools.lru_cache(maxsize=None)
def _libzstd_frames(alice):
    return list(T.libzstd_frames(alice))


def test_libzstd_frames_in_slabs_and_block_by_block(gpu, alice):
    for cname, level, data, frame in _libzstd_frames(alice):
        for checksum in (True, False):
            d = Dec(gpu, frame, checksum)
            s = d.by_slabs(100000)
            assert (s.status, d.pos) == (FINISHED, len(frame)) and bytes(d.out) == data, (cname, level, checksum)
            assert len(d.calls) >= 4
            d = Dec(gpu, frame, checksum)
            s = d.block_by_block()
            assert (s.status, d.pos) == (FINISHED, len(frame)) and bytes(d.out) == data, (cname, level, checksum)
            assert d.cur.raw.xxh.total == (len(data) if checksum else 0)


def test_a_libzstd_frame_with_a_16_mib_window(gpu, alice):
    import compu_amd
    import zstd_ref

    z = zstd_ref.load()
    data = b"".join(alice[k * 997 % len(alice):] + alice[:k * 997 % len(alice)] for k in range(112))  # 16.2 MiB: matches about 150 KB back
    cctx = z.ZSTD_createCCtx()
    rcs = [z.ZSTD_CCtx_setParameter(cctx, 100, 1), z.ZSTD_CCtx_setParameter(cctx, 201, 1), z.ZSTD_CCtx_setParameter(cctx, 101, 24)]  # level, checksum, windowLog
    if any(z.ZSTD_isError(r) for r in rcs):
        z.ZSTD_freeCCtx(cctx)
        print("the system libzstd does not accept ZSTD_c_windowLog = 24: nothing to decode")
        return
    cap = z.ZSTD_compressBound(len(data))
    dst = C.create_string_buffer(cap)
    n = z.ZSTD_compress2(cctx, dst, cap, data, len(data))
    z.ZSTD_freeCCtx(cctx)
    assert not z.ZSTD_isError(n)
    frame = dst.raw[:n]
    _, bs = compu_amd.zstd_blocks_host(frame)
    assert bs.window_size == 1 << 24, bs
    d = Dec(gpu, frame)
    s = d.by_slabs(max(len(frame) // 9, 4096), 4 << 20)
    assert (s.status, d.pos) == (FINISHED, len(frame)) and bytes(d.out) == data
    assert len(d.calls) >= 8 and d.cur.state.numel() == 524352 + (1 << 24)


# ---- cursor discipline ----
def test_cursor_discipline(gpu, alice):
    import compu_amd

    cname, level, data, frame = _libzstd_frames(alice)[1]
    d = Dec(gpu, frame)
    for _ in range(4):
        d.call(d.next_block_end())
    twin = Dec(gpu, frame, cursor=d.cur.copy(), pos=d.pos)
    assert bytes(twin.cur.raw) == bytes(d.cur.raw) and twin.cur.state.data_ptr() != d.cur.state.data_ptr()
    compu_amd.trim()  # the scratch goes away between two calls of a frame
    # the two cursors interleaved on one stream
    done = [False, False]
    while not all(done):
        for k, x in enumerate((d, twin)):
            if not done[k]:
                s = x.call(min(len(frame), x.pos + (260000 if k else 190000)), 1 << 20)  # (either holds a whole block of at most 128 KiB)
                done[k] = s.status == FINISHED
                assert s.status in (NEED_INPUT, NEED_OUTPUT, FINISHED)
    assert bytes(d.out) == data and bytes(twin.out) == data[len(data) - len(twin.out):] and len(twin.out) == len(data) - 4 * 131072
    # an invalid cursor, and the flag changed mid-frame
    e = Dec(gpu, frame)
    e.call(e.next_block_end())
    e.cur.hist += 1
    with pytest.raises(RuntimeError, match="-101"):
        e.call(len(frame))
    e.cur.hist -= 1
    e.checksum = False
    with pytest.raises(RuntimeError, match="-101"):
        e.call(len(frame))
    e.checksum = True
    assert e.by_slabs(1 << 20, 1 << 21).status == FINISHED and bytes(e.out) == data


# ---- scratch ----
def test_scratch_is_bounded_by_slab_and_room(gpu):
    import compu_amd

    rnd = random.Random(87)
    f = W.Frame(fcs=None, window=(7, 0), checksum=True)
    piece = rnd.randbytes(131072)
    for k in range(192):  # 48 MiB: raw and RLE blocks, and now and then a compressed one that copies from both
        f.raw(piece[k:] + piece[:k]).rle(k & 255, 131072)
        if k % 23 == 0:
            f.compressed(P._rb(rnd, 100), [(40, 60000, N(131072)), (30, 50000, N(70000)), (0, 9000, N(1))])
    f.raw(b"the end", last=True)
    frame, content = f.finish()
    assert len(content) > 48 << 20
    compu_amd.trim()
    torch = gpu
    d_in = torch.frombuffer(bytearray(frame), dtype=torch.uint8).cuda()
    room = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
    cur, pos, out_pos, used = compu_amd.ZstdCursor(), 0, 0, []
    for _ in range(100):
        s = compu_amd.zstd_parallel_next(cur, d_in[pos:pos + (4 << 20)], room)
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        used.append(total - free)
        assert room[:s.out_len].cpu().numpy().tobytes() == content[out_pos:out_pos + s.out_len]
        pos, out_pos = pos + s.in_used, out_pos + s.out_len
        if s.status == FINISHED:
            break
        assert s.status in (NEED_INPUT, NEED_OUTPUT) and s.out_len > 0
    assert s.status == FINISHED and out_pos == len(content) and pos == len(frame) and len(used) >= 6
    print("device bytes in use after each call:", used)
    assert max(used[1:]) <= used[1], used  # nothing grows from the second call to the last
    compu_amd.trim()  # the scratch is the launch slot's: it goes with it
    free, total = torch.cuda.mem_get_info()
    assert total - free < used[-1]


# ---- zstd_parallel_stream ----
def test_zstd_parallel_stream(gpu, alice):
    import compu_amd

    frame, content = T.three_blocks(random.Random(88), checksum=True, fcs=None, window=(0, 0)).finish()
    assert compu_amd.zstd_parallel_stream(frame) == content
    assert compu_amd.zstd_parallel_stream(frame, slab_bytes=5, out_bytes=3) == content  # the slab doubles, the room goes to need_out
    assert compu_amd.zstd_parallel_stream(frame, checksum=False) == content
    sink = io.BytesIO()
    assert compu_amd.zstd_parallel_stream(io.BytesIO(frame), sink, slab_bytes=64, out_bytes=200) == len(content) and sink.getvalue() == content
    cname, level, data, big = _libzstd_frames(alice)[4]
    assert compu_amd.zstd_parallel_stream(io.BytesIO(big), slab_bytes=300000, out_bytes=1 << 20) == data
    # frames=True: two frames with a skippable frame between them, and one behind; without it the first frame alone
    second, content2 = T.three_blocks(random.Random(89)).finish()
    both = frame + W.skippable(b"between") + second + W.skippable(b"", 5)
    assert compu_amd.zstd_parallel_stream(both, frames=True, slab_bytes=50) == content + content2
    assert compu_amd.zstd_parallel_stream(io.BytesIO(both), frames=True) == content + content2
    assert compu_amd.zstd_parallel_stream(both) == content
    with pytest.raises(EOFError):
        compu_amd.zstd_parallel_stream(frame[:-3])
    with pytest.raises(EOFError):
        compu_amd.zstd_parallel_stream(io.BytesIO(frame[:40]), slab_bytes=16)
    with pytest.raises(compu_amd.DecodeError):
        compu_amd.zstd_parallel_stream(b"not a zstd frame at all")
    bad, _ = T.three_blocks(random.Random(90), checksum=True).finish(checksum_value=1)
    with pytest.raises(compu_amd.DecodeError) as err:
        compu_amd.zstd_parallel_stream(bad)
    assert "-22" in str(err.value) or getattr(err.value, "code", -22) == -22
