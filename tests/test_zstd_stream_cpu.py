"""The host twins of chip_zstd_parallel_next, no GPU: the walk from a block boundary against the writer's
block_cuts() and the Python reading of tests/zstd_parallel_cases.py, the header step against chip_zstd_blocks_host's summary, and
the running XXH64 against the checksum field the system libzstd writes.  Without the feature every test here fails at the missing
symbol.

The slab is cut at every byte, from every block boundary, and every record is compared at every cut: the expected records of a
boundary are laid out once as the library's own record array and compared as bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import zstd_cases as Z
import zstd_parallel_cases as P
import zstd_writer as W

FINISHED, NEED_INPUT = 2, 0
ANY_SIZE = 1 << 21  # a Block_Maximum_Size no 21-bit Block_Size exceeds: the structural tests look at the walk alone


def decodable_frames():
    out = [(c.name, c.frame) for c in P.all_cases()]
    out += [(c.name, c.frame) for c in Z.all_cases() if isinstance(c.want, bytes) and c.frame[:4] == W.MAGIC]
    return out


FRAMES = decodable_frames()


class Walk:
    """chip_zstd_slab_blocks_host into one array that is allocated once"""

    def __init__(self, room):
        import compu_amd
        from compu_amd.api import _ZstdSlabSummary

        self.call = compu_amd.lib().chip_zstd_slab_blocks_host
        self.blocks = np.zeros(room, compu_amd.zstd_block_dtype())
        self.raw = _ZstdSlabSummary()

    def __call__(self, buf, start, length, block_max=ANY_SIZE):
        """the walk over buf[start : start + length] (buf a uint8 array): (rows, (n_blocks, in_used, status, last))"""
        self.blocks[:] = 0
        rc = self.call(C.c_void_p(buf.ctypes.data + start) if length else None, length, block_max, len(self.blocks),
                       self.blocks.ctypes.data_as(C.c_void_p), C.byref(self.raw))
        assert rc == 0
        n = int(self.raw.n_blocks)
        rows = [(int(b["offset"]), int(b["size"]), int(b["lit_regen"]), int(b["lit_comp"]), int(b["n_seq"]), int(b["type"]), int(b["flags"]),
                 int(b["lit_type"]), tuple(int(m) for m in b["mode"]), tuple(int(s) for s in b["src"])) for b in self.blocks[:n]]
        return rows, (n, int(self.raw.in_used), int(self.raw.status), int(self.raw.last))


def expected_records(rows, cuts, j):
    """rows[j:] as the record array the walk from boundary j must fill: slab-relative offsets, sources inside the slab"""
    import compu_amd

    exp = np.zeros(len(rows) - j, compu_amd.zstd_block_dtype())
    for k, r in enumerate(rows[j:]):
        e = exp[k]
        e["offset"], e["size"], e["lit_regen"], e["lit_comp"], e["n_seq"], e["type"], e["flags"], e["lit_type"] = (r[0] - cuts[j],) + r[1:8]
        e["mode"] = r[8]
        e["src"] = [s - j if s >= j else -1 for s in r[9]]  # a definer in front of the slab is the carry's business
    return exp


@pytest.mark.parametrize("name,frame", FRAMES, ids=[f[0] for f in FRAMES])
def test_walk_from_every_boundary_with_the_slab_cut_at_every_byte(name, frame):
    import compu_amd
    from compu_amd.api import _ZstdSlabSummary

    rows, summ = P.py_blocks(frame)
    assert summ[4] == P.OK
    cuts = [r[0] for r in rows] + [summ[1] - (4 if summ[5] & 4 else 0)]  # block starts, and the end of the last block
    call, raw = compu_amd.lib().chip_zstd_slab_blocks_host, _ZstdSlabSummary()
    got = np.zeros(len(rows) + 1, compu_amd.zstd_block_dtype())
    room, p_got, p_raw = len(got), got.ctypes.data_as(C.c_void_p), C.byref(raw)
    buf = np.frombuffer(frame, np.uint8)
    for j in range(len(rows)):
        exp = expected_records(rows, cuts, j)
        exp_bytes = [exp[:k].tobytes() for k in range(len(exp) + 1)]
        p_in, whole = C.c_void_p(buf.ctypes.data + cuts[j]), 0
        for length in range(len(frame) - cuts[j] + 1):  # every byte, through the checksum behind the last block
            while j + whole < len(rows) and cuts[j + whole + 1] - cuts[j] <= length:
                whole += 1
            at_end = j + whole == len(rows)
            assert call(p_in, length, ANY_SIZE, room, p_got, p_raw) == 0
            assert (raw.n_blocks, raw.in_used, raw.status, raw.last) == (whole, cuts[j + whole] - cuts[j], P.OK if at_end else P.TRUNCATED, int(at_end)), (j, length)
            assert got[:whole].tobytes() == exp_bytes[whole], (j, length)


def test_walk_agrees_with_the_writers_block_cuts():
    seen = 0
    for c in Z.all_cases():
        if not isinstance(c.want, bytes) or c.frame[:4] != W.MAGIC:
            continue
        walk, buf = Walk(len(c.cuts)), np.frombuffer(c.frame, np.uint8)
        for j in range(len(c.cuts) - 1):
            got, (n, in_used, status, last) = walk(buf, c.cuts[j], len(c.frame) - c.cuts[j])
            assert (n, in_used, status, last) == (len(c.cuts) - 1 - j, c.cuts[-1] - c.cuts[j], P.OK, 1), (c.name, j)
            assert [g[0] for g in got] == [x - c.cuts[j] for x in c.cuts[j:-1]], (c.name, j)
        seen += 1
    assert seen > 60


def test_reserved_type_and_oversized_blocks_are_errors_and_a_cut_block_never_is():
    walk = Walk(8)
    raw = lambda n, last=0: ((n << 3) | last).to_bytes(3, "little") + bytes(n)  # noqa: E731
    reserved = ((3 << 3) | (3 << 1) | 1).to_bytes(3, "little") + b"xyz"
    data = np.frombuffer(raw(5) + raw(7) + reserved, np.uint8)
    for length in range(len(data) + 1):
        rows, (n, in_used, status, last) = walk(data, 0, length)
        whole = (length >= 8) + (length >= 18)
        seen_header = whole == 2 and length >= 21  # the verdict needs the three header bytes
        assert (n, in_used, status, last) == (whole, (0, 8, 18)[whole], P.BAD_HEADER if seen_header else P.TRUNCATED, 0), length
    # Block_Size against Block_Maximum_Size, for every type; the size itself is legal
    for btype in (0, 1, 2):
        for size, bad in ((1024, False), (1025, True)):
            body = bytes(1 if btype == 1 else size)
            data = np.frombuffer(raw(5) + ((size << 3) | (btype << 1) | 1).to_bytes(3, "little") + body, np.uint8)
            rows, (n, in_used, status, last) = walk(data, 0, len(data), block_max=1024)
            assert (n, in_used, status, last) == ((1, 8, P.BAD_HEADER, 0) if bad else (2, len(data), P.OK, 1)), (btype, size)
            rows, summ = walk(data, 0, len(data) - 1, block_max=1024)  # cut: the header alone decides
            assert summ == ((1, 8, P.BAD_HEADER, 0) if bad else (1, 8, P.TRUNCATED, 0)), (btype, size)
    # more blocks than the walk follows
    data = np.frombuffer(bytes(3) * 5, np.uint8)
    import compu_amd
    from compu_amd.api import _ZstdSlabSummary

    s = _ZstdSlabSummary()
    assert compu_amd.lib().chip_zstd_slab_blocks_host(C.c_void_p(data.ctypes.data), len(data), 1024, 0, None, C.byref(s)) == 0
    assert (s.n_blocks, s.in_used, s.status) == (5, 15, P.TRUNCATED)
    assert compu_amd.lib().chip_zstd_slab_blocks_host(None, 5, 1024, 0, None, C.byref(s)) == -101
    assert compu_amd.lib().chip_zstd_slab_blocks_host(C.c_void_p(data.ctypes.data), len(data), 1024, 0, None, None) == -101
    blocks, summ = compu_amd.zstd_slab_blocks_host(bytes(data), 1024)
    assert len(blocks) == 5 and summ.as_tuple() == (5, 15, P.TRUNCATED, 0)


# ---- the header step ----
def header(data, wlog=0, checksum=True):
    import compu_amd

    return compu_amd.zstd_cursor_header_host(data, wlog, checksum)


def header_frames():
    out = [(c.name, c.frame) for c in P.form_cases() + [P.three_block_frame()]]
    out += [(c.name, c.frame) for c in Z.header_cases() if c.frame[:4] == W.MAGIC]
    return out


@pytest.mark.parametrize("name,frame", header_frames(), ids=[f[0] for f in header_frames()])
def test_header_step_against_the_block_description(name, frame):
    import compu_amd
    from compu_amd.api import _ZstdCursor

    _, bs = compu_amd.zstd_blocks_host(frame)
    hs = P.py_blocks(frame)[1][6]
    did_bytes = (0, 1, 2, 4)[bs.descriptor & 3]
    did_at = 5 + (0 if bs.descriptor & 0x20 else 1)
    did = int.from_bytes(frame[did_at:did_at + did_bytes], "little")
    rc, cur, hb, need = header(frame, 31)
    if bs.descriptor & 8:
        want = -14
    elif bs.window_size > 1 << 31:
        want = -16
    elif did:
        want = -32
    else:
        want = FINISHED
    assert rc == want
    if rc == FINISHED:
        assert (hb, cur.in_total, cur.out_total, cur.window_size, cur.content_size, cur.descriptor) == (hs, hs, 0, bs.window_size, bs.content_size, bs.descriptor)
        assert (cur.phase, list(cur.rep), cur.hist, cur.ring, cur.waived, cur.error, list(cur.carry_len)) == (1, [1, 4, 8], 0, 0, 0, 0, [0] * 4)
        assert need == compu_amd.ZCUR_CARRY_BYTES + bs.window_size
        assert header(frame, 31, checksum=False)[1].waived == 1
    else:
        assert (cur.phase, cur.error) == (4, want)
    # a header cut at every byte: NeedInput and no progress (a magic that is whole and wrong is judged at once)
    for n in range(hs):
        rc, cur, hb, need = header(frame[:n], 31)
        assert (rc, hb, need) == (NEED_INPUT, 0, 0) and bytes(cur) == bytes(_ZstdCursor()), n


def test_need_state_and_the_window_limit_for_windows_from_1_kib_up():
    import compu_amd

    for e in range(0, 22):
        for m in (0, 3, 7):
            f = W.Frame(fcs=None, window=(e, m))
            f.raw(b"x", last=True)
            frame, _ = f.finish()
            window = W.window_size(e, m)
            for wlog in (0, 10, 20, 27, 31):
                rc, cur, hb, need = header(frame, wlog)
                if window > 1 << (wlog or 27):
                    assert (rc, cur.phase, cur.error) == (-16, 4, -16), (e, m, wlog)
                else:
                    assert (rc, hb, need, cur.window_size) == (FINISHED, 6, compu_amd.ZCUR_CARRY_BYTES + window, window), (e, m, wlog)
    # Single_Segment: the window is the content size
    for n, ok in ((1 << 27, True), ((1 << 27) + 1, False)):
        frame = W.MAGIC + bytes([0xE0]) + n.to_bytes(8, "little")
        rc, cur, hb, need = header(frame)
        assert rc == (FINISHED if ok else -16)
        if ok:
            assert (cur.window_size, cur.content_size, need) == (n, n, compu_amd.ZCUR_CARRY_BYTES + n)
    # a window exponent beyond 31 is too large whatever the limit
    assert header(W.MAGIC + bytes([0x00, 22 << 3]) + b"\1\0\0", 31)[0] == -16


def test_dictionary_id_reserved_bit_magic_and_arguments():
    import compu_amd
    from compu_amd.api import _ZstdCursor

    for b in (1, 2, 4):
        for v, want in ((0, FINISHED), (1, -32), ((1 << (8 * b)) - 1, -32)):
            f = W.Frame(dict_id=(v, b))
            f.raw(b"abc", last=True)
            assert header(f.finish()[0])[0] == want
    f = W.Frame(reserved_bit=True)
    f.raw(b"abc", last=True)
    assert header(f.finish()[0])[0] == -14
    assert header(b"abcd")[0] == -10 and header(W.skippable(b"abc"))[0] == -10 and header(W.MAGIC[:3])[0] == NEED_INPUT
    lib = compu_amd.lib()
    cur, hb, need = _ZstdCursor(), C.c_uint32(), C.c_uint64()
    data = np.frombuffer(W.MAGIC + b"\x20\x00", np.uint8)
    p = C.c_void_p(data.ctypes.data)
    assert lib.chip_zstd_cursor_header_host(None, p, 6, 0, 0, C.byref(hb), C.byref(need)) == -101
    assert lib.chip_zstd_cursor_header_host(C.byref(cur), None, 6, 0, 0, C.byref(hb), C.byref(need)) == -101
    assert lib.chip_zstd_cursor_header_host(C.byref(cur), p, 6, 0, 2, C.byref(hb), C.byref(need)) == -101
    assert lib.chip_zstd_cursor_header_host(C.byref(cur), p, 6, 32, 0, C.byref(hb), C.byref(need)) == -101
    assert lib.chip_zstd_cursor_header_host(C.byref(cur), p, 6, 0, 0, C.byref(hb), C.byref(need)) == FINISHED
    assert lib.chip_zstd_cursor_header_host(C.byref(cur), p, 6, 0, 0, C.byref(hb), C.byref(need)) == -101  # the cursor has left HEADER


def test_the_device_call_refuses_bad_arguments_before_it_looks_for_a_device():
    import compu_amd
    from compu_amd.api import _ZstdCursor, _ZstdNextSummary

    call = compu_amd.lib().chip_zstd_parallel_next
    s, p = _ZstdNextSummary(), C.c_void_p(4096)  # (never dereferenced: every call here is refused)

    def rc(cur=None, state=p, cap=1 << 20, inp=p, n=10, out=p, ocap=10, wlog=0, flags=0, summ=s):
        return call(C.byref(cur if cur is not None else _ZstdCursor()), state, cap, inp, n, out, ocap, wlog, flags, C.byref(summ) if summ is not None else None, None)

    assert call(None, p, 1 << 20, p, 10, p, 10, 0, 0, C.byref(s), None) == -101
    assert rc(state=None) == -101 and rc(inp=None) == -101 and rc(out=None) == -101 and rc(summ=None) == -101
    assert rc(n=(1 << 31) + 1) == -101 and rc(ocap=1 << 31) == -101 and rc(flags=2) == -101 and rc(wlog=32) == -101 and rc(wlog=-1) == -101

    def blocks_cursor(**kw):
        c = _ZstdCursor()
        c.phase, c.window_size, c.content_size, c.in_total = 1, 1024, P.UNSIZED, 6
        c.rep[0], c.rep[1], c.rep[2] = 1, 4, 8
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert rc(cur=blocks_cursor(phase=5)) == -101
    assert rc(cur=blocks_cursor(out_total=100, hist=99, ring=100)) == -101
    assert rc(cur=blocks_cursor(out_total=5000, hist=1024, ring=5000 % 1024 + 1)) == -101
    c = blocks_cursor()
    c.carry_len[2] = compu_amd.api.ZCUR_SLOT_BYTES
    assert rc(cur=c) == -101
    c = blocks_cursor()
    c.xxh.tail_n = 32
    assert rc(cur=c) == -101
    c = blocks_cursor()
    c.rep[1] = 0
    assert rc(cur=c) == -101
    assert rc(cur=blocks_cursor(waived=1), flags=0) == -101 and rc(cur=blocks_cursor(waived=0), flags=1) == -101  # the flag changed mid-frame
    c = _ZstdCursor()
    c.out_total = 1
    assert rc(cur=c) == -101  # HEADER with content in front of it


# ---- XXH64 ----
def libzstd_checksum(z, data):
    import zstd_ref

    return int.from_bytes(zstd_ref.compress(z, data, 1, True, True)[-4:], "little")


def digest_of(pieces):
    import compu_amd

    x = compu_amd.Xxh64()
    for p in pieces:
        x.update(p)
    return x.digest()


def split_digests(data):
    """the digest of data fed as data[:k] and data[k:], for EVERY k in 0 .. len(data): two updates of a fresh state each"""
    import compu_amd
    from compu_amd.api import _Xxh64State

    lib, st = compu_amd.lib(), _Xxh64State()
    buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
    base, n, p_st, size = buf.ctypes.data, len(data), C.byref(st), C.sizeof(_Xxh64State)
    update, digest, out = lib.chip_xxh64_update_host, lib.chip_xxh64_digest_host, []
    for k in range(n + 1):
        C.memset(p_st, 0, size)
        assert update(p_st, C.c_void_p(base), k) == 0 and update(p_st, C.c_void_p(base + k), n - k) == 0
        out.append(digest(p_st))
    return out


def check_content(z, rnd, data):
    from oracle import oracle as O

    n = len(data)
    want = libzstd_checksum(z, data)
    assert O.xxh64(data) & 0xFFFFFFFF == want
    assert digest_of([data]) & 0xFFFFFFFF == want and digest_of([data]) == O.xxh64(data), n
    got = split_digests(data)
    assert len(got) == n + 1
    wrong = [k for k, d in enumerate(got) if d & 0xFFFFFFFF != want]
    assert not wrong, (n, wrong[:5])
    for _ in range(3):
        pieces, at = [], 0
        while at < n:
            k = rnd.randrange(1, 98)
            pieces.append(data[at:at + k])
            at += k
        assert digest_of(pieces) & 0xFFFFFFFF == want, n


def test_xxh64_of_0_to_200_bytes_in_every_two_way_split_and_in_random_pieces():
    import zstd_ref

    z = zstd_ref.load()
    assert z is not None
    rnd = random.Random(64)
    for n in range(201):
        check_content(z, rnd, rnd.randbytes(n))


@pytest.mark.parametrize("n", [99991, 100000, 100032, 131072 + 17])
def test_xxh64_of_about_100_kb_in_every_two_way_split_and_in_random_pieces(n):
    import zstd_ref

    z = zstd_ref.load()
    assert z is not None
    rnd = random.Random(n)
    check_content(z, rnd, rnd.randbytes(n))


def test_a_state_copied_mid_way_gives_the_same_digest():
    import compu_amd

    rnd = random.Random(65)
    data = rnd.randbytes(5000)
    for k in (0, 1, 31, 32, 33, 2500, 4999, 5000):
        a = compu_amd.Xxh64().update(data[:k])
        mid = a.digest()
        b = a.copy()
        assert b.digest() == mid == a.digest()  # the digest leaves the state usable
        a.update(data[k:])
        b.update(data[k:k + 100]).update(data[k + 100:])
        assert a.digest() == b.digest() == digest_of([data])
    lib = compu_amd.lib()
    assert lib.chip_xxh64_update_host(None, None, 0) == -101 and lib.chip_xxh64_update_host(C.byref(compu_amd.Xxh64().raw), None, 5) == -101


def test_struct_layouts():
    from compu_amd.api import _Xxh64State, _ZstdCursor, _ZstdNextSummary, _ZstdSlabSummary

    assert (C.sizeof(_Xxh64State), C.sizeof(_ZstdCursor), C.sizeof(_ZstdNextSummary), C.sizeof(_ZstdSlabSummary)) == (80, 208, 56, 24)
    assert _ZstdCursor.xxh.offset == 128 and _ZstdCursor.carry_len.offset == 80 and _ZstdCursor.phase.offset == 108
