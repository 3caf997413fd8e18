"""Buffers of zstd frames for the frame-index tests (chip_zstd_plan_host, chip_zstd_plan, chip_layout_units): the serial walk of
include/compu_hip.h restated in Python -- the expectation of every test -- and the named cases, built with tests/zstd_writer.py and
the tests/golden/*.zstd files.  A case is (name, buffer); `decodable()` adds the content of those whose frames all decode."""
import ctypes as C
import functools
import random

import numpy as np

import zstd_writer as W
from conftest import golden
from zstd_writer import new_offset as N

OK, TRUNCATED, BAD_HEADER, TOO_LARGE = 0, 1, 2, 3
UNSIZED = 0xFFFFFFFF
MAX_BLOCKS = 1 << 20
MAGIC = W.MAGIC


def _le(d, at, n):
    return int.from_bytes(d[at:at + n], "little")


def walk(d, max_frames=None):
    """The plan of `d` by definition: (rows of (in_off, in_len, out_off, out_cap) cut to max_frames,
    (n_frames, n_skippable, n_unsized, total_out, in_used, status))."""
    ln, p, rows, skipped, unsized, total = len(d), 0, [], 0, 0, 0

    def stop(status):
        return rows[:len(rows) if max_frames is None else max_frames], (len(rows), skipped, unsized, total, p, status)

    while True:
        if p == ln:
            return stop(OK)
        if ln - p < 4:
            return stop(TRUNCATED)
        m = _le(d, p, 4)
        if 0x184D2A50 <= m <= 0x184D2A5F:
            if ln - p < 8:
                return stop(TRUNCATED)
            s = _le(d, p + 4, 4)
            if s > ln - p - 8:
                return stop(TRUNCATED)
            skipped += 1
            p += 8 + s
            continue
        if m != 0xFD2FB528:
            return stop(BAD_HEADER)
        if ln - p < 5:
            return stop(TRUNCATED)
        fhd = d[p + 4]
        f, ss, dd = fhd >> 6, (fhd >> 5) & 1, fhd & 3
        fcs_bytes = ss if f == 0 else (0, 2, 4, 8)[f]
        fcs_at = 5 + (0 if ss else 1) + (0, 1, 2, 4)[dd]
        hs = fcs_at + fcs_bytes
        if ln - p < hs:
            return stop(TRUNCATED)
        fcs = None if fcs_bytes == 0 else _le(d, p + fcs_at, fcs_bytes) + (256 if fcs_bytes == 2 else 0)
        q, blocks = p + hs, 0
        while True:
            if ln - q < 3:
                return stop(TRUNCATED)
            h = _le(d, q, 3)
            btype = (h >> 1) & 3
            if btype == 3:
                return stop(BAD_HEADER)
            blocks += 1
            if blocks > MAX_BLOCKS:
                return stop(TOO_LARGE)
            body = 1 if btype == 1 else h >> 3
            if body > ln - q - 3:
                return stop(TRUNCATED)
            q += 3 + body
            if h & 1:
                break
        if fhd & 4:
            if ln - q < 4:
                return stop(TRUNCATED)
            q += 4
        if q - p > 0xFFFFFFFF or (fcs is not None and fcs >= 0xFFFFFFFF):
            return stop(TOO_LARGE)
        rows.append((p, q - p, total, UNSIZED if fcs is None else fcs))
        if fcs is None:
            unsized += 1
        else:
            total += fcs
        p = q


# ---- frames ---------------------------------------------------------------------------------------

def text(n, seed=0):
    alice = golden("alice29.txt")
    s = (seed * 7919) % 40000
    return alice[s:s + n]


def raw_frame(data, block=60000, **kw):
    f = W.Frame(**kw)
    if not data:
        return f.raw(b"", last=True).finish()[0]
    for k in range(0, len(data), block):
        f.raw(data[k:k + block], last=k + block >= len(data))
    return f.finish()[0]


def unsized_frame(data, **kw):
    return raw_frame(data, fcs=None, window=(10, 0), **kw)


NINE = raw_frame(b"")  # magic, descriptor, a 1-byte Frame_Content_Size of 0, one empty raw block: the smallest frame
assert len(NINE) == 9


@functools.lru_cache(maxsize=None)
def _parts():
    """frames that decode, with their content: (frame, content) by name"""
    t = text
    out = {}
    out["fcs1"] = (raw_frame(t(200, 1)), t(200, 1))
    out["fcs1_zero"] = (NINE, b"")
    out["fcs2_plus256"] = (raw_frame(t(256, 2), fcs=2), t(256, 2))  # the field holds 0
    out["fcs2"] = (raw_frame(t(3000, 3), fcs=2, checksum=True), t(3000, 3))
    out["fcs4"] = (raw_frame(t(70000, 4), fcs=4), t(70000, 4))  # two blocks
    out["fcs8"] = (raw_frame(t(500, 5), fcs=8, checksum=True), t(500, 5))
    out["fcs4_windowed"] = (raw_frame(t(900, 6), fcs=4, window=(10, 0)), t(900, 6))
    out["fcs8_windowed_checksum"] = (raw_frame(t(1000, 7), fcs=8, window=(12, 3), checksum=True), t(1000, 7))
    out["unsized"] = (unsized_frame(t(777, 8)), t(777, 8))
    out["unsized_checksum_blocks"] = (unsized_frame(t(2500, 9), block=1000, checksum=True), t(2500, 9))
    out["unsized_empty"] = (unsized_frame(b""), b"")
    f = W.Frame(checksum=True).rle(0x41, 300).raw(b"between").rle(0x42, 1, last=True)
    out["rle_raw_rle"] = f.finish()
    f = W.Frame().compressed(b"0123456789", [(10, 6, N(7)), (0, 4, N(9))]).raw(b"tail", last=True)
    out["compressed_raw"] = f.finish()
    f = W.Frame(fcs=None, window=(10, 0), checksum=True).compressed(b"xy", [(2, 10, N(2))], last=True)
    out["unsized_compressed"] = f.finish()
    out["golden_alice"] = (golden("alice29.txt.compressed.zstd"), golden("alice29.txt"))
    out["golden_xy"] = (golden("10x10y.compressed.zstd"), golden("10x10y"))
    return out


def part(name):
    return _parts()[name][0]


def _dict_frames():
    """every Dictionary_ID width, value 0 ("no dictionary"): the plan only has to step over the field"""
    return [raw_frame(text(50 + b, b), dict_id=(0, b)) for b in (1, 2, 4)] + [raw_frame(text(60, 3), fcs=None, window=(10, 0), dict_id=(0x1234, 2))]


@functools.lru_cache(maxsize=None)
def shape_files():
    P = {k: v[0] for k, v in _parts().items()}
    sized = [P[k] for k in ("fcs1", "fcs1_zero", "fcs2_plus256", "fcs2", "fcs4", "fcs8", "fcs4_windowed", "fcs8_windowed_checksum", "rle_raw_rle",
                            "compressed_raw", "golden_alice", "golden_xy")]
    skip = W.skippable(b"seek table", 14)
    out = [("empty", b""), ("one_frame", P["fcs1"]), ("nine_bytes", NINE)]
    out += [(k, P[k]) for k in P if k not in ("fcs1", "fcs1_zero")]
    out.append(("all_sized", b"".join(sized)))
    out.append(("mixed_sized_unsized", P["unsized"] + P["fcs2"] + P["unsized_compressed"] + P["unsized_empty"] + P["fcs4"] + P["unsized_checksum_blocks"]))
    out.append(("dict_id_widths", b"".join(_dict_frames())))
    out.append(("skippable_first", skip + P["fcs2"]))
    out.append(("skippable_between", P["fcs1"] + skip + W.skippable(b"") + P["fcs8"]))
    out.append(("skippable_last", P["golden_xy"] + skip))
    out.append(("skippable_alone", skip + W.skippable(b"", 0)))
    out.append(("skippable_every_magic", b"".join(W.skippable(bytes(k), k) + (P["fcs1"] if k % 5 == 0 else b"") for k in range(16))))
    frames = [P["fcs2"], P["unsized"], P["golden_xy"], P["rle_raw_rle"]]
    out.append(("pzstd_style", b"".join(W.skippable(len(f).to_bytes(4, "little")) + f for f in frames)))
    return out


def _cut_points():
    """a victim frame (windowed, 2-byte dictionary ID, 4-byte content size, two blocks, checksum) and where to cut it"""
    f = W.Frame(fcs=4, window=(10, 0), dict_id=(0, 2), checksum=True).raw(text(40, 1)).rle(0x55, 9, last=True)
    v = f.finish()[0]
    hs = len(f.header())
    assert hs == 12 and len(v) == hs + 3 + 40 + 3 + 1 + 4
    cuts = {"in_magic_1": 1, "in_magic_3": 3, "after_magic": 4, "after_descriptor": 5, "in_header": hs - 1, "after_header": hs, "in_block_header": hs + 2,
            "after_block_header": hs + 3, "in_block_body": hs + 20, "in_second_block_header": hs + 43 + 1, "before_rle_byte": hs + 43 + 3,
            "before_checksum": len(v) - 4, "in_checksum": len(v) - 1}
    return v, cuts


@functools.lru_cache(maxsize=None)
def stop_files():
    """(name, bytes): each stop once at position 0 (@0) and once behind three frames and a skippable frame (@3)"""
    P = {k: v[0] for k, v in _parts().items()}
    lead = P["fcs1"] + P["unsized"] + W.skippable(b"xyz", 3) + P["fcs2"]
    v, cuts = _cut_points()
    skip = W.skippable(b"0123456789", 7)
    stops = {f"cut_{k}": v[:c] for k, c in cuts.items()}
    stops.update({f"cut_skippable_{c}": skip[:c] for c in (4, 5, 7, 8, 12, 17)})
    stops.update({f"trailing_{k}": b"\x00\x01\x02"[:k] for k in (1, 2, 3)})
    stops.update({f"stray_magic_{k}": MAGIC[:k] for k in (1, 2, 3)})
    stops["trailing_4_no_magic"] = b"\x00\x00\x00\x00"
    stops["trailing_gzip"] = b"\x1f\x8b\x08\x00" + bytes(14)
    stops["near_magic"] = b"\x28\xb5\x2f\xfc" + NINE[4:]
    stops["skippable_range_end"] = (0x184D2A60).to_bytes(4, "little") + bytes(8)
    stops["skippable_range_start"] = (0x184D2A4F).to_bytes(4, "little") + bytes(8)
    stops["block_type_3"] = W.Frame().raw(text(100, 2)).reserved().finish()[0] + NINE
    stops["block_type_3_first"] = W.Frame(fcs=None, window=(10, 0)).reserved(b"").finish()[0]
    stops["fcs_ffffffff"] = raw_frame(b"abc", fcs=4, fcs_value=0xFFFFFFFF) + NINE
    stops["fcs8_2_pow_32"] = raw_frame(b"abc", fcs=8, fcs_value=1 << 32) + NINE
    stops["fcs_ffffffff_cut"] = raw_frame(b"abc", fcs=4, fcs_value=0xFFFFFFFF)[:-1]  # the cut is met first
    stops["skippable_size_past_end"] = (0x184D2A50).to_bytes(4, "little") + (0xFFFFFFFF).to_bytes(4, "little") + bytes(40)
    out = []
    for name, f in stops.items():
        out.append((name + "@0", f))
        out.append((name + "@3", lead + f))
    out.append(("fcs_fffffffe_is_fine", lead + raw_frame(b"abc", fcs=4, fcs_value=0xFFFFFFFE) + NINE))
    return out


@functools.lru_cache(maxsize=None)
def block_cap_files():
    """frames of empty raw blocks (about 3 MiB each): 2^20 blocks are followed, one more is TOO_LARGE"""
    head = MAGIC + b"\x00\x00"  # no content size, window descriptor 0
    at_cap = head + b"\x00\x00\x00" * (MAX_BLOCKS - 1) + b"\x01\x00\x00"
    over = head + b"\x00\x00\x00" * MAX_BLOCKS + b"\x01\x00\x00"
    return [("blocks_2_pow_20", NINE + at_cap + NINE), ("blocks_2_pow_20_plus_1", NINE + over + NINE)]


def _host_raw(parts, tail=b"", **kw):
    """a frame of ONE raw block whose data is the concatenation of `parts`, no checksum: (frame, [offset of each part in it])"""
    f = W.Frame(**kw).raw(b"".join(parts), last=True)
    frame = f.finish()[0]
    at, offs = len(f.header()) + 3, []
    for p in parts:
        offs.append(at)
        at += len(p)
    return frame + tail, offs


@functools.lru_cache(maxsize=None)
def decoy_files():
    """name -> bytes: magic numbers inside block data that the walk never visits (the last one aside)"""
    P = {k: v[0] for k, v in _parts().items()}
    fill = text(120, 7)
    out = {}
    out["magic_in_raw_block"] = P["fcs1"] + _host_raw([fill, MAGIC, fill, MAGIC + b"\x20", fill])[0] + P["fcs2"]
    out["frame_in_raw_block"] = P["fcs1"] + _host_raw([fill, P["fcs2"], fill, P["unsized"], NINE, fill])[0] + P["fcs8"]
    # the embedded frames are the last bytes of the host frame: their chain joins the true one at the next frame
    out["frame_at_end_of_last_block"] = _host_raw([fill, P["fcs8_windowed_checksum"], P["rle_raw_rle"]])[0] + P["fcs1"] + W.skippable(b"s") + NINE
    out["skippable_in_raw_block_past_end"] = _host_raw([fill, (0x184D2A5B).to_bytes(4, "little") + (1 << 30).to_bytes(4, "little"), fill])[0] + P["fcs1"]
    out["skippable_in_raw_block_joins"] = _host_raw([fill, W.skippable(fill[:50], 9)])[0] + P["fcs1"]
    out["cut_frame_in_raw_block"] = _host_raw([fill, P["fcs4"][:300]])[0] + NINE  # the decoy is truncated, the walk is not
    out["first_candidate_not_at_0"] = b"junk" + P["fcs1"] + NINE
    out["first_candidate_not_at_0_short"] = b"\x00" + NINE
    return out


def _pad_to(at, target, nibble=1):
    """skippable frames that move the position from `at` to `target` (target - at >= 8)"""
    assert target - at >= 8
    return W.skippable(bytes(target - at - 8), nibble)


@functools.lru_cache(maxsize=None)
def geometry_files():
    """name -> bytes"""
    P = {k: v[0] for k, v in _parts().items()}
    out = {}
    for shift in (0, 1, 2, 3):  # a frame magic and a skippable magic at 32 - shift and 64 - shift, ..
        d = _pad_to(0, 32 - shift) + P["fcs1"]
        d += _pad_to(len(d), (len(d) + 8 + 15) // 16 * 16 + 16 - shift) + W.skippable(b"abc", 5) + NINE
        out[f"chunk_boundary_shift_{shift}"] = d
    for shift in (1, 2, 3):
        d = P["fcs2"] + _pad_to(len(P["fcs2"]), 16384 - shift) + P["fcs4"]
        d += _pad_to(len(d), 6 * 16384 - shift, 2) + W.skippable(b"", 6) + NINE
        out[f"tile_boundary_shift_{shift}"] = d
    base = P["fcs1"] + P["unsized"]
    for r in (1, 2, 3):
        d = base + W.skippable(bytes((r - len(base) - 8) % 4), 4)  # ends with a skippable frame
        e = base + W.skippable(bytes((r - len(base) - 8 - 9) % 4), 4) + NINE  # ends with a frame
        assert len(d) % 4 == r and len(e) % 4 == r
        out[f"len_mod_4_is_{r}"], out[f"len_mod_4_is_{r}_frame_last"] = d, e
    out["magic_in_last_4_bytes"] = P["fcs1"] + NINE + MAGIC  # a candidate that is cut behind its magic
    out["skippable_magic_in_last_4_bytes"] = P["fcs1"] + NINE + (0x184D2A5F).to_bytes(4, "little")
    out["stray_byte_then_magic_at_end"] = P["fcs1"] + b"\x00" + MAGIC  # a candidate in the last 4 bytes that the walk never reaches
    out["nine_x_300"] = NINE * 300  # more than one 256-thread group of candidates
    out["nine_x_3000"] = NINE * 3000  # two tiles, crosses the 1 024-entry scan partial, 12 doubling levels
    out["nine_x_3000_mixed"] = b"".join((NINE, W.skippable(b"", k % 16), part("unsized_empty"))[k % 3] for k in range(3000))
    # more than 1 024 tiles (16 MiB): frames start on both sides of tile 1 024, whose scan partial of the tile counts is not 0
    r = random.Random(1024)
    out["past_1024_tiles"] = b"".join(raw_frame(r.randbytes(1 << 20)) for _ in range(17)) + NINE
    return out


def all_files():
    return shape_files() + stop_files() + sorted(decoy_files().items()) + sorted(geometry_files().items())


@functools.lru_cache(maxsize=None)
def decodable():
    """(name, buffer, content): buffers whose walk ends OK and whose frames all decode, for the decode tests"""
    C_ = {k: v for k, v in _parts().items()}
    names = list(C_)
    r = random.Random(12)
    out = [("every_part", b"".join(C_[k][0] for k in names), b"".join(C_[k][1] for k in names))]
    sized = [k for k in names if not k.startswith("unsized")]
    out.append(("sized_only", b"".join(C_[k][0] for k in sized), b"".join(C_[k][1] for k in sized)))
    pick = [r.choice(names) for _ in range(40)]
    buf = b"".join(C_[k][0] + (W.skippable(bytes(r.randrange(20)), r.randrange(16)) if r.random() < 0.3 else b"") for k in pick)
    out.append(("forty_with_skippables", buf, b"".join(C_[k][1] for k in pick)))
    small = [k for k in sized if len(C_[k][0]) < 4000]
    pick = [r.choice(small) for _ in range(1100)]  # more than one scan partial of frames
    out.append(("eleven_hundred_sized", b"".join(C_[k][0] for k in pick), b"".join(C_[k][1] for k in pick)))
    for name, buf, content in out:
        assert walk(buf)[1][5] == OK, name
    return out


# ---- calling the library into poisoned arrays ------------------------------------------------------

POISON64, POISON32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def new_summary():
    from compu_amd.api import _ZstdPlanSummary

    return _ZstdPlanSummary(7, 7, 7, 7, 7, 7, 7)


def host_plan(lib, data, max_frames, room):
    """chip_zstd_plan_host into poisoned arrays of `room` entries: (rows written, summary tuple)"""
    buf = np.frombuffer(data, np.uint8)
    arrs = [np.full(room, POISON64, np.uint64), np.full(room, POISON32, np.uint32), np.full(room, POISON64, np.uint64), np.full(room, POISON32, np.uint32)]
    s = new_summary()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.chip_zstd_plan_host(ptr(buf) if len(data) else None, len(data), max_frames, *[ptr(a) if max_frames else None for a in arrs], C.byref(s))
    assert rc == 0
    return check_arrays(arrs, s, max_frames)


def check_arrays(arrs, s, max_frames):
    """Nothing behind min(n_frames, max_frames) is written; returns (rows, summary tuple)."""
    k = min(int(s.n_frames), max_frames)
    assert k <= len(arrs[0])
    for a, poison in zip(arrs, (POISON64, POISON32, POISON64, POISON32)):
        assert (a[k:] == poison).all(), "entries behind min(n_frames, max_frames) were written"
    rows = [tuple(int(a[i]) for a in arrs) for i in range(k)]
    assert int(s.pad) == 0
    return rows, (int(s.n_frames), int(s.n_skippable), int(s.n_unsized), int(s.total_out), int(s.in_used), int(s.status))
