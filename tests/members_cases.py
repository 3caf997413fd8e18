"""Units for CHIP_F_MEMBERS: series of gzip members and of zstd frames, built with zlib / gzip, tests/deflate_writer.py,
tests/zstd_writer.py and the golden files.  A case is (name, format, unit bytes, cap or None = ample); what it must answer comes from
tests/members_ref.py.  Shared by tests/test_members_cpu.py and tests/test_members_gpu.py."""
import random
import zlib
from collections import namedtuple

import deflate_writer as D
import zstd_writer as W
from conftest import golden
from zstd_writer import new_offset as N

GZIP, AUTO, ZSTD = 31, 47, 100
Case = namedtuple("Case", "name fmt unit cap")

LENGTHS = (0, 1, 15, 16, 17, 65, 100000)  # the last crosses the 32 KiB window and has several blocks


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=31):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(data) + c.flush()


def payload(n, seed=0):
    alice = golden("alice29.txt")
    s = (seed * 7919) % 40000
    return alice[s:s + n]


def gz_kind(data, kind):
    """kind: stored, fixed or dynamic blocks"""
    if kind == "stored":
        return gz(data, 0)
    if kind == "fixed":
        return gz(data, 6, zlib.Z_FIXED)
    return gz(data, 6)


def wgz(tokens_or_deflate, **kw):
    d = tokens_or_deflate if isinstance(tokens_or_deflate, D.Deflate) else D.Deflate().fixed(tokens_or_deflate, final=True)
    return D.wrap(d, "gzip", **kw).data


def zframe(data, checksum=False, fcs=True, kind="raw"):
    """one zstd frame of hand-written blocks: raw, rle (data = one byte repeated) or compressed (raw literals + one match)"""
    f = W.Frame(fcs=fcs, window=None if fcs else (10, 0), checksum=checksum)
    if kind == "rle":
        f.rle(data[0], len(data), last=True)
    elif kind == "compressed":
        f.compressed(data, [(len(data), 7, N(len(data)))], last=True)
    elif len(data) > 60000:
        for k in range(0, len(data), 60000):
            f.raw(data[k:k + 60000], last=k + 60000 >= len(data))
    else:
        f.raw(data, last=True)
    return f.finish()


def shape_cases():
    out = []
    rnd = random.Random(5)
    # every length, every block kind, as 1, 2, 3 and 8 members
    for kind in ("stored", "fixed", "dynamic"):
        members = [gz_kind(payload(n, i), kind) for i, n in enumerate(LENGTHS)]
        for count in (1, 2, 3, 8):
            pick = [members[rnd.randrange(len(members) - 1)] for _ in range(count)]
            out.append(Case(f"gzip_{kind}_{count}", GZIP, b"".join(pick), None))
        out.append(Case(f"gzip_{kind}_all_lengths", GZIP, b"".join(members), None))
    long_, short = gz(payload(100000, 3)), gz(payload(17, 4))
    out.append(Case("gzip_long_short", GZIP, long_ + short, None))
    out.append(Case("gzip_short_long", GZIP, short + long_, None))
    out.append(Case("gzip_long_long_auto", AUTO, long_ + gz(payload(100000, 9), 1), None))
    # headers with every optional field between members (a BGZF-like extra field with a foreign subfield among them)
    fancy = wgz([104, 105], header=D.gzip_header(extra=b"BC\x02\x00\x1b\x00XY\x01\x00z", name=b"n", comment=b"c", hcrc=True))
    out.append(Case("gzip_header_fields", GZIP, short + fancy + fancy + short, None))
    out.append(Case("gzip_empty_unit", GZIP, b"", None))
    return out


def base_reset_cases():
    m1 = gz(b"abcdefgh" * 4)
    ok = wgz([97, 98, 99, ("m", 3, 3)])  # the first match reaches the member's own first byte
    bad = wgz([97, 98, 99, ("m", 3, 4)])  # one byte further: member 1's last byte lies there
    out = [Case("gzip_distance_to_member_start", GZIP, m1 + ok, None), Case("gzip_distance_past_member_start", GZIP, m1 + bad, None)]
    f1, _ = W.Frame(checksum=True).compressed(b"0123456789", [(10, 6, N(7)), (0, 4, N(9))], last=True).finish()
    zok, _ = W.Frame().compressed(b"xy", [(2, 10, N(2))], last=True).finish()
    zbad, _ = W.Frame().compressed(b"xy", [(2, 10, N(3))], last=True, invalid=1).finish()
    out.append(Case("zstd_offset_to_frame_start", ZSTD, f1 + zok, None))
    out.append(Case("zstd_offset_past_frame_start", ZSTD, f1 + zbad, None))
    # a second frame's first sequences use the repeat offsets: they are the initial 1 / 4 / 8, not frame 1's 9 / 7
    for ov, ll in ((1, 4), (2, 4), (3, 8)):
        f2, _ = W.Frame(checksum=True).compressed(b"ABCDEFGHIJ"[:ll + 1], [(ll, 5, ov), (1, 3, N(2))], last=True).finish()
        out.append(Case(f"zstd_repeat_offset_{ov}", ZSTD, f1 + f2, None))
    return out


def tail_cases():
    m = gz(payload(65, 1))
    m2 = gz(payload(1000, 2))
    out = []
    for name, tail in (("nothing", b""), ("zero1", b"\0"), ("zero2", b"\0\0"), ("zero7", b"\0" * 7), ("lone_1f", b"\x1f"), ("magic_only", b"\x1f\x8b"),
                       ("bad_method", b"\x1f\x8b\x07" + b"\0" * 20), ("cut_header", m2[:6]), ("cut_body", m2[:len(m2) // 2]), ("cut_trailer", m2[:-3]),
                       ("zlib_behind", zlib.compress(b"zlib stream")), ("reserved_flag", b"\x1f\x8b\x08\xe0" + b"\0" * 20)):
        out.append(Case(f"gzip_then_{name}", GZIP, m + tail, None))
        out.append(Case(f"gzip2_then_{name}", AUTO, m + m2 + tail, None))
    out.append(Case("auto_zlib_then_gzip", AUTO, zlib.compress(payload(300, 5)) + m, None))
    return out


def zstd_cases():
    out = []
    alice_z = golden("alice29.txt.compressed.zstd")
    xy_z = golden("10x10y.compressed.zstd")
    rnd = random.Random(8)
    frames = [zframe(payload(n, 20 + i), checksum=bool(i & 1), fcs=bool(i & 2))[0] for i, n in enumerate(LENGTHS)]
    frames.append(zframe(b"r" * 300, kind="rle")[0])
    frames.append(zframe(b"compressed block", checksum=True, kind="compressed")[0])
    empty = W.Frame().raw(b"", last=True).finish()[0]
    skip = W.skippable(b"seek table", 14)
    for count in (1, 2, 3, 8):
        out.append(Case(f"zstd_{count}", ZSTD, b"".join(frames[rnd.randrange(len(frames))] for _ in range(count)), None))
    out.append(Case("zstd_all", ZSTD, b"".join(frames), None))
    out.append(Case("zstd_golden", ZSTD, alice_z + xy_z + alice_z, None))
    out.append(Case("zstd_empty_frames", ZSTD, empty + frames[3] + empty + empty, None))
    out.append(Case("zstd_skippable_first", ZSTD, skip + frames[2], None))
    out.append(Case("zstd_skippable_between", ZSTD, frames[2] + skip + W.skippable(b"") + frames[5], None))
    out.append(Case("zstd_skippable_last", ZSTD, xy_z + skip, None))
    out.append(Case("zstd_skippable_alone", ZSTD, skip + W.skippable(b"", 0), None))
    out.append(Case("zstd_empty_unit", ZSTD, b"", None))
    for k in (1, 2, 3):
        out.append(Case(f"zstd_stray_{k}", ZSTD, frames[4] + xy_z + b"\x28\xb5\x2f"[:k], None))
    out.append(Case("zstd_cut_magic_only", ZSTD, frames[4] + b"\x28\xb5\x2f\xfd", None))
    out.append(Case("zstd_cut_second", ZSTD, frames[4] + alice_z[:5000], None))
    out.append(Case("zstd_cut_skippable", ZSTD, frames[4] + skip[:9], None))
    out.append(Case("zstd_gzip_behind", ZSTD, frames[4] + gz(b"gzip"), None))
    return out


def damage_cases():
    """damage in member k of 3: a wrong CRC, a wrong ISIZE, an invalid code; zstd: a wrong XXH64, a reserved block"""
    out = []
    datas = [payload(700, 31), payload(40000, 32), payload(65, 33)]
    good = [gz(d) for d in datas]
    for k in range(3):
        crc = bytearray(good[k]); crc[-8] ^= 1
        isz = bytearray(good[k]); isz[-1] ^= 0x40
        inv = wgz(D.Deflate().fixed(list(datas[k][:50]) + [("s", 286)], final=True))  # a literal/length code that does not exist
        for name, m in (("crc", bytes(crc)), ("isize", bytes(isz)), ("code", inv)):
            out.append(Case(f"gzip_bad_{name}_in_{k + 1}", GZIP, b"".join(good[:k]) + m + b"".join(good[k + 1:]), None))
    zgood = [zframe(d, checksum=True)[0] for d in datas]
    for k in range(3):
        f = W.Frame(checksum=True)
        f.raw(datas[k], last=True)
        xxh = f.finish(checksum_value=0x12345678)[0]
        res = W.Frame().raw(datas[k][:100]).reserved().finish()[0]
        for name, m in (("xxh64", xxh), ("block", res)):
            out.append(Case(f"zstd_bad_{name}_in_{k + 1}", ZSTD, b"".join(zgood[:k]) + m + b"".join(zgood[k + 1:]), None))
    return out


def capacity_cases():
    out = []
    datas = [payload(5000, 41), payload(70000, 42), payload(17, 43)]
    total, first = sum(len(d) for d in datas), len(datas[0])
    g = b"".join(gz(d) for d in datas)
    z = b"".join(zframe(d, checksum=True)[0] for d in datas) + golden("10x10y.compressed.zstd")
    ztotal = total + len(golden("10x10y"))
    for cap_name, cap, zcap in (("total", total, ztotal), ("total_less_1", total - 1, ztotal - 1), ("member1", first, first), ("zero", 0, 0)):
        out.append(Case(f"gzip_cap_{cap_name}", GZIP, g, cap))
        out.append(Case(f"zstd_cap_{cap_name}", ZSTD, z, zcap))
    return out


def all_cases():
    return shape_cases() + base_reset_cases() + tail_cases() + zstd_cases() + damage_cases() + capacity_cases()
