"""Tar images for the plan's tests: archives tarfile writes in its three formats with every name length, member type and the
decoys the walk must not follow, and hand-built images for what tarfile does not write (or writes only one way): base-256 sizes,
pax overrides, a header only the signed checksum accepts, everything the walk refuses, zero blocks and garbage behind the end.
Case: name, data, wellformed (tarfile reads it to the end, and the plan must agree with it), sweep (small enough for a cut at every
block), status (what the plan's summary must say)."""
import functools
import io
import tarfile
from collections import namedtuple

import tar_ref as R

Case = namedtuple("Case", "name data wellformed sweep status")

FORMATS = (("ustar", tarfile.USTAR_FORMAT), ("gnu", tarfile.GNU_FORMAT), ("pax", tarfile.PAX_FORMAT))
NAME_99, NAME_100, NAME_102 = b"a" * 95 + b".dat", b"b" * 96 + b".dat", b"ab/" + b"c" * 99
NAME_241, NAME_300 = b"p" * 140 + b"/" + b"n" * 100, b"q" * 149 + b"/" + b"r" * 150
LINK_200 = b"target/" + b"t" * 193


def noise(n, seed):
    out, x = bytearray(), (seed * 2654435761 + 12345) & 0xFFFFFFFF
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out += x.to_bytes(4, "little")
    return bytes(out[:n])


def header(name=b"f", size=0, typeflag=b"0", linkname=b"", prefix=b"", magic=b"ustar\x0000", mode=0o644, mtime=0o14000000000, size_field=None,
           signed=False, chksum=None):
    """one 512-byte header block; size_field overrides the octal size, chksum the computed one"""
    octal = lambda v, n: (b"%0*o" % (n - 1, v)) + b"\0"  # noqa: E731
    h = bytearray(512)
    h[0:len(name)] = name
    h[100:108], h[108:116], h[116:124] = octal(mode, 8), octal(0, 8), octal(0, 8)
    h[124:136] = size_field if size_field is not None else octal(size, 12)
    h[136:148] = octal(mtime, 12)
    h[148:156] = b" " * 8
    h[156:157] = typeflag
    h[157:157 + len(linkname)] = linkname
    h[257:265] = magic
    h[265:270], h[297:302] = b"owner", b"group"
    h[345:345 + len(prefix)] = prefix
    total = sum(c - 256 if signed and c > 127 else c for c in h)
    h[148:156] = chksum if chksum is not None else b"%06o\0 " % (total & 0o777777)
    return bytes(h)


def padded(body):
    return body + bytes(-len(body) % 512)


def member(name, body=b"", **kw):
    return header(name, len(body), **kw) + padded(body)


def pax_record(key, value):
    n = len(key) + len(value) + 3
    while len(b"%d" % n) + len(key) + len(value) + 3 != n:
        n = len(b"%d" % n) + len(key) + len(value) + 3
    return b"%d %s=%s\n" % (n, key, value)


def ext(typeflag, body, name=b"././@ext"):
    return header(name, len(body), typeflag=typeflag) + padded(body)


END = bytes(1024)


def inner_tar():
    """a complete small archive: as a member's content its headers are aligned decoys that chain among themselves"""
    return member(b"inner/one", b"1" * 700) + member(b"inner/two", b"2" * 30) + ext(b"L", b"inner/long" + b"g" * 120 + b"\0") + member(
        b"inner/short", b"3" * 512) + END


def tarfile_archive(fmt, members_only=None):
    buf = io.BytesIO()
    kw = {"pax_headers": {"comment": "written by the test"}} if fmt == tarfile.PAX_FORMAT else {}
    with tarfile.open(fileobj=buf, mode="w", format=fmt, encoding="utf-8", errors="surrogateescape", **kw) as t:
        def add(name, body=b"", type=tarfile.REGTYPE, linkname=""):
            info = tarfile.TarInfo(name.decode("utf-8", "surrogateescape") if isinstance(name, bytes) else name)
            info.type, info.size, info.linkname, info.mtime, info.mode = type, len(body), linkname, 1600000000, 0o640
            t.addfile(info, io.BytesIO(body))

        for k, n in enumerate((0, 1, 511, 512, 513)):
            add(b"size/%d" % n, noise(n, k))
        for name in (NAME_99, NAME_100, NAME_102, NAME_241):
            add(name, noise(33, len(name)))
        if fmt != tarfile.USTAR_FORMAT:  # (USTAR has no room for them)
            add(NAME_300, noise(65, 300))
            add(b"long/symlink", type=tarfile.SYMTYPE, linkname=LINK_200.decode())
        add(b"dir", type=tarfile.DIRTYPE)
        add(b"dir/symlink", type=tarfile.SYMTYPE, linkname="size/513")
        add(b"dir/hardlink", type=tarfile.LNKTYPE, linkname="size/512")
        add("dir/grüße-世界.txt", b"non-ASCII name\n")
        add(b"nested.tar", inner_tar())
        add(b"ends-in-a-header", noise(512, 9) + header(b"decoy/at-the-end", 4096))
        add(b"after-the-decoy", b"the true next header follows the decoy directly")
        add(b"size/1", b"a repeated name: the last one wins")
    return buf.getvalue()


def many_members(n=3000):
    """n members of one byte: more candidates than a scan workgroup's 1 024, many tiles, 12 doubling levels"""
    return b"".join(member(b"many/%05d" % k, bytes([k & 0xFF])) for k in range(n)) + END


def group_of(exts, name=b"plain", body=b"payload"):
    return b"".join(exts) + member(name, body)


def malformed_pax():
    ok = pax_record(b"path", b"fine")
    bad = {
        "no_digits": b" path=x\n",
        "eleven_digits": b"00000000011 path=x\n",
        "no_space": b"12path=xyzw\n",
        "length_too_short": b"2 \n",
        "length_past_the_data": b"40 path=x\n",
        "no_newline_at_the_length": b"10 path=xy\n",
        "no_equals": b"8 path\n\n",
        "size_empty": pax_record(b"size", b""),
        "size_twenty_digits": pax_record(b"size", b"12345678901234567890"),
        "size_not_decimal": pax_record(b"size", b"1a"),
    }
    return [("pax_" + k, group_of([ext(b"x", ok + v)]) + END) for k, v in bad.items()]


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []

    def case(name, data, wellformed=False, sweep=False, status=R.OK):
        cases.append(Case(name, data, wellformed, sweep, status))

    for tag, fmt in FORMATS:
        case("tarfile_" + tag, tarfile_archive(fmt), wellformed=True, sweep=True)
    case("many_members", many_members(), wellformed=True)
    first, last = member(b"first", b"one"), member(b"last", b"three")
    case("base256_size", first + header(b"b256", size_field=b"\x80" + (700).to_bytes(11, "big")) + padded(noise(700, 1)) + last + END, wellformed=True)
    case("pax_size_disagrees", first + ext(b"x", pax_record(b"size", b"600")) + header(b"sized-by-pax", 5) + padded(noise(600, 2)) + last + END,
         wellformed=True)
    case("name_L_then_x", first + group_of([ext(b"L", b"from-L\0"), ext(b"x", pax_record(b"path", b"from-x") + pax_record(b"mtime", b"1.5"))]) + last + END)
    case("name_x_then_L", first + group_of([ext(b"x", pax_record(b"path", b"from-x")), ext(b"L", b"from-L" + b"l" * 130)]) + last + END)
    case("link_K_and_pax", first + group_of([ext(b"K", b"k-target\0"), ext(b"x", pax_record(b"linkpath", b"x-target"))], b"lnk", b"") + last + END)
    case("signed_checksum_only", first + member(b"h\xfc\xfe\xff-signed", b"body", signed=True) + last + END, wellformed=True)
    case("gnu_magic", first + member(b"gnu", b"body", magic=b"ustar  \0") + last + END, wellformed=True)
    case("prefix_and_name", first + member(b"leaf", b"body", prefix=b"some/dir") + last + END, wellformed=True)
    case("size_with_leading_spaces_and_an_empty_one", first + header(b"spaces", size_field=b"   1 \0" + b"x" * 6) + padded(b"1") +
         header(b"no-digits", size_field=b" " * 12) + last + END, wellformed=True)
    bad_mtime = bytearray(header(b"bad-mtime-and-mode", 3))
    bad_mtime[100:108], bad_mtime[136:148] = b"0000644x", b"\xff" * 12
    bad_mtime[148:156] = b" " * 8
    bad_mtime[148:156] = b"%06o\0 " % sum(bad_mtime)
    case("invalid_mode_and_mtime_are_zero", first + bytes(bad_mtime) + padded(b"abc") + last + END)
    case("typeflag_S", first + member(b"sparse", b"", typeflag=b"S") + last + END, status=R.UNSUPPORTED)
    case("typeflag_M", first + member(b"volume", b"", typeflag=b"M") + last + END, status=R.UNSUPPORTED)
    case("gnu_sparse_key", first + group_of([ext(b"x", pax_record(b"path", b"p") + pax_record(b"GNU.sparse.major", b"1"))]) + last + END,
         status=R.UNSUPPORTED)
    case("sixteen_extension_headers", first + group_of([ext(b"L", b"name-%02d\0" % k) for k in range(16)]) + last + END)
    case("seventeen_extension_headers", first + group_of([ext(b"L", b"name-%02d\0" % k) for k in range(17)]) + last + END, status=R.UNSUPPORTED)
    case("extension_data_too_large", first + header(b"././@ext", (1 << 20) + 1, typeflag=b"L") + bytes(2048), status=R.UNSUPPORTED)
    case("g_behind_L", first + ext(b"L", b"long\0") + ext(b"g", pax_record(b"comment", b"c")) + member(b"m") + END, status=R.BAD_HEADER)
    case("g_twice_then_members", ext(b"g", pax_record(b"comment", b"c")) + first + ext(b"g", pax_record(b"size", b"oops")) + last + END)
    case("extension_header_before_a_bad_header", first + ext(b"x", pax_record(b"path", b"p")) + noise(512, 3) + END, status=R.BAD_HEADER)
    case("extension_header_at_the_end", first + ext(b"L", b"long\0"), status=R.TRUNCATED)
    for name, data in malformed_pax():
        case(name, first + data, status=R.BAD_HEADER)
    flipped = bytearray(first + member(b"middle", b"two") + last + END)
    flipped[len(first) + 20] ^= 0x01
    case("flipped_byte_in_a_middle_header", bytes(flipped), status=R.BAD_HEADER)
    case("bad_size_field", first + header(b"bad-size", size_field=b"00000000019\0") + END, status=R.BAD_HEADER)
    case("no_magic_v7", first + member(b"v7", b"x", magic=bytes(8)) + END, status=R.BAD_HEADER)
    case("one_zero_block_then_garbage", first + bytes(512) + noise(1500, 4))
    case("zero_blocks_0", first + last, wellformed=True)
    case("zero_blocks_1", first + last + bytes(512), wellformed=True)
    case("zero_blocks_2", first + last + END, wellformed=True)
    case("zero_blocks_20", first + last + bytes(10240), wellformed=True)
    case("header_first_bytes_only", header(b"cut")[:300], status=R.TRUNCATED)
    case("content_without_padding", header(b"short", 100) + noise(100, 5), status=R.TRUNCATED)
    case("no_header_at_all", noise(2048, 6), status=R.BAD_HEADER)
    case("zero_blocks_only", END)
    case("empty", b"")
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


def cuts(data, every_block):
    """where an image is cut: every multiple of 512 and the odd places, or 16 sampled block boundaries and the odd places"""
    n = len(data)
    blocks = range(0, n, 512) if every_block else sorted({(n // 512) * k // 16 * 512 for k in range(16)})
    return sorted({c for c in list(blocks) + [1, 100, 511, 513, n - 1] if 0 <= c < n})
