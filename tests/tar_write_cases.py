"""The cases of the tar writer's tests (test_tar_write_cpu.py, test_tar_write_gpu.py): what chip_tar_write_host and chip_tar_write
are run on, each with the answer of the Python restatement (tar_write_ref.py).  A case is a list of members laid out into a names
buffer and a content buffer (both with odd offsets and bytes nobody uses), flags and record_bytes.  The layouts are built in all four
flag combinations where the rules differ by flag.
The lengths of a pax record cross a digit count at 9 -> 11 (no record of 10 bytes exists: a `size` record of a one-digit and of a
two-digit size), 999 -> 1001 and 9999 -> 10001 (path and linkpath records); a record of 99 or 100 bytes cannot be written, because
the path and linkpath records start at values of 101 bytes and a size record ends at 28."""
import random

import tar_write_ref as WR

FLAGSETS = (0, WR.TW_GNU, WR.TW_FORCE_EXT, WR.TW_GNU | WR.TW_FORCE_EXT)
FLAG_NAMES = {0: "pax", 1: "gnu", 2: "pax_force", 3: "gnu_force"}


class Member:
    def __init__(self, name, data=b"", link=b"", typeflag="0", mode=0o644, uid=1000, gid=100, mtime=1700000000):
        self.name, self.data, self.link, self.typeflag = name, data, link, ord(typeflag)
        self.mode, self.uid, self.gid, self.mtime = mode, uid, gid, mtime


class Case:
    def __init__(self, name, sources, names, content, flags=0, record_bytes=0, content_len=None, arith=False, members=None):
        self.name, self.sources, self.names, self.content, self.flags, self.record_bytes = name, sources, bytes(names), bytes(content), flags, record_bytes
        self.content_len = len(content) if content_len is None else content_len
        self.arith, self.members = arith, members
        self._want = None

    def want(self):
        """(image or None, rows, summary) of the reference: with the room it needs, or for an arithmetic case with none"""
        if self._want is None:
            self._want = WR.write(self.sources, self.names, self.content_len, self.content, self.flags, self.record_bytes, 0 if self.arith else None)
        return self._want

    @property
    def bad(self):
        return self.want()[2][6] == WR.BAD_SOURCE


def payload(n, seed):
    return random.Random(seed).randbytes(n)


def lay_out(name, members, flags=0, record_bytes=0):
    """a case from members: names and link names, and the contents, each behind a few bytes of filler so that no offset is aligned"""
    names, content, sources = bytearray(b"\xfe\0\xfe"), bytearray(b"\xfd" * 5), []
    for k, m in enumerate(members):
        name_off = len(names)
        names += m.name + b"\0"  # (the NUL is outside the name)
        link_off = len(names)
        names += m.link + b"\xfe" * (k % 3)
        data_off = len(content)
        content += m.data + b"\xfd" * (1 + k % 7)
        sources.append((data_off, len(m.data), name_off, link_off, m.mtime, len(m.name), len(m.link), m.mode, m.uid, m.gid, m.typeflag, (0, 0, 0)))
    return Case(name, sources, names, content, flags, record_bytes, members=members)


def plain_name(n, slash=True):
    """a name of n bytes: directories of nine letters when slash, else no '/' at all; never a '/' at the end"""
    if not slash:
        return (b"n" * n)
    s = (b"abcdefghi/" * (n // 10 + 1))[:n]
    return s[:-1] + b"z"


def member_sets():
    sets = {}
    sets["name_lengths"] = [Member(plain_name(n), payload(10 + k, n)) for k, n in enumerate((1, 99, 100, 101, 255, 256, 257, 1000))]
    sets["name_lengths_no_slash"] = [Member(plain_name(n, False), payload(3, n)) for n in (100, 101, 255, 256, 257)]
    sets["name_65535"] = [Member(plain_name(65535), b"x"), Member(plain_name(65535, False), b"", link=plain_name(65535), typeflag="2")]
    sets["split"] = [
        Member(b"a" * 155 + b"/" + b"b" * 100, b"p155"),          # p = 155, a rest of 100
        Member(b"a" * 156 + b"/" + b"b" * 50, b"p156"),           # the only '/' at 156: no split
        Member(b"a" * 50 + b"/" + b"b" * 101, b"rest101"),        # a rest of 101: no split
        Member(b"a" * 120 + b"/", typeflag="5", mode=0o755),      # ends in its only '/': no split
        Member(b"a" * 50 + b"/" + b"b" * 50 + b"/" + b"c" * 50, b"largest"),  # p = 50 leaves 101, p = 101 leaves 50
        Member(b"d/" * 60 + b"e", b"many"),                        # many candidates: the largest that fits
        Member(b"/" + b"f" * 100, b"p0"),                          # the only '/' at 0: p >= 1, no split
        Member(b"g/" + b"h" * 100, b"p1"),                         # p = 1
    ]
    sets["links"] = [Member(b"l%d" % n, link=plain_name(n) if n else b"", typeflag="2", mode=0o777) for n in (0, 100, 101, 300)] + [
        Member(plain_name(300, False), link=plain_name(300, False), typeflag="1")]
    sets["sizes"] = [Member(b"s/%d" % n, payload(n, n)) for n in (0, 1, 511, 512, 513, 4095, 4096, 4097, 70000)]
    sets["typeflags"] = [Member(b"t" + t.encode(), payload(20, 7) if t in "07" else b"", link=b"target" if t in "12" else b"", typeflag=t) for t in "01234567"]
    sets["record_digits"] = [Member(plain_name(n, False), payload(s, n)) for n, s in ((989, 5), (990, 50), (991, 0), (9988, 1), (9989, 12))] + [
        Member(b"k%d" % n, link=plain_name(n, False), typeflag="2") for n in (985, 986, 9984, 9985)]
    sets["one"] = [Member(b"only", b"hello\n")]
    sets["one_empty"] = [Member(b"e")]
    sets["numbers"] = [Member(b"max", b"m", mode=0o7777777, uid=8 ** 7 - 1, gid=8 ** 7 - 1, mtime=8 ** 11 - 1), Member(b"zero", b"", mode=0, uid=0, gid=0, mtime=0)]
    sets["bytes_above_127"] = [Member(bytes(range(1, 256)) * 2, b"hi", link=bytes(range(128, 256)) * 2, typeflag="0")]
    return sets


BAD_RULES = {
    "typeflag_below_0": dict(typeflag=ord("0") - 1), "typeflag_above_7": dict(typeflag=ord("8")), "typeflag_x": dict(typeflag=ord("x")),
    "size_of_a_link": dict(typeflag=ord("2"), size=1), "size_of_a_directory": dict(typeflag=ord("5"), size=1), "size_of_type_1": dict(typeflag=ord("1"), size=1),
    "size_of_type_6": dict(typeflag=ord("6"), size=3),
    "name_len_0": dict(name_len=0), "name_len_65536": dict(name_len=65536, long_names=True), "link_len_65536": dict(link_len=65536, long_names=True),
    "nul_in_a_short_name": dict(nul="name", at=2, length=5), "nul_at_the_end_of_a_name_of_64": dict(nul="name", at=63, length=64),
    "nul_in_a_name_of_65": dict(nul="name", at=64, length=65), "nul_first_in_a_long_name": dict(nul="name", at=0, length=3000),
    "nul_last_in_a_long_name": dict(nul="name", at=2999, length=3000), "nul_in_the_tail_of_a_long_name": dict(nul="name", at=1001, length=1003),
    "nul_in_a_short_link": dict(nul="link", at=0, length=1), "nul_in_a_long_link": dict(nul="link", at=777, length=2000),
    "name_outside": dict(name_off="end"), "name_off_wraps": dict(name_off=(1 << 64) - 1), "link_outside": dict(link_off="end", link_len=4),
    "link_off_wraps": dict(link_off=(1 << 64) - 2, link_len=4), "data_outside": dict(data_off="end"), "data_off_wraps": dict(data_off=(1 << 64) - 1),
    "size_wraps": dict(size=(1 << 64) - 1, data_off=2),
    "mode": dict(mode=0o10000000), "uid": dict(uid=8 ** 7), "gid": dict(gid=8 ** 7), "mtime_negative": dict(mtime=-1), "mtime_8_pow_11": dict(mtime=8 ** 11),
    "pad_0": dict(pad=(1, 0, 0)), "pad_1": dict(pad=(0, 1, 0)), "pad_2": dict(pad=(0, 0, 0x80)),
}
FIELDS = ("data_off", "size", "name_off", "link_off", "mtime", "name_len", "link_len", "mode", "uid", "gid", "typeflag", "pad")


def bad_case(rule, spec, second):
    """three good members with one made bad by `spec` at index 1 (sole) -- or, second: another bad record at index 1 and this one at 2"""
    spec = dict(spec)
    members = [Member(b"good%d" % k, payload(9, k)) for k in range(4)]
    which = 2 if second else 1
    if "nul" in spec:
        text = bytearray(b"q" * spec["length"])
        text[spec["at"]] = 0
        if spec["nul"] == "name":
            members[which] = Member(bytes(text), b"x")
        else:
            members[which] = Member(b"lnk", link=bytes(text), typeflag="2")
    case = lay_out(("bad_second_" if second else "bad_") + rule, members)
    if spec.pop("long_names", False):
        case.names += b"n" * 70000
    rows = [dict(zip(FIELDS, s)) for s in case.sources]
    for key, v in spec.items():
        if key in ("nul", "at", "length"):
            continue
        if v == "end":  # one byte too far
            r = rows[which]
            v = {"name_off": len(case.names) - r["name_len"] + 1, "link_off": len(case.names) - 3, "data_off": len(case.content) - r["size"] + 1}[key]
        rows[which][key] = v
    if second:
        rows[1]["typeflag"] = ord("L")
    case.sources = [tuple(r[f] for f in FIELDS) for r in rows]
    case.members = None
    return case


def arith_cases():
    out = []
    big = 8 ** 11
    for flags in FLAGSETS:
        tag = FLAG_NAMES[flags]
        names = b"huge" + b"second/" + b"n" * 120
        src = lambda size, off=0: [(off, size, 0, 0, 5, 4, 0, 0o600, 0, 0, ord("0"), (0, 0, 0)),  # noqa: E731
                                   (1, 513, 4, 4, 6, 127, 0, 0o644, 1, 1, ord("0"), (0, 0, 0))]
        out.append(Case(f"arith_2_pow_40_{tag}", src(1 << 40), names, b"", flags, 0, content_len=1 << 40, arith=True))
        out.append(Case(f"arith_size_8_pow_11_{tag}", src(big, 1), names, b"", flags, 512, content_len=big + 1, arith=True))
        out.append(Case(f"arith_size_8_pow_11_minus_1_{tag}", src(big - 1), names, b"", flags, 0, content_len=big, arith=True))
        out.append(Case(f"arith_size_2_pow_61_{tag}", src(1 << 61), names, b"", flags, 1 << 20, content_len=(1 << 61) + 1024, arith=True))
    return out


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        cases = []
        for key, members in member_sets().items():
            for flags in FLAGSETS:
                cases.append(lay_out(f"{key}_{FLAG_NAMES[flags]}", members, flags))
        for rb in (512, 10240, 1 << 20):
            cases.append(lay_out(f"record_{rb}", member_sets()["sizes"][:4], 0, rb))
            cases.append(Case(f"empty_record_{rb}", [], b"", b"", 0, rb))
        cases.append(Case("empty", [], b"", b"", 0, 0))
        cases.append(Case("empty_gnu_force", [], b"", b"", 3, 0))
        for rule, spec in BAD_RULES.items():
            cases.append(bad_case(rule, spec, False))
            cases.append(bad_case(rule, spec, True))
        cases.append(Case("bad_only_member", [(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, ord("0"), (0, 0, 0))], b"n", b""))
        b = bad_case("typeflag_x", BAD_RULES["typeflag_x"], False)
        cases.append(Case("bad_first_and_last", [b.sources[1], b.sources[0], b.sources[1]], b.names, b.content, WR.TW_GNU))
        cases += arith_cases()
        _ALL = cases
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
