"""The named inputs of the ZIP writer's tests (chip_zip_assemble_host, chip_zip_assemble, chip_zip_write), a few entries each, at the
smallest sizes that reach every rule of include/compu_hip.h ("ZIP archives: writing").  A Case carries the arguments of the assemble
calls -- sources (tuples, see zip_write_ref), names, content, the comp triple or None, crcs, flags -- and says whether its streams
are real deflate (`real`: zipfile and the plan can read the archive; else it is byte-compared only) and whether it is pure arithmetic
(`arith`: run with out_cap = 0 and a stated content_len the bytes do not have)."""
import functools
import zlib

import zip_write_ref as WR
from zip_cases import noise, text
from zip_writer import raw_deflate

STORE, DEFLATE = WR.STORE, WR.DEFLATE
ZIP64, UTF8 = WR.ZW_ZIP64, WR.ZW_UTF8
M32 = WR.M32


class Case:
    def __init__(self, name, sources, names, content, comp, crcs, flags=0, real=True, arith=False, content_len=None, payloads=None):
        self.name, self.sources, self.names, self.content, self.comp, self.crcs = name, list(sources), bytes(names), bytes(content), comp, list(crcs)
        self.flags, self.real, self.arith = flags, real, arith
        self.content_len = len(content) if content_len is None else content_len
        self.payloads = payloads if payloads is not None or self.sources else []

    def __repr__(self):
        return f"Case({self.name}, {len(self.sources)} entries)"

    def want(self, out_cap=None):
        """what the reference makes of it"""
        return WR.assemble(self.sources, self.names, self.content, self.comp, self.crcs, self.flags, out_cap=0 if self.arith else out_cap,
                           content_len=self.content_len)


def items(name, entries, flags=0, streams="real", shift=0, dos=(0x6000, 0x5A21)):
    """a case from (name, payload, method) triples: the contents end to end from `shift` with one byte between them, so that the
    data offsets take every alignment; streams "real" (zlib's raw deflate for the method 8 entries), "none" (no comp arrays)"""
    names, content, sources, crcs, raw = bytearray(), bytearray(b"\xEE" * shift), [], [], []
    for nm, pay, method in entries:
        sources.append((len(content), len(pay), len(names), len(nm), method, dos[0], dos[1]))
        names += nm
        content += pay + b"\xEE"
        crcs.append(zlib.crc32(pay))
        raw.append(raw_deflate(pay) if method == DEFLATE else None)
    comp = WR.pack_streams(raw) if streams == "real" else None
    return Case(name, sources, names, content, comp, crcs, flags, payloads=[e[1] for e in entries])


def pinned(name, size, comp_len):
    """one entry that asks for method 8 with a hand-given comp_len around its size: the streams are filler bytes"""
    pay = text(size, 31)
    filler = [bytes([0xC0 + k % 16 for k in range(comp_len)]), b"\xDD" * 5]
    comp = WR.pack_streams(filler)
    sources = [(0, size, 0, 1, DEFLATE, 0, 0x21), (0, size, 1, 1, DEFLATE, 0, 0x21)]
    return Case(name, sources, b"ab", pay, comp, [zlib.crc32(pay)] * 2, real=False)


def bad_sources():
    good = [(0, 10, 0, 2, STORE, 0, 0x21), (3, 7, 2, 3, DEFLATE, 0, 0x21), (10, 0, 5, 0, STORE, 0, 0x21), (0, 10, 0, 5, DEFLATE, 0, 0x21)]
    names, content = b"abcde", text(10, 5)
    comp = WR.pack_streams([None, b"\x01\x02\x03", None, b"\x01\x02\x03\x04"])
    crcs = [1, 2, 3, 4]

    def case(name, edits, comp=comp):
        s = list(good)
        for k, e in edits.items():
            row = list(s[k])
            for f, v in e.items():
                row[f] = v
            s[k] = tuple(row)
        return Case("bad_" + name, s, names, content, comp, crcs, real=False)

    out = [case("method_1", {1: {4: 1}}), case("method_9", {0: {4: 9}}), case("method_0xffff", {3: {4: 0xFFFF}}),
           case("data_one_past_the_end", {1: {0: 4}}), case("data_off_behind_the_end", {2: {0: 11}}), case("data_sum_wraps", {0: {0: 2**64 - 1, 1: 2}}),
           case("size_2_pow_64_minus_1", {3: {1: 2**64 - 1}}), case("name_one_past_the_end", {1: {2: 3}}), case("name_off_behind_the_end", {2: {2: 6}}),
           case("name_sum_wraps", {0: {2: 2**64 - 1}}),
           case("stream_one_past_the_end", {}, comp=(comp[0], [0, 0, 0, 4], [0, 3, 0, 4])),
           case("stream_off_wraps", {}, comp=(comp[0], [0, 2**64 - 2, 0, 3], [0, 3, 0, 4])),
           case("two_bad_records_the_lower_wins", {1: {4: 3}, 3: {0: 11}}), case("first_and_last", {0: {2: 6}, 3: {4: 2}})]
    # a stream out of range that is not used -- the entry is stored, its comp_len is 0 or not smaller than the size -- is no fault
    ok = Case("unused_stream_out_of_range_is_ignored", good, names, content, (comp[0], [0, 0, 99, 99], [0, 3, 0, 10]), crcs, real=False)
    return out + [ok]


def arithmetic():
    big = 1 << 40
    one = lambda name, sources, flags=0: Case("arith_" + name, sources, b"n", b"\0" * 8, None, [7] * len(sources), flags, real=False, arith=True,  # noqa: E731
                                              content_len=big)
    st = lambda size: (0, size, 0, 1, STORE, 0, 0x21)  # noqa: E731
    fill = M32 - 1 - 31  # a stored entry named "n" whose local part ends at M32 - 1
    return [one("stored_m32_minus_1_is_plain", [st(M32 - 1)]), one("stored_m32_takes_the_zip64_sizes", [st(M32)]),
            one("stored_2_pow_40", [st(big), st(5)]),
            one("header_off_m32_minus_1_is_plain", [st(fill), st(5)]), one("header_off_m32_goes_into_the_subfield_alone", [st(fill + 1), st(5)]),
            one("cd_off_m32_minus_1_is_plain", [st(fill)]), one("cd_off_m32_alone_takes_the_zip64_end", [st(fill + 1)]),
            one("cd_off_crosses_with_the_last_header_below", [st(M32 - 100), st(200)]),
            one("both_forms_in_one_entry", [st(M32 + 5), st(M32 + 5)]), one("forced_small", [st(3), st(0)], ZIP64)]


def counted(n):
    names = b"".join(b"e%05d" % k for k in range(n))
    return Case(f"count_{n}", [(0, 0, 6 * k, 6, STORE, 0, 0x21) for k in range(n)], names, b"", None, [0] * n, real=True, payloads=[b""] * n)


@functools.lru_cache(maxsize=None)
def all_cases():
    t, r = text(5000, 11), noise(700, 12)
    mixed = [(b"a.txt", text(300, 1), STORE), (b"dir/", b"", DEFLATE), (b"dir/b.txt", t, DEFLATE), (b"c.bin", r, DEFLATE), (b"d", b"x", DEFLATE)]
    cases = [Case("empty", [], b"", b"", None, []), Case("empty_force", [], b"", b"", None, [], ZIP64),
             Case("empty_with_buffers", [], b"unused", b"unused", (b"zz", [], []), [], UTF8),
             items("one_empty_entry", [(b"dir/", b"", DEFLATE)]), items("one_empty_stored_entry", [(b"dir/", b"", STORE)]),
             items("empty_name", [(b"", text(40, 2), DEFLATE), (b"", b"", STORE)]),
             items("name_of_1_byte", [(b"x", text(100, 3), DEFLATE)]), items("name_of_255_bytes", [(b"n" * 255, text(100, 3), DEFLATE), (b"m", b"q", STORE)]),
             items("name_of_65535_bytes", [(b"L" * 65535, text(100, 3), DEFLATE), (b"after", b"tail", STORE)]),
             items("contents_of_0_1_2_bytes", [(b"0", b"", DEFLATE), (b"1", b"a", DEFLATE), (b"2", b"ab", DEFLATE), (b"s0", b"", STORE), (b"s1", b"a", STORE),
                                                 (b"s2", b"ab", STORE)]),
             items("text_deflates", [(b"t", t, DEFLATE)]), items("noise_does_not", [(b"r", r, DEFLATE)]),
             items("method_0_asked_for_text", [(b"t", t, STORE)]),
             pinned("comp_len_size_minus_1_is_deflated", 40, 39), pinned("comp_len_size_is_stored", 40, 40),
             pinned("comp_len_size_plus_1_is_stored", 40, 41), pinned("comp_len_0_is_stored", 40, 0), pinned("comp_len_1_is_deflated", 40, 1),
             items("no_comp_arrays", mixed, streams="none"),
             items("mixed", mixed), items("mixed_utf8", mixed, UTF8), items("mixed_force", mixed, ZIP64), items("mixed_force_utf8", mixed, ZIP64 | UTF8),
             items("no_comp_arrays_force", mixed, ZIP64, streams="none"),
             items("sizes_around_a_tile", [(b"%d" % n, text(n, n), DEFLATE if k % 2 else STORE) for k, n in enumerate((15, 16, 17, 4095, 4096, 4097))])]
    for shift in range(4):
        cases.append(items(f"data_off_alignment_{shift}", mixed, shift=shift))
    # the ranges in any order, two entries sharing one range
    base = items("x", [(b"p", text(333, 4), DEFLATE), (b"q", noise(50, 5), STORE), (b"r", text(1000, 6), DEFLATE)], shift=1)
    order = [2, 0, 1, 0]
    comp = (base.comp[0], [base.comp[1][k] for k in order], [base.comp[2][k] for k in order])
    cases.append(Case("ranges_in_any_order_and_shared", [base.sources[k] for k in order], base.names, base.content, comp, [base.crcs[k] for k in order],
                      payloads=[base.payloads[k] for k in order]))
    return cases + bad_sources() + arithmetic() + [counted(65534), counted(65535)]


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


def seventy_thousand():
    """the one archive above toy size: 70 000 entries of 0 or 1 bytes named e%05d, every third one asking for method 8"""
    n = 70000
    names = b"".join(b"e%05d" % k for k in range(n))
    content = bytes(range(256)) * 4
    sources = [(k % 1000, k % 2, 6 * k, 6, DEFLATE if k % 3 == 0 else STORE, k % 65536, 0x21 + k % 7) for k in range(n)]
    crcs = [zlib.crc32(content[s[0]:s[0] + s[1]]) for s in sources]
    return sources, names, content, crcs
