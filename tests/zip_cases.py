"""The named ZIP archives of the tests of chip_zip_plan / chip_crc32_batch / chip_zip_decode, at the smallest sizes that reach each
path of the walk in include/compu_hip.h: archives zipfile wrote, hand-built ZIP64 forms, decoys, every refusal, every entry
status, alignments and the sizes around every power-of-two piece.  A Case carries the archive, the payload of every directory
entry in directory order (None where the case has no well-formed directory) and whether zipfile is expected to read it and to
agree (`independent`)."""
import functools
import io
import struct
import zipfile
import zlib

import numpy as np

import zip_writer as W
from zip_writer import DEFLATED, STORED, M32, Spec, build

SIZES = [0, 1, 15, 16, 17] + [(1 << k) + d for k in range(6, 19) for d in (-1, 0, 1)]  # around every piece and tile size


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text(n, seed):
    rng = np.random.default_rng(seed)
    words = [b"archive", b"entry", b"directory", b"central", b"local", b"deflate", b"stored", b"zip", b"crc", b"offset", b"wave", b"lane"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + (b" " if rng.integers(0, 7) else b"\n")
    return bytes(out[:n])


class Case:
    def __init__(self, name, data, payloads=None, independent=False):
        self.name, self.data, self.payloads, self.independent = name, bytes(data), payloads, independent

    def __repr__(self):
        return f"Case({self.name}, {len(self.data)} bytes)"


def three(**kw):
    """the three entries most hand-built cases start from: stored, deflated text, deflated noise (which deflate stores)"""
    return [Spec("a.txt", text(300, 1), STORED), Spec("dir/b.txt", text(5000, 2), DEFLATED), Spec("c.bin", noise(700, 3), DEFLATED)]


def built(name, specs, independent=False, **kw):
    return Case(name, build(specs, **kw).data, [s.payload for s in specs], independent)


class Unseekable:
    """a stream zipfile cannot seek in: every entry gets flag bit 3 and a data descriptor"""

    def __init__(self):
        self.buf = bytearray()

    def write(self, d):
        self.buf += d
        return len(d)

    def flush(self):
        pass


def by_zipfile():
    cases = []

    def make(name, fill, comment=b"", stream=None):
        target = stream if stream is not None else io.BytesIO()
        payloads = []
        with zipfile.ZipFile(target, "w") as zf:
            zf.comment = comment
            fill(zf, payloads)
        data = bytes(target.buf) if stream is not None else target.getvalue()
        cases.append(Case(name, data, payloads, True))

    def mixed(zf, payloads):
        for nm, pay, ct in (("a.txt", text(300, 1), zipfile.ZIP_STORED), ("dir/b.txt", text(5000, 2), zipfile.ZIP_DEFLATED),
                            ("c.bin", noise(700, 3), zipfile.ZIP_DEFLATED), ("d.txt", text(70000, 4), zipfile.ZIP_DEFLATED),
                            ("e.bin", noise(4097, 5), zipfile.ZIP_STORED)):
            zf.writestr(nm, pay, compress_type=ct)
            payloads.append(pay)

    def empty_and_dir(zf, payloads):
        zf.writestr("empty.txt", b"", compress_type=zipfile.ZIP_STORED)
        zi = zipfile.ZipInfo("b/")
        zi.compress_type = zipfile.ZIP_DEFLATED  # 2 bytes in, 0 out
        zf.writestr(zi, b"")
        zf.writestr("x.txt", text(100, 6), compress_type=zipfile.ZIP_DEFLATED)
        zf.writestr("empty.z", b"", compress_type=zipfile.ZIP_DEFLATED)
        payloads.extend([b"", b"", text(100, 6), b""])

    def forced(zf, payloads):
        zf.writestr("first.txt", text(200, 7), compress_type=zipfile.ZIP_DEFLATED)
        zi = zipfile.ZipInfo("forced.bin")
        zi.compress_type = zipfile.ZIP_DEFLATED
        with zf.open(zi, "w", force_zip64=True) as f:  # a ZIP64 extra in the local header only
            f.write(text(3000, 8))
        zf.writestr("last.txt", text(50, 9), compress_type=zipfile.ZIP_STORED)
        payloads.extend([text(200, 7), text(3000, 8), text(50, 9)])

    make("zipfile_mixed", mixed)
    make("zipfile_empty_file_and_directory", empty_and_dir)
    make("zipfile_unseekable_data_descriptors", mixed, stream=Unseekable())
    make("zipfile_comment_1", mixed, comment=b"!")
    make("zipfile_comment_65535", mixed, comment=text(65535, 10))
    make("zipfile_force_zip64_local", forced)
    return cases


def hand_zip64():
    cases = [built("zip64_end_record_and_locator", three(), True, zip64=True),
             built("zip64_count_ffff_real_count_in_record", three(), True, zip64=True, end=dict(n_here=0xFFFF, n_total=0xFFFF)),
             built("zip64_end_all_fields_ffffffff", three(), True, zip64=True, end=dict(n_here=0xFFFF, n_total=0xFFFF, cd_size=M32, cd_off=M32)),
             built("zip64_end_with_extensible_data", three(), False, zip64=True, end64=dict(extensible=b"PK\x01\x02 extensible"), between=b"")]
    foreign = W.subfield(0x5455, b"\x01" + struct.pack("<I", 1_600_000_000))
    fields = ("usize", "csize", "lho")
    for mask in range(8):
        subset = tuple(f for k, f in enumerate(fields) if mask >> k & 1)
        for where in ("front", "behind"):
            specs = three()
            specs[1] = Spec("dir/b.txt", text(5000, 2), DEFLATED, z64=subset, **({"extra_front": foreign} if where == "front" else {"extra_back": foreign}))
            # zipfile wants a ZIP64 extra to hold exactly the fields that are 0xFFFFFFFF: it agrees with every subset
            cases.append(built(f"zip64_extra_{'_'.join(subset) or 'none'}_foreign_{where}", specs, True))
    specs = three()
    specs[2] = Spec("c.bin", noise(700, 3), DEFLATED, z64=("usize",), cd=dict(disk=0xFFFF))
    cases.append(built("zip64_extra_and_disk_ffff", specs))
    specs = three()  # a broken subfield chain behind the id-1 subfield: not looked at
    specs[0] = Spec("a.txt", text(300, 1), STORED, z64=("csize",), extra_back=struct.pack("<Q", 77) + b"\x99\x99\xff\xff\x00")
    cases.append(built("zip64_extra_malformed_chain_behind_the_values", specs))
    return cases


def fake_record():
    """a whole directory record that is nobody's: a decoy the marking has to drop"""
    return W.central_record(b"decoy", 8, 0, 0x12345678, 10, 20, 0)


def decoys():
    cases = []
    specs = three()
    specs[1] = Spec(b"PK\x01\x02" + fake_record() + b".txt", text(5000, 2), DEFLATED)
    cases.append(built("decoy_signature_in_a_name", specs, True))
    specs = three()
    specs[1] = Spec("dir/b.txt", text(5000, 2), DEFLATED, extra_front=W.subfield(0x7777, fake_record() + b"PK\x01\x02"))
    cases.append(built("decoy_signature_in_an_extra_field", specs, True))
    specs = three()
    specs[0] = Spec("a.txt", text(300, 1), STORED, comment=b"see PK\x01\x02 and " + fake_record() * 2)
    specs[2] = Spec("c.bin", noise(700, 3), DEFLATED, comment=b"PK\x01\x02")
    cases.append(built("decoy_signature_in_a_file_comment", specs, True))
    # an end record inside the archive comment whose comment length does not reach the end: ignored
    inner = W.end_record(9, 9, 1234, 5678, clen=3)
    cases.append(built("decoy_end_record_in_the_comment_ignored", three(), False, comment=b"note " + inner + b" end"))  # (zipfile takes it)
    # one crafted so that it does: the highest qualifying position wins, by the rule.  It says "no entries".
    inner = W.end_record(0, 0, 0, 0, clen=6)
    cases.append(built("decoy_end_record_in_the_comment_wins", three(), False, comment=b"note " + inner + b"123456"))
    specs = three()
    specs[0] = Spec("a.txt", b"PK\x03\x04" + W.local_header(b"inner", 0, 0, 0, 4, 4) + b"data" + text(100, 11), STORED)
    cases.append(built("decoy_local_signature_in_stored_data", specs, True))
    return cases


def refusals():
    a = build(three())
    full = a.data
    cases = [Case("refused_21_bytes", full[-21:]), Case("refused_22_zero_bytes", bytes(22)), Case("refused_no_end_record", noise(3000, 12)),
             Case("refused_empty", b""), Case("refused_trailing_bytes", full + b"\x00"), Case("refused_trailing_64k", full + bytes(70000)),
             Case("accepted_end_record_alone", W.end_record(0, 0, 0, 0), [], True),
             Case("refused_end_record_cut", full[:-1])]
    z = build(three(), zip64=True)
    broken = bytearray(z.data)
    broken[z.end64_off:z.end64_off + 4] = b"PK\x06\x08"
    cases.append(Case("refused_locator_without_a_record", broken))
    cases.append(built("refused_locator_points_behind_itself", three(), zip64=True, loc=dict(end64_off=z.eocd_off - 20 - 55)))
    cases.append(built("refused_locator_offset_2_pow_64_minus_1", three(), zip64=True, loc=dict(end64_off=2**64 - 1)))
    cases.append(built("refused_directory_overlaps_the_end_record", three(), end=dict(cd_size=a.cd_size + 1)))
    cases.append(built("refused_directory_behind_the_end_record", three(), end=dict(cd_off=a.eocd_off + 1, cd_size=0)))
    cases.append(built("refused_zip64_directory_overlaps_its_record", three(), zip64=True, end64=dict(cd_size=a.cd_size + 1)))
    cases.append(built("refused_directory_sum_wraps", three(), zip64=True, end64=dict(cd_off=2**64 - 1, cd_size=2)))
    cases.append(built("refused_directory_size_wraps", three(), zip64=True, end64=dict(cd_off=1, cd_size=2**64 - 1)))
    cases.append(built("refused_count_2_pow_32", three(), zip64=True, end64=dict(n_here=1 << 32, n_total=1 << 32)))
    for k, label in ((0, "0"), (1, "1"), (2, "last")):
        specs = three()
        specs[k].cd["sig"] = b"PK\x01\x03"
        cases.append(built(f"refused_bad_signature_at_entry_{label}", specs))
    cases.append(built("refused_record_cut_by_the_directory_end", three(), end=dict(cd_size=a.cd_size - 1)))
    cases.append(built("refused_header_cut_by_the_directory_end", three(), end=dict(cd_size=a.record_off[2] - a.cd_off + 45)))
    cases.append(built("refused_count_larger_than_the_chain", three(), end=dict(n_here=4, n_total=4)))
    cases.append(built("accepted_count_smaller_than_the_chain", three(), end=dict(n_here=2, n_total=2)))
    cases.append(built("accepted_bytes_behind_the_last_record", three(), cd_tail=b"PK\x01\x02 not a record"))
    cases.append(built("refused_empty_directory_with_a_count", [], end=dict(n_here=1, n_total=1)))
    for f in ("usize", "csize", "lho"):
        specs = three()
        specs[1].cd[f] = M32  # 0xFFFFFFFF and no id-1 subfield
        cases.append(built(f"refused_missing_zip64_value_{f}", specs))
    specs = three()
    specs[1] = Spec("dir/b.txt", text(5000, 2), DEFLATED, z64=("usize",), cd=dict(csize=M32))  # one value for two fields
    cases.append(built("refused_zip64_extra_one_value_short", specs))
    specs = three()
    specs[1] = Spec("dir/b.txt", text(5000, 2), DEFLATED, cd=dict(usize=M32, extra=struct.pack("<HH", 1, 8) + b"\x01\x02\x03"))  # cut by the field
    cases.append(built("refused_zip64_value_cut_by_the_extra_field", specs))
    for label, kw in (("disk", dict(end=dict(disk=1))), ("directory_disk", dict(end=dict(cd_disk=1))), ("counts_differ", dict(end=dict(n_here=2))),
                      ("zip64_locator_disk", dict(zip64=True, loc=dict(disk=1))), ("zip64_locator_total_2", dict(zip64=True, loc=dict(total_disks=2))),
                      ("zip64_record_disk", dict(zip64=True, end64=dict(disk=1))), ("zip64_record_directory_disk", dict(zip64=True, end64=dict(cd_disk=1))),
                      ("zip64_counts_differ", dict(zip64=True, end64=dict(n_here=2)))):
        cases.append(built(f"refused_spanning_{label}", three(), **kw))
    return cases


def entry_statuses():
    cases = []

    def one(name, spec, k=1, **kw):
        specs = three()
        specs[k] = spec
        cases.append(built(name, specs, **kw))

    for m in (12, 14, 93):
        one(f"entry_method_{m}", Spec("m.bin", noise(100, 13), m))
    for bit in (0, 6, 13):
        one(f"entry_encrypted_bit_{bit}", Spec("s.bin", text(500, 14), DEFLATED, flags=1 << bit))
    one("entry_method_12_and_encrypted", Spec("s.bin", text(500, 14), 12, flags=1))
    a = build(three())
    one("entry_local_header_behind_the_directory_start", Spec("dir/b.txt", text(5000, 2), DEFLATED, cd=dict(lho=a.cd_off - 29)))
    one("entry_local_header_in_the_directory", Spec("dir/b.txt", text(5000, 2), DEFLATED, cd=dict(lho=a.cd_off)))
    one("entry_local_header_offset_2_pow_64_minus_1", Spec("dir/b.txt", text(5000, 2), DEFLATED, z64=("lho",), cd=dict(lho=2**64 - 1)))
    one("entry_wrong_local_signature", Spec("dir/b.txt", text(5000, 2), DEFLATED, local=dict(sig=b"PK\x03\x05")))
    one("entry_data_reaches_into_the_directory", Spec("c.bin", noise(700, 3), DEFLATED, cd=dict(csize=len(W.raw_deflate(noise(700, 3))) + 1)), k=2)
    one("entry_comp_size_2_pow_64_minus_1", Spec("c.bin", noise(700, 3), DEFLATED, z64=("csize",), cd=dict(csize=2**64 - 1)), k=2)
    one("entry_stored_with_another_size", Spec("a.txt", text(300, 1), STORED, cd=dict(usize=301)), k=0)
    patched = bytearray(a.data)  # the local header's name length says 65 535: the data would begin behind the directory's start
    patched[a.header_off[2] + 26:a.header_off[2] + 28] = b"\xff\xff"
    cases.append(Case("entry_local_name_length_reaches_out", patched, [s.payload for s in three()]))
    one("entry_size_2_pow_32_minus_1_is_too_large", Spec("dir/b.txt", text(5000, 2), DEFLATED, z64=("usize",), cd=dict(usize=(1 << 32) - 1)))
    one("entry_size_2_pow_32_minus_2_is_a_unit", Spec("dir/b.txt", text(5000, 2), DEFLATED, cd=dict(usize=(1 << 32) - 2)))
    # BAD_LOCAL comes before TOO_LARGE in the header's order: so much data is not in front of this directory
    one("entry_comp_size_2_pow_29_minus_63_in_a_tiny_file", Spec("dir/b.txt", text(5000, 2), DEFLATED, z64=("usize",),
                                                                 cd=dict(csize=(1 << 29) - 63, usize=(1 << 32) - 1)))
    one("entry_stored_size_2_pow_32_in_a_tiny_file", Spec("a.txt", text(300, 1), STORED, z64=("usize", "csize"), cd=dict(usize=1 << 32, csize=1 << 32)),
        k=0)
    one("entry_disk_1", Spec("dir/b.txt", text(5000, 2), DEFLATED, cd=dict(disk=1)))
    one("entry_disk_ffff_without_zip64_extra", Spec("dir/b.txt", text(5000, 2), DEFLATED, cd=dict(disk=0xFFFF)))
    one("entry_local_header_differs_from_the_directory", Spec("dir/b.txt", text(5000, 2), DEFLATED, local=dict(crc=0, csize=0, usize=0, name=b"other")))
    return cases


def alignments():
    cases = []
    for k in range(16):
        specs = three()
        pad = (k - build(specs).cd_off) % 16
        cases.append(built(f"directory_starts_at_{k}_mod_16", specs, True, gap=bytes(pad)))
        assert build(specs, gap=bytes(pad)).cd_off % 16 == k
    specs = []
    for k in range(16):  # entry data at every alignment, stored and deflated
        for method in (STORED, DEFLATED):
            name = f"{'sd'[method == DEFLATED]}{k:02d}".encode()
            at = sum(len(s.pre) + 30 + len(s.name) + len(s.data) for s in specs)
            specs.append(Spec(name, text(1000 + 37 * k, 20 + k), method, pre=bytes((k - (at + 30 + len(name))) % 16)))
    a = build(specs)
    assert [o % 16 for o in a.data_off] == [k for k in range(16) for _ in range(2)]
    cases.append(Case("entry_data_at_every_alignment", a.data, [s.payload for s in specs], True))
    return cases


def stored_sizes():
    blob = noise(max(SIZES), 30)
    specs = [Spec(f"s{n}", blob[:n] if n % 2 else blob[len(blob) - n:], STORED) for n in SIZES]
    return [built("stored_sizes_around_every_power_of_two", specs, True)]


def deflated_sizes():
    specs = [Spec(f"d{n}", text(n, 40 + k), DEFLATED) for k, n in enumerate((0, 1, 15, 16, 17, 4095, 4096, 4097, 65535, 65536, 65537, 200001))]
    return [built("deflated_sizes", specs, True)]


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = by_zipfile() + hand_zip64() + decoys() + refusals() + entry_statuses() + alignments() + stored_sizes() + deflated_sizes()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def seventy_thousand_empty():
    """70 000 empty stored entries: more than 65 535, so zipfile writes the ZIP64 end record and its locator itself"""
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as zf:
        for k in range(70000):
            zf.writestr(f"e{k:05d}", b"", compress_type=zipfile.ZIP_STORED)
    return b.getvalue()


def flip_directory_crc(data, summary, k):
    """the archive with the directory's CRC-32 of entry k changed (entries are walked from the directory's start)"""
    d = bytearray(data)
    q = summary[3]
    for _ in range(k):
        q += 46 + sum(struct.unpack_from("<HHH", d, q + 28))
    d[q + 16] ^= 0x40
    return bytes(d)


def crc32(b):
    return zlib.crc32(b) & M32
