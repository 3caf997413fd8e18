"""What the file-writer tests share (chip_pack_units, chip_encode_file; include/compu_hip.h, "writing files"): the cut of a buffer
into units, chip_encode_file_bound's formula restated, and a writer and a parser of the seek table of zstd's seekable format
(contrib/seekable_format; all integers little endian):

    LE32 0x184D2A5E | LE32 Frame_Size | n x { LE32 Compressed_Size, LE32 Decompressed_Size [, LE32 checksum] } |
    LE32 Number_Of_Frames | u8 Seek_Table_Descriptor (bit 7 Checksum_Flag, bits 6..2 reserved) | LE32 0x8F92EAB1
"""
import struct

FMT_GZIP, FMT_ZSTD, FMT_BGZF = 31, 100, 131
W_SEEK_TABLE = 1
FILE_OK, FILE_NEED_OUTPUT = 0, 1
SKIPPABLE_MAGIC, SEEKABLE_MAGIC = 0x184D2A5E, 0x8F92EAB1
BGZF_PAYLOAD, DEFAULT_UNIT, MAX_UNIT = 65280, 262144, 1 << 30


def unit_of(fmt, unit_bytes):
    return unit_bytes or (BGZF_PAYLOAD if fmt == FMT_BGZF else DEFAULT_UNIT)


def cuts(fmt, length, unit_bytes=0):
    """[(offset, length)] of the units chip_encode_file encodes: ceil(length / unit) cuts; an empty gzip / zstd input is one
    unit of empty content, an empty BGZF input none."""
    unit = unit_of(fmt, unit_bytes)
    out = [(at, min(unit, length - at)) for at in range(0, length, unit)]
    return out or ([] if fmt == FMT_BGZF else [(0, 0)])


def trailer_bytes(fmt, flags, n):
    return 28 if fmt == FMT_BGZF else 17 + 8 * n if flags & W_SEEK_TABLE else 0


def file_bound(lib, fmt, unit_bytes, flags, length):
    """(n - 1) * bound(unit) + bound(last unit) + trailer, with the library's chip_encode_bound"""
    c = cuts(fmt, length, unit_bytes)
    if not c:
        return trailer_bytes(fmt, flags, 0)
    return (len(c) - 1) * lib.chip_encode_bound(fmt, unit_of(fmt, unit_bytes)) + lib.chip_encode_bound(fmt, c[-1][1]) + trailer_bytes(fmt, flags, len(c))


def seek_table(entries, descriptor=0):
    """the table of [(compressed size, decompressed size)], without per-frame checksums"""
    body = b"".join(struct.pack("<II", c, d) for c, d in entries)
    return struct.pack("<II", SKIPPABLE_MAGIC, len(body) + 9) + body + struct.pack("<IBI", len(entries), descriptor, SEEKABLE_MAGIC)


def parse_seek_table(data, table_off):
    """[(compressed size, decompressed size)] of the seek table that fills data[table_off:]; ValueError when it is none."""
    t = bytes(data[table_off:])
    if len(t) < 17:
        raise ValueError("shorter than an empty seek table")
    magic, frame_size = struct.unpack_from("<II", t, 0)
    n, descriptor, tail_magic = struct.unpack_from("<IBI", t, len(t) - 9)
    if magic != SKIPPABLE_MAGIC or tail_magic != SEEKABLE_MAGIC:
        raise ValueError(f"magic numbers {magic:#x} / {tail_magic:#x}")
    if descriptor & 0x7C:
        raise ValueError(f"reserved bits in the descriptor {descriptor:#x}")
    size = 12 if descriptor & 0x80 else 8
    if frame_size != len(t) - 8 or frame_size != n * size + 9:
        raise ValueError(f"Frame_Size {frame_size} for {n} entries of {size} bytes in {len(t)} bytes")
    return [struct.unpack_from("<II", t, 8 + size * i) for i in range(n)]
