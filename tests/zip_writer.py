"""ZIP archives built field by field (APPNOTE.TXT 4.3), for the tests of chip_zip_plan / chip_zip_decode: every record is a function
of its fields, and `build` lays out an archive from entry specs in which any field of any record can be overridden, so that
every form the directory walk of include/compu_hip.h distinguishes is reachable with three or four entries.  Nothing here
reads an archive."""
import struct
import zlib

SIG_LOCAL, SIG_CENTRAL, SIG_END, SIG_END64, SIG_LOC64 = b"PK\x03\x04", b"PK\x01\x02", b"PK\x05\x06", b"PK\x06\x06", b"PK\x06\x07"
STORED, DEFLATED = 0, 8
M32, M16 = 0xFFFFFFFF, 0xFFFF


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def subfield(ident, data):
    return struct.pack("<HH", ident, len(data)) + data


def zip64_extra(values):
    """the id-1 subfield holding `values` as 64-bit integers, in the order given"""
    return subfield(1, b"".join(struct.pack("<Q", v) for v in values))


def local_header(name, method, flags, crc, csize, usize, extra=b"", sig=SIG_LOCAL, version=20, dos_time=0, dos_date=0x21):
    return sig + struct.pack("<HHHHHIIIHH", version, flags, method, dos_time, dos_date, crc & M32, csize & M32, usize & M32, len(name), len(extra)) + name + extra


def central_record(name, method, flags, crc, csize, usize, lho, extra=b"", comment=b"", disk=0, sig=SIG_CENTRAL, made_by=20, version=20,
                   dos_time=0, dos_date=0x21, internal=0, external=0, nlen=None, xlen=None, clen=None):
    nlen = len(name) if nlen is None else nlen
    xlen = len(extra) if xlen is None else xlen
    clen = len(comment) if clen is None else clen
    return (sig + struct.pack("<HHHHHHIIIHHHHHII", made_by, version, flags, method, dos_time, dos_date, crc & M32, csize & M32, usize & M32, nlen,
                              xlen, clen, disk, internal, external, lho & M32) + name + extra + comment)


def end_record(n_here, n_total, cd_size, cd_off, comment=b"", disk=0, cd_disk=0, sig=SIG_END, clen=None):
    clen = len(comment) if clen is None else clen
    return sig + struct.pack("<HHHHIIH", disk, cd_disk, n_here & M16, n_total & M16, cd_size & M32, cd_off & M32, clen) + comment


def end_record64(n_here, n_total, cd_size, cd_off, disk=0, cd_disk=0, sig=SIG_END64, extensible=b""):
    return sig + struct.pack("<QHHIIQQQQ", 44 + len(extensible), 45, 45, disk, cd_disk, n_here, n_total, cd_size & (2**64 - 1), cd_off & (2**64 - 1)) + extensible


def locator64(end64_off, disk=0, total_disks=1, sig=SIG_LOC64):
    return sig + struct.pack("<IQI", disk, end64_off & (2**64 - 1), total_disks)


class Spec:
    """One entry.  payload is the content; method STORED / DEFLATED compress it (any other method number stores the bytes as they
    are).  `pre` bytes are written in front of the local header (alignment, decoys).  z64 names the directory fields ("usize",
    "csize", "lho") that are written as 0xFFFFFFFF with their value in an id-1 subfield; extra_front / extra_back are subfields
    around it.  cd and local override any argument of central_record / local_header by name; data replaces the entry's bytes."""

    def __init__(self, name, payload=b"", method=DEFLATED, flags=0, pre=b"", z64=(), extra_front=b"", extra_back=b"", comment=b"", cd=None,
                 local=None, data=None, level=6):
        self.name = name if isinstance(name, bytes) else name.encode()
        self.payload, self.method, self.flags, self.pre, self.z64 = payload, method, flags, pre, tuple(z64)
        self.extra_front, self.extra_back, self.comment = extra_front, extra_back, comment
        self.cd, self.local, self.level = dict(cd or {}), dict(local or {}), level
        self.data = data if data is not None else (raw_deflate(payload, level) if method == DEFLATED else payload)


class Archive:
    """what build() made: the bytes, and where it put things"""

    def __init__(self):
        self.data = b""
        self.header_off, self.data_off, self.record_off = [], [], []
        self.cd_off = self.cd_size = self.eocd_off = self.end64_off = 0


def build(specs, comment=b"", zip64=False, gap=b"", end=None, end64=None, loc=None, cd_tail=b"", tail=b"", between=b""):
    """The archive of `specs`: local headers and data, `gap` bytes, the directory (cd_tail: bytes behind its last record that
    count as part of it), with zip64 the ZIP64 end record and its locator (`between`: bytes between the two), the end record,
    `tail` behind everything.  end / end64 / loc override arguments of end_record / end_record64 / locator64 by name."""
    a = Archive()
    out = bytearray()
    for s in specs:
        out += s.pre
        a.header_off.append(len(out))
        crc = zlib.crc32(s.payload)
        kw = dict(name=s.name, method=s.method, flags=s.flags, crc=crc, csize=len(s.data), usize=len(s.payload))
        kw.update(s.local)
        out += local_header(**kw)
        a.data_off.append(len(out))
        out += s.data
    out += gap
    a.cd_off = len(out)
    for s, lho in zip(specs, a.header_off):
        crc = zlib.crc32(s.payload)
        vals = {"usize": len(s.payload), "csize": len(s.data), "lho": lho}
        over = dict(s.cd)
        for k in ("usize", "csize", "lho"):
            if k in s.z64 and k in over:  # the true value of a field that goes into the id-1 subfield
                vals[k] = over.pop(k)
        extra = s.extra_front
        if s.z64:
            extra += zip64_extra([vals[k] for k in ("usize", "csize", "lho") if k in s.z64])
        extra += s.extra_back
        kw = dict(name=s.name, method=s.method, flags=s.flags, crc=crc, extra=extra, comment=s.comment)
        kw.update({k: (M32 if k in s.z64 else v) for k, v in vals.items()})
        kw.update(over)
        a.record_off.append(len(out))
        out += central_record(**kw)
    out += cd_tail
    a.cd_size = len(out) - a.cd_off
    n = len(specs)
    if zip64:
        a.end64_off = len(out)
        kw = dict(n_here=n, n_total=n, cd_size=a.cd_size, cd_off=a.cd_off)
        kw.update(end64 or {})
        out += end_record64(**kw)
        out += between
        kw = dict(end64_off=a.end64_off)
        kw.update(loc or {})
        out += locator64(**kw)
    a.eocd_off = len(out)
    kw = dict(n_here=n, n_total=n, cd_size=a.cd_size, cd_off=a.cd_off, comment=comment)
    kw.update(end or {})
    out += end_record(**kw)
    out += tail
    a.data = bytes(out)
    return a
