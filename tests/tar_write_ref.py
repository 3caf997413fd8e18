"""The rules that define chip_tar_write (include/compu_hip.h, "tar archives: writing"), written down once more in Python from that
text and independent of the C code: the accepted sources, a header block, the pax and the GNU group, the end.
write(sources, names, content_len, content, flags, record_bytes, out_cap) -> (image bytes or None, entry rows, summary tuple); a
source is a tuple in the field order of chip_tar_source without its pad (data_off, size, name_off, link_off, mtime, name_len,
link_len, mode, uid, gid, typeflag) or with it as a twelfth value; the rows are in the field order of chip_tar_entry, the summary
as TarWriteSummary.as_tuple() gives it."""

OK, NEED_OUTPUT, BAD_SOURCE = 0, 1, 2
TW_GNU, TW_FORCE_EXT = 1, 2
NAME_MAX = 65535
NAME_GNU, NAME_PAX, LINK_GNU, LINK_PAX, SIZE_PAX, SIZE_BASE256 = 1, 2, 4, 8, 16, 32
OCT7, OCT11 = 8 ** 7, 8 ** 11
U64 = 1 << 64


def up(v, m):
    return (v + m - 1) // m * m


def record_of(record_bytes):
    return record_bytes or 10240


def bound(n, names_total, content_total, record_bytes=0):
    if record_bytes % 512 or record_bytes > 1 << 20:
        return 0
    v = up(content_total + 2 * names_total + 3072 * n + 1024, record_of(record_bytes))
    # (the C function forms the sum, and the round-up, in 64 bits)
    return v if content_total + 2 * names_total + 3072 * n + 1024 + record_of(record_bytes) - 1 < U64 else 0


def source_ok(s, names, content_len):
    data_off, size, name_off, link_off, mtime, name_len, link_len, mode, uid, gid, typeflag = s[:11]
    pad = s[11] if len(s) > 11 else 0
    if isinstance(pad, (tuple, list)):  # the three bytes
        pad = int(any(pad))
    if not ord("0") <= typeflag <= ord("7"):
        return False
    if ord("1") <= typeflag <= ord("6") and size != 0:
        return False
    if not 1 <= name_len <= NAME_MAX or link_len > NAME_MAX:
        return False
    if name_off + name_len > len(names) or link_off + link_len > len(names) or data_off + size > content_len:
        return False  # (Python's integers do not wrap)
    if b"\0" in names[name_off:name_off + name_len] or b"\0" in names[link_off:link_off + link_len]:
        return False
    if mode > 0o7777777 or uid >= OCT7 or gid >= OCT7 or not 0 <= mtime < OCT11:
        return False
    return pad == 0


def header(name, mode, uid, gid, size, mtime, typeflag, link, prefix, gnu, base256=False):
    assert len(name) <= 100 and len(link) <= 100 and len(prefix) <= 155
    h = bytearray(512)
    h[0:len(name)] = name
    h[100:108] = b"%07o\0" % mode
    h[108:116] = b"%07o\0" % uid
    h[116:124] = b"%07o\0" % gid
    h[124:136] = b"\x80" + size.to_bytes(11, "big") if base256 else b"%011o\0" % size
    h[136:148] = b"%011o\0" % mtime
    h[148:156] = b" " * 8
    h[156] = typeflag
    h[157:157 + len(link)] = link
    h[257:265] = b"ustar  \0" if gnu else b"ustar\x0000"
    h[329:337] = b"0000000\0"
    h[337:345] = b"0000000\0"
    h[345:345 + len(prefix)] = prefix
    h[148:156] = b"%06o\0 " % sum(h)
    return bytes(h)


def record(key, value):
    body = b" " + key + b"=" + value + b"\n"
    n = len(body) + 1
    while len(str(n)) + len(body) != n:
        n += 1
    return str(n).encode() + body


def split(name):
    """the largest p the prefix split allows, None without one"""
    best = None
    for p in range(1, min(155, len(name) - 1) + 1):
        if name[p:p + 1] == b"/" and 1 <= len(name) - p - 1 <= 100:
            best = p
    return best


def padded(data):
    return data + bytes(up(len(data), 512) - len(data))


def group(s, names, content, g, flags):
    """(the group's bytes without the content and its padding -- the front --, the entry row, extension headers, front length)"""
    data_off, size, name_off, link_off, mtime, name_len, link_len, mode, uid, gid, typeflag = s[:11]
    name, link = names[name_off:name_off + name_len], names[link_off:link_off + link_len]
    gnu, big = bool(flags & TW_GNU), size >= OCT11 or bool(flags & TW_FORCE_EXT)
    front, f, n_ext = b"", 0, 0
    e_name_off = e_link_off = None
    prefix, field, e_name_len, prefix_len = b"", name[:100], name_len, 0
    if gnu:
        if link_len > 100:
            front += header(b"././@LongLink", 0, 0, 0, link_len + 1, 0, ord("K"), b"", b"", True)
            e_link_off, f, n_ext = g + len(front), f | LINK_GNU, n_ext + 1
            front += padded(link + b"\0")
        if name_len > 100:
            front += header(b"././@LongLink", 0, 0, 0, name_len + 1, 0, ord("L"), b"", b"", True)
            e_name_off, f, n_ext = g + len(front), f | NAME_GNU, n_ext + 1
            front += padded(name + b"\0")
        if big:
            f |= SIZE_BASE256
        member = header(field, mode, uid, gid, size, mtime, typeflag, link[:100], b"", True, base256=big)
    else:
        records = b""
        if name_len > 100:
            p = split(name)
            if p is None:
                r = record(b"path", name)
                e_name_off, f = g + 512 + len(records) + r.index(b"=") + 1, f | NAME_PAX
                records += r
            else:
                prefix, field, e_name_len, prefix_len = name[:p], name[p + 1:], name_len - p - 1, p
        if link_len > 100:
            r = record(b"linkpath", link)
            e_link_off, f = g + 512 + len(records) + r.index(b"=") + 1, f | LINK_PAX
            records += r
        if big:
            records += record(b"size", str(size).encode())
            f |= SIZE_PAX
        if records:
            front = header(b"././@PaxHeader", 0o644, 0, 0, len(records), mtime, ord("x"), b"", b"", False) + padded(records)
            n_ext = 1
        member = header(field, mode, uid, gid, size if size < OCT11 else 0, mtime, typeflag, link[:100], prefix, False)
    hdr = g + len(front)
    row = (g, hdr, hdr + 512, size, hdr if e_name_off is None else e_name_off, hdr + 157 if e_link_off is None else e_link_off, mtime,
           e_name_len, link_len, mode, prefix_len, typeflag, f)
    return front + member, row, n_ext


def write(sources, names, content_len, content, flags=0, record_bytes=0, out_cap=None):
    """content may be None (or shorter than content_len) for a call that never reads it: out_cap below the image's length"""
    names = bytes(names)
    n = len(sources)
    for i, s in enumerate(sources):
        if not source_ok(s, names, content_len):
            return None, [], (n, 0, 0, 0, 0, i, BAD_SOURCE)
    rows, fronts, g, n_ext, total = [], [], 0, 0, 0
    for s in sources:
        front, row, ext = group(s, names, content, g, flags)
        rows.append(row)
        fronts.append(front)
        g += len(front) + up(s[1], 512)
        n_ext += ext
        total += s[1]
    out_len = up(g + 1024, record_of(record_bytes))
    if out_cap is not None and out_len > out_cap:
        return None, rows, (n, n_ext, out_len, g, total, 0, NEED_OUTPUT)
    parts = []
    for s, front in zip(sources, fronts):
        parts.append(front)
        parts.append(padded(bytes(content[s[0]:s[0] + s[1]])))
    parts.append(bytes(out_len - g))
    image = b"".join(parts)
    assert len(image) == out_len
    return image, rows, (n, n_ext, out_len, g, total, 0, OK)
