"""The walk of a tar image that defines chip_tar_plan (include/compu_hip.h, "tar archives"), written down once more in Python from
that text: number fields, the header test, the groups of extension headers and member header, the pax records, the stop.
plan(data, max_entries) -> (records, summary): the records as tuples in the field order of chip_tar_entry, the summary as
TarPlanSummary.as_tuple() gives it."""

OK, TRUNCATED, BAD_HEADER, UNSUPPORTED = 0, 1, 2, 3
EXT_MAX, EXT_BYTES = 16, 1 << 20
NAME_GNU, NAME_PAX, LINK_GNU, LINK_PAX, SIZE_PAX, SIZE_BASE256 = 1, 2, 4, 8, 16, 32
FIELDS = ("group_off", "header_off", "data_off", "size", "name_off", "link_off", "mtime", "name_len", "link_len", "mode", "prefix_len",
          "typeflag", "flags")


def up512(v):
    return (v + 511) // 512 * 512


def number(field):
    """(value, base256) of a number field, None when it is invalid"""
    if field[0] == 0x80:
        v = int.from_bytes(field[1:], "big")
        return None if v >= 1 << 63 else (v, True)
    if field[0] == 0xFF:
        return None
    rest = field.lstrip(b" ")
    digits = 0
    while digits < len(rest) and 0x30 <= rest[digits] <= 0x37:
        digits += 1
    if digits < len(rest) and rest[digits] not in (0, 0x20):
        return None
    return (int(rest[:digits], 8) if digits else 0, False)


def text(field):
    """a field up to its first NUL"""
    return field.split(b"\0", 1)[0]


class Memo:
    """What a walk of data[:n] may keep for the walk of another prefix of the same data.  The rule looks at the length only in
    comparisons `x > n`: the header test in `p + 512 > n`, a group where an extension header's successor or the group's end must
    lie inside the image.  So the rest of the header test is a property of the position, and a group that was read whole is read
    the same in every prefix that holds the largest x it compared."""

    def __init__(self):
        self.headers, self.groups = {}, {}


def is_header(data, p, n=None, memo=None):
    n = len(data) if n is None else n
    if p % 512 or p + 512 > n:
        return False
    if memo is None:
        return header_fields_ok(data, p)
    if p not in memo.headers:
        memo.headers[p] = header_fields_ok(data, p)
    return memo.headers[p]


def header_fields_ok(data, p):
    """is_header(p) behind its first line: the magic, the two number fields, the checksum"""
    h = data[p:p + 512]
    if h[257:262] != b"ustar":
        return False
    size, chk = number(h[124:136]), number(h[148:156])
    if size is None or chk is None:
        return False
    counted = h[:148] + b" " * 8 + h[156:]
    unsigned = sum(counted)
    signed = sum(c - 256 if c > 127 else c for c in counted)
    return chk[0] in (unsigned, signed)


class Stop(Exception):
    def __init__(self, status, bad_off):
        self.status, self.bad_off = status, bad_off


def pax(data, q, body, over):
    """applies the records of the x header at q, whose data is `body` at offset q + 512"""
    at = 0
    while at < len(body):
        k = at
        while k < len(body) and k - at < 10 and 0x30 <= body[k] <= 0x39:
            k += 1
        if k == at or k >= len(body) or body[k] != 0x20:
            raise Stop(BAD_HEADER, q)
        n = int(body[at:k])
        if at + n > len(body) or n < k - at + 2 or body[at + n - 1] != 0x0A:
            raise Stop(BAD_HEADER, q)
        key, eq, value = body[k + 1:at + n - 1].partition(b"=")
        if not eq:
            raise Stop(BAD_HEADER, q)
        value_off = q + 512 + k + 1 + len(key) + 1
        if key.startswith(b"GNU.sparse."):
            raise Stop(UNSUPPORTED, q)
        if key == b"path":
            over["name"] = (value_off, len(value), NAME_PAX)
        elif key == b"linkpath":
            over["link"] = (value_off, len(value), LINK_PAX)
        elif key == b"size":
            if not 1 <= len(value) <= 19 or not value.isdigit():
                raise Stop(BAD_HEADER, q)
            over["size"] = int(value)
        at += n


def group(data, e, n=None, memo=None):
    """the group at e (is_header(e) holds): ("global", end) or ("member", end, record)"""
    n = len(data) if n is None else n
    if memo is None:
        return read_group(data, e, n, [], None)
    if e in memo.groups and memo.groups[e][1] <= n:
        return memo.groups[e][0]
    compared = []
    g = read_group(data, e, n, compared, memo)  # (a group that stops raises, and is read again in the next prefix)
    memo.groups[e] = (g, max(compared))
    return g


def read_group(data, e, n, compared, memo):
    """group(); `compared` collects every offset that is compared with n"""
    q, ext, over = e, 0, {}
    while True:
        h = data[q:q + 512]
        t = h[156:157]
        s, base256 = number(h[124:136])
        if t in (b"L", b"K", b"x"):
            ext += 1
            if ext > EXT_MAX or s > EXT_BYTES:
                raise Stop(UNSUPPORTED, q)
            q2 = q + 512 + up512(s)
            compared.append(q2 + 512)
            if q2 + 512 > n:
                raise Stop(TRUNCATED, q)
            if not is_header(data, q2, n, memo):
                raise Stop(BAD_HEADER, q2)
            body = data[q + 512:q + 512 + s]
            if t == b"L":
                over["name"] = (q + 512, len(text(body)), NAME_GNU)
            elif t == b"K":
                over["link"] = (q + 512, len(text(body)), LINK_GNU)
            else:
                pax(data, q, body, over)
            q = q2
            continue
        if t == b"g":
            if q != e:
                raise Stop(BAD_HEADER, q)
            end = q + 512 + up512(s)
            compared.append(end)
            if end > n:
                raise Stop(TRUNCATED, q)
            return ("global", end)
        if t in (b"S", b"M"):
            raise Stop(UNSUPPORTED, q)
        flags = 0
        if "size" in over:
            size, flags = over["size"], flags | SIZE_PAX
        else:
            size, flags = s, flags | (SIZE_BASE256 if base256 else 0)
        if t in (b"1", b"2", b"3", b"4", b"5", b"6"):
            size = 0
        end = q + 512 + up512(size)
        compared.append(end)
        if end > n:
            raise Stop(TRUNCATED, q)
        if "name" in over:
            name_off, name_len, f = over["name"]
            prefix_len, flags = 0, flags | f
        else:
            name_off, name_len, prefix_len = q, len(text(h[0:100])), len(text(h[345:500]))
        if "link" in over:
            link_off, link_len, f = over["link"]
            flags |= f
        else:
            link_off, link_len = q + 157, len(text(h[157:257]))
        mtime, mode = number(h[136:148]), number(h[100:108])
        rec = (e, q, q + 512, size, name_off, link_off, mtime[0] if mtime else 0, name_len, link_len, (mode[0] if mode else 0) & 0xFFFFFFFF,
               prefix_len, t[0], flags)
        return ("member", end, rec)


def plan(data, max_entries=None, n=None, memo=None):
    """the plan of data[:n] (n None: of all of data); memo: a Memo kept for the prefixes of this one `data`"""
    data = bytes(data) if not isinstance(data, bytes) else data
    n, e = (len(data) if n is None else n), 0
    assert n <= len(data)
    records, n_global, total, zero_blocks = [], 0, 0, 0
    while True:
        status, bad = OK, e
        if e == n:
            break
        if n - e < 512:
            status = TRUNCATED
            break
        if not any(data[e:e + 512]):
            zero_blocks = 2 if e + 1024 <= n and not any(data[e + 512:e + 1024]) else 1
            break
        if not is_header(data, e, n, memo):
            status = BAD_HEADER
            break
        try:
            g = group(data, e, n, memo)
        except Stop as stop:
            status, bad = stop.status, stop.bad_off
            break
        if g[0] == "global":
            n_global += 1
        else:
            records.append(g[2])
            total += g[2][3]
        e = g[1]
    kept = records if max_entries is None else records[:max_entries]
    return kept, (len(records), n_global, total, e, bad, status, zero_blocks)


def names(records, data):
    out = []
    for r in records:
        rec = dict(zip(FIELDS, r))
        name = data[rec["name_off"]:rec["name_off"] + rec["name_len"]]
        prefix = data[rec["header_off"] + 345:rec["header_off"] + 345 + rec["prefix_len"]]
        out.append(prefix + b"/" + name if prefix else name)
    return out
