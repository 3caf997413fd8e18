"""The rules of include/compu_hip.h ("ZIP archives: writing"), restated in Python on top of the record functions of
tests/zip_writer.py: assemble(sources, names, content, comp, crcs, flags) -> (bytes, rows, summary) with the tuples the tests
compare with chip_zip_assemble_host, chip_zip_assemble and chip_zip_write.
  source   (data_off, size, name_off, name_len, method, dos_time, dos_date)
  comp     None (every entry is stored), or (stream bytes, comp_off list, comp_len list)
  row      (header_off, data_off, comp_size, size, name_off, crc32, name_len, method, flags, pad, status): zip_ref.plan's row
  summary  (n_entries, n_deflated, out_len, cd_off, cd_size, eocd_off, bad_index, status, zip64)
out_cap smaller than the archive (0 for the cases that are pure arithmetic) answers NEED_OUTPUT with rows and summary and never
looks at `content` or the streams; content_len then states a length the bytes need not have."""
import zip_ref as R
import zip_writer as W

OK, NEED_OUTPUT, BAD_SOURCE = 0, 1, 2
STORE, DEFLATE = 0, 8
ZW_ZIP64, ZW_UTF8 = 1, 2
M32 = 0xFFFFFFFF


def pack_streams(streams):
    """per-entry streams (bytes, or None for an entry without one) end to end: the comp triple"""
    blob, off, ln = bytearray(), [], []
    for s in streams:
        off.append(len(blob))
        ln.append(len(s or b""))
        blob += s or b""
    return bytes(blob), off, ln


def bound(n, names_total, content_total):
    v = content_total + 2 * names_total + 124 * n + 98
    return v if v < 1 << 64 else 0


def assemble(sources, names, content, comp, crcs, flags, out_cap=None, content_len=None):
    n = len(sources)
    force = bool(flags & ZW_ZIP64)
    gp = 0x0800 if flags & ZW_UTF8 else 0
    content_len = len(content) if content_len is None else content_len
    comp_all = len(comp[0]) if comp else 0
    chosen = []  # (method, c, where the data comes from)
    for i, (data_off, size, name_off, name_len, method, _, _) in enumerate(sources):
        bad = method not in (STORE, DEFLATE) or data_off + size > content_len or name_off + name_len > len(names)
        defl = not bad and method == DEFLATE and comp is not None and 0 < comp[2][i] < size
        if defl and comp[1][i] + comp[2][i] > comp_all:
            bad = True
        if bad:
            return b"", [], (n, 0, 0, 0, 0, 0, i, BAD_SOURCE, 0)
        chosen.append((DEFLATE, comp[2][i], comp[1][i]) if defl else (STORE, size, data_off))
    # the layout
    header_off, at = [], 0
    for (data_off, size, name_off, name_len, *_), (method, c, _) in zip(sources, chosen):
        header_off.append(at)
        zs = force or size >= M32 or c >= M32
        at += 30 + name_len + (20 if zs else 0) + c
    cd_off = at
    records, rows, rel = [], [], 0
    for i, ((data_off, size, name_off, name_len, _, dos_time, dos_date), (method, c, src)) in enumerate(zip(sources, chosen)):
        zs, zl = force or size >= M32 or c >= M32, force or header_off[i] >= M32
        vals = ([size, c] if zs else []) + ([header_off[i]] if zl else [])
        extra = W.zip64_extra(vals) if vals else b""
        version = 45 if vals else 20 if method == DEFLATE else 10
        name = names[name_off:name_off + name_len]
        rec = W.central_record(name, method, gp, crcs[i], M32 if zs else c, M32 if zs else size, M32 if zl else header_off[i], extra=extra, made_by=version,
                               version=version, dos_time=dos_time, dos_date=dos_date)
        lextra = W.zip64_extra([size, c]) if zs else b""
        local = W.local_header(name, method, gp, crcs[i], M32 if zs else c, M32 if zs else size, extra=lextra, version=version, dos_time=dos_time,
                               dos_date=dos_date)
        status = R.ENT_TOO_LARGE if method == DEFLATE and (c > R.UNIT_IN_MAX or size > R.UNIT_OUT_MAX) else R.ENT_OK
        rows.append((header_off[i], header_off[i] + len(local), c, size, cd_off + rel + 46, crcs[i] & M32, name_len, method, gp, 0, status))
        records.append((local, rec, method, c, src))
        rel += len(rec)
    cd_size = rel
    z = force or n >= 0xFFFF or cd_size >= M32 or cd_off >= M32
    end = b""
    if z:
        end = W.end_record64(n, n, cd_size, cd_off) + W.locator64(cd_off + cd_size)
    end += W.end_record(min(n, 0xFFFF), min(n, 0xFFFF), min(cd_size, M32), min(cd_off, M32))
    out_len = cd_off + cd_size + len(end)
    n_deflated = sum(1 for m, _, _ in chosen if m == DEFLATE)
    summary = (n, n_deflated, out_len, cd_off, cd_size, out_len - 22, 0, OK, int(z))
    if out_cap is not None and out_len > out_cap:
        return b"", rows, summary[:7] + (NEED_OUTPUT, int(z))
    out = bytearray()
    for local, rec, method, c, src in records:
        out += local
        out += (comp[0] if method == DEFLATE else content)[src:src + c]
    assert len(out) == cd_off
    for local, rec, *_ in records:
        out += rec
    out += end
    assert len(out) == out_len
    return bytes(out), rows, summary
