"""Writing tar images on the GPU: chip_tar_write against chip_tar_write_host on every case of tests/tar_write_cases.py (bytes,
entries, summary, poison in front of and behind a shifted `out`); too little room and every bad source on the device, the lowest
index winning across workgroups; 70 000 members of 0 to 3 bytes, whose scans take more than one partial block and whose copy tiles
hold up to eight headers; one member of 3 MiB, many tiles inside one piece; a round trip tar_write_items -> tar_open and tarfile;
the slot reused at a smaller and a larger n, and trimmed.  The host writer is pinned to the rules of include/compu_hip.h, to tarfile
and to chip_tar_plan_host by tests/test_tar_write_cpu.py.  Without the feature every test here fails at the missing symbol."""
import ctypes as C
import io
import tarfile

import numpy as np
import pytest

import tar_ref as R
import tar_write_cases as TC
import tar_write_ref as WR
from test_tar_write_cpu import arrays, run_host

pytestmark = pytest.mark.gpu

CASES = TC.all_cases()
IDS = [c.name for c in CASES]
POISON = 0xA7
FRONT = 16  # poisoned bytes in front of `out`


def stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class Uploaded:
    """a case's arrays in device memory, made once per case"""

    def __init__(self, torch, case):
        import compu_amd

        src, names, content = arrays(case)
        self.case, self.n = case, len(case.sources)
        self.src = dev(torch, src.view(np.uint8).reshape(-1, 64)) if self.n else None
        self.names, self.content = dev(torch, names), dev(torch, content)
        self.lib = compu_amd.lib()


def run_device(torch, up, out_cap, shift=0, want_entries=True):
    """chip_tar_write into a poisoned device buffer, `out` FRONT + shift bytes behind its start and 16 poisoned bytes behind out_cap:
    (the whole buffer as bytes, the entries array as bytes with one poisoned row behind it, summary tuple)"""
    from compu_amd.api import TarWriteSummary, _TarWriteSummary

    case, n = up.case, up.n
    buf = torch.full((FRONT + shift + out_cap + 16,), POISON, dtype=torch.uint8, device="cuda")
    entries = torch.full((n + 1, 72), POISON, dtype=torch.uint8, device="cuda")
    raw = _TarWriteSummary()
    rc = up.lib.chip_tar_write(
        n, ptr(up.src), ptr(up.names) if len(case.names) else None, len(case.names), ptr(up.content) if case.content_len else None, case.content_len,
        case.flags, case.record_bytes, C.c_void_p(buf.data_ptr() + FRONT + shift) if out_cap else None, out_cap,
        C.c_void_p(entries.data_ptr()) if want_entries else None, C.byref(raw), stream_ptr(torch))
    assert rc == 0
    return buf.cpu().numpy().tobytes(), entries.cpu().numpy().tobytes(), TarWriteSummary(raw).as_tuple()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_image_equals_the_host_image(gpu, case):
    host_buf, rows, summ, host_rows = run_host(case)
    assert summ == case.want()[2]
    up = Uploaded(gpu, case)
    n = len(case.sources)
    row_poison = bytes([POISON]) * 72
    if summ[6] != WR.OK:  # a bad source, or an arithmetic case run without room
        buf, ent, got = run_device(gpu, up, 0)
        assert got == summ and buf == bytes([POISON]) * len(buf)
        assert ent == (row_poison * (n + 1) if summ[6] == WR.BAD_SOURCE else host_rows + row_poison)
        if summ[6] == WR.BAD_SOURCE:  # with room as well: nothing but the summary
            buf, ent, got = run_device(gpu, up, 20480)
            assert got == summ and buf == bytes([POISON]) * len(buf) and ent == row_poison * (n + 1)
        return
    want = host_buf[:summ[2]]
    for shift in (0, 1, 7, 8, 15, 16):
        buf, ent, got = run_device(gpu, up, summ[2], shift)
        assert got == summ and ent == host_rows + row_poison
        assert buf == bytes([POISON]) * (FRONT + shift) + want + bytes([POISON]) * 16, shift
    # more room than needed, and no entries array
    buf, ent, got = run_device(gpu, up, summ[2] + 5, 3, want_entries=False)
    assert got == summ and ent == row_poison * (n + 1) and buf == bytes([POISON]) * (FRONT + 3) + want + bytes([POISON]) * 21
    # too little room: the exact length, the entries, nothing written
    for cap in (summ[2] - 1, 0):
        buf, ent, got = run_device(gpu, up, cap)
        assert got == summ[:6] + (WR.NEED_OUTPUT,) and ent == host_rows + row_poison and buf == bytes([POISON]) * len(buf)


def test_the_lowest_bad_index_wins_across_workgroups(gpu):
    """7 000 small members with bad records 3 000 apart, in different workgroups of the check: the lower one is answered, and neither
    `out` nor the entries are written"""
    many = 7000
    members = [TC.Member(b"f%04d" % k, b"x" * (k % 5)) for k in range(many)]
    base = TC.lay_out("many", members)
    for lower, rule in ((1500, "mode"), (4499, "nul"), (64, "link")):
        s = [list(r) for r in base.sources]
        s[4500][10] = ord("x")
        if rule == "mode":
            s[lower][7] = 0o10000000
        elif rule == "nul":
            s[lower][5] += 1  # (the name now ends in the NUL that the layout puts behind it)
        else:
            s[lower][3], s[lower][6] = len(base.names) - 100, 101  # a link name of 101 bytes that ends one byte too far
        case = TC.Case("many_bad", [tuple(r) for r in s], base.names, base.content)
        assert case.want()[2] == (many, 0, 0, 0, 0, lower, WR.BAD_SOURCE)
        buf, ent, got = run_device(gpu, Uploaded(gpu, case), 1 << 16)
        assert got == case.want()[2] and buf == bytes([POISON]) * len(buf) and ent == bytes([POISON]) * 72 * (many + 1)


@pytest.mark.parametrize("flags", TC.FLAGSETS, ids=[TC.FLAG_NAMES[f] for f in TC.FLAGSETS])
def test_seventy_thousand_members(gpu, flags):
    """sizes 0 to 3: a group is one or two blocks (three or four with the forced pax records), so a copy tile holds up to eight
    headers and the scans take 69 partial blocks; every 1 000th member has a long name"""
    import compu_amd

    n = 70000
    names = bytearray()
    sources = []
    content = bytes(range(1, 200))
    for k in range(n):
        nm = b"m/%05d" % k if k % 1000 else b"long/" + b"%05d" % k * 30
        sources.append((k % 190, k % 4, len(names), 0, k, len(nm), 0, 0o600 + k % 64, k % 7, k % 5, ord("0"), (0, 0, 0)))
        names += nm
    case = TC.Case("seventy_thousand", sources, bytes(names), content, flags, 512)
    want, rows, summ = case.want()
    up = Uploaded(gpu, case)
    buf, ent, got = run_device(gpu, up, summ[2], shift=9)
    assert got == summ
    assert buf == bytes([POISON]) * (FRONT + 9) + want + bytes([POISON]) * 16
    assert [tuple(int(v) for v in e) for e in np.frombuffer(ent[:72 * n], compu_amd.tar_entry_dtype()).tolist()] == rows
    if flags == 0:
        with tarfile.open(fileobj=io.BytesIO(want), mode="r:") as tf:
            infos = tf.getmembers()
        assert len(infos) == n and infos[1].name == "m/00001" and infos[-1].name == "m/69999" and infos[3000].name == "long/" + "03000" * 30
        assert [ti.size for ti in infos[:6]] == [0, 1, 2, 3, 0, 1]


def test_one_member_of_three_mebibytes(gpu):
    """many tiles inside one piece, at an odd data offset and an odd `out`"""
    size = 3 * (1 << 20) + 5
    pay = TC.payload(size, 3)
    case = TC.lay_out("large", [TC.Member(b"small", b"abc"), TC.Member(b"dir/large.bin", pay), TC.Member(b"after", b"z" * 513)], 0, 512)
    want, rows, summ = case.want()
    up = Uploaded(gpu, case)
    for shift in (0, 5):
        buf, ent, got = run_device(gpu, up, summ[2], shift)
        assert got == summ and buf == bytes([POISON]) * (FRONT + shift) + want + bytes([POISON]) * 16
    with tarfile.open(fileobj=io.BytesIO(want), mode="r:") as tf:
        assert tf.extractfile("dir/large.bin").read() == pay


def test_round_trip_through_tar_open(gpu):
    import compu_amd

    rng = np.random.default_rng(5)
    blobs = {"shard/0000.bin": rng.integers(0, 256, 70001, dtype=np.uint8).tobytes(), "shard/empty": b"", "meta.json": b'{"n": 2}\n',
             "deep/" + "d" * 150 + "/" + "f" * 90: b"split", "x" * 300: b"long"}
    items = [("shard/", b"")]
    for k, (name, blob) in enumerate(blobs.items()):
        c = blob if k % 2 else gpu.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
        items.append((name, c) if k % 3 else (name, c, 0o600, 1700000000 + k))
    for flags in (0, compu_amd.TW_GNU):
        image, entries, summ = compu_amd.tar_write_items(items, flags=flags)
        assert summ.status == compu_amd.TarWriteStatus.Ok and summ.n_entries == len(items) and image.numel() == summ.out_len
        assert summ.n_ext == (1 if flags == 0 else 2)
        arch = compu_amd.tar_open(image, summ.out_len)
        assert arch.names == [b"shard/"] + [n.encode() for n in blobs]
        assert arch.entries.tobytes() == entries.cpu().numpy().tobytes() and arch.summary.zero_blocks == 2
        for name, blob in blobs.items():
            assert arch.member(name).cpu().numpy().tobytes() == blob
        with tarfile.open(fileobj=io.BytesIO(image.cpu().numpy().tobytes()), mode="r:") as tf:
            infos = tf.getmembers()
            assert [ti.name for ti in infos] == ["shard"] + list(blobs) and infos[0].isdir() and infos[0].mode == 0o755
            assert [(ti.mode, ti.mtime) for ti in infos[1:3]] == [(0o600, 1700000000), (0o644, 0)]
            for name, blob in blobs.items():
                assert tf.extractfile(name).read() == blob
    # the image goes on to the file encoder, and comes back through tar_open's decode
    packed, fsumm = compu_amd.encode_file(compu_amd.FMT_ZSTD, 3, image, summ.out_len)
    arch = compu_amd.tar_open(packed, fsumm.out_len)
    assert arch.member("meta.json").cpu().numpy().tobytes() == blobs["meta.json"]
    image, entries, summ = compu_amd.tar_write_items([])
    assert image.cpu().numpy().tobytes() == bytes(10240) and entries.shape[0] == 0 and summ.n_entries == 0


def test_the_slot_is_reused_and_trimmed(gpu):
    """calls on one stream reuse the slot: a smaller n behind a larger one, a larger one behind both; chip_trim() releases it and the
    next call allocates again"""
    import compu_amd

    case = TC.by_name("sizes_pax")
    src, names, content = arrays(case)
    d_src, d_names, d_content = dev(gpu, src.view(np.uint8).reshape(-1, 64)), dev(gpu, names), dev(gpu, content)
    first, e1, s1 = compu_amd.tar_write(d_src, d_names, d_content)
    small, _, s2 = compu_amd.tar_write(d_src[:3].contiguous(), d_names, d_content)
    large, _, s3 = compu_amd.tar_write(d_src.repeat(300, 1), d_names, d_content)
    again, e4, s4 = compu_amd.tar_write(d_src, d_names, d_content)
    assert s1.as_tuple() == s4.as_tuple() == case.want()[2] and s2.n_entries == 3 and s3.n_entries == 300 * len(case.sources)
    assert first.cpu().numpy().tobytes() == again.cpu().numpy().tobytes() == case.want()[0]
    assert small.cpu().numpy().tobytes()[:s2.end_off] == case.want()[0][:s2.end_off]
    assert large.cpu().numpy().tobytes()[:s3.end_off] == case.want()[0][:s1.end_off] * 300
    compu_amd.trim()
    after, e5, s5 = compu_amd.tar_write(d_src, d_names, d_content)
    assert s5.as_tuple() == s1.as_tuple() and after.cpu().numpy().tobytes() == case.want()[0] and e5.cpu().numpy().tobytes() == e1.cpu().numpy().tobytes()
    compu_amd.trim()
    planned, psumm = compu_amd.tar_plan(after, s5.out_len)
    assert psumm.status == compu_amd.TarStatus.Ok and planned.cpu().numpy().tobytes() == e1.cpu().numpy().tobytes()
    assert R.plan(case.want()[0])[1] == psumm.as_tuple()
