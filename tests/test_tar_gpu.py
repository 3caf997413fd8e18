"""tar archives on the GPU: chip_tar_plan against chip_tar_plan_host on every case of tests/tar_cases.py -- every record byte, every
summary field, poisoned arrays, the rows behind the count untouched, count-then-fill, the image at every 4-byte shift -- and on the
cuts (every block of the three tarfile archives, 16 sampled cuts of the 3 000-member one, the odd places of all); tar_open on a
plain image, the image gzipped and a zstd frame of it, every member's bytes and name against tarfile; a damaged image behind a clean
gzip stream; two host threads on two streams; chip_trim.  The host plan is pinned to the walk of include/compu_hip.h and to tarfile
by tests/test_tar_cpu.py.  Without the feature every test here fails at the missing symbol."""
import ctypes as C
import io
import tarfile
import threading
import zlib

import numpy as np
import pytest

import tar_cases as T

pytestmark = pytest.mark.gpu

CASES = T.all_cases()
IDS = [c.name for c in CASES]
POISON = 0xA7


def upload(torch, data, shift=0, fill=0xA5):
    """`data` in a device tensor at a 4-byte aligned start `shift` bytes behind a 16-byte aligned one, padded to a multiple of 4;
    the bytes around it hold `fill`."""
    room = shift + (len(data) + 3) // 4 * 4 + 4
    t = torch.full((room,), fill, dtype=torch.uint8, device="cuda")
    if len(data):
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    return t[shift:]


@pytest.fixture(scope="module")
def host_plans():
    """the host plan of every case, made once: (record array, summary tuple)"""
    import compu_amd

    plans = {}
    for c in CASES:
        entries, summ = compu_amd.tar_plan_host(c.data)
        plans[c.name] = (entries, summ.as_tuple())
    return plans


def gpu_plan(torch, lib, d_buf, length, max_entries, room, stream=None):
    """chip_tar_plan into a poisoned device array of `room` records: (the records as host bytes, summary tuple)"""
    from compu_amd.api import TarPlanSummary, _TarPlanSummary

    rows = torch.full((room, 72), POISON, dtype=torch.uint8, device="cuda")
    s = _TarPlanSummary()
    sp = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = lib.chip_tar_plan(C.c_void_p(d_buf.data_ptr()) if length else None, length, max_entries, C.c_void_p(rows.data_ptr()) if max_entries else None,
                           C.byref(s), sp)
    assert rc == 0
    return rows.cpu().numpy(), TarPlanSummary(s).as_tuple()


def assert_plan(torch, lib, data, want, shift=0, max_entries=None, fill=0xA5, stream=None):
    """the device plan of `data` equals the host plan `want`, bytewise, and nothing behind the rows it owes is written"""
    entries, summ = want
    n = summ[0]
    m = n + 2 if max_entries is None else max_entries
    got, got_summ = gpu_plan(torch, lib, upload(torch, data, shift, fill), len(data), m, max(n, m) + 3, stream)
    assert got_summ == summ
    k = min(n, m)
    assert got[:k].tobytes() == entries[:k].tobytes()
    assert (got[k:] == POISON).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_plan_equals_the_host_plan(gpu, case, host_plans):
    import compu_amd

    lib, want = compu_amd.lib(), host_plans[case.name]
    assert want[1][5] == case.status
    assert_plan(gpu, lib, case.data, want)
    assert_plan(gpu, lib, case.data, want, shift=4, fill=0x00)
    assert_plan(gpu, lib, case.data, want, shift=8, fill=0x75)  # ('u')
    assert_plan(gpu, lib, case.data, want, shift=12, fill=0xFF)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_plan_equals_the_host_plan_on_the_cuts(gpu, case):
    import compu_amd

    lib = compu_amd.lib()
    for c in T.cuts(case.data, every_block=case.sweep):
        entries, summ = compu_amd.tar_plan_host(case.data[:c])
        assert_plan(gpu, lib, case.data[:c], (entries, summ.as_tuple()), shift=4 * (c % 4), fill=0x00 if c % 2 else 0x72)


def test_plan_counts_then_fills_then_fills_a_part(gpu, host_plans):
    import compu_amd

    lib = compu_amd.lib()
    for name in ("tarfile_gnu", "many_members", "seventeen_extension_headers", "zero_blocks_0"):
        case, want = T.by_name(name), host_plans[name]
        n = want[1][0]
        for m in sorted({0, 1, n // 2, max(n - 1, 0), n, n + 1}):
            assert_plan(gpu, lib, case.data, want, max_entries=m)
    case, want = T.by_name("tarfile_pax"), host_plans["tarfile_pax"]
    d = upload(gpu, case.data)
    entries, summ = compu_amd.tar_plan(d, len(case.data))
    assert summ.as_tuple() == want[1] and entries.cpu().numpy().tobytes() == want[0].tobytes()
    assert compu_amd.tar_plan(d, len(case.data), max_entries=5)[0].cpu().numpy().tobytes() == want[0][:5].tobytes()
    assert compu_amd.tar_names(entries, d) == compu_amd.tar_names(want[0], case.data)
    assert compu_amd.tar_names(entries[:0], d) == []
    assert compu_amd.tar_plan(upload(gpu, b""), 0)[1].as_tuple() == (0, 0, 0, 0, 0, 0, 0)


def tarfile_contents(data):
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:", encoding="utf-8", errors="surrogateescape") as t:
        return [(m.name.encode("utf-8", "surrogateescape"), t.extractfile(m).read() if m.isreg() else b"") for m in t.getmembers()]


def gzipped(data):
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


def zstd_frame(data):
    import zstd_ref

    return zstd_ref.compress(zstd_ref.load(), data, 3, True, True)


@pytest.mark.parametrize("form", ["plain", "gzip", "zstd"])
def test_tar_open_reads_every_member(gpu, form):
    import compu_amd

    image = T.by_name("tarfile_gnu").data
    blob = {"plain": lambda d: d, "gzip": gzipped, "zstd": zstd_frame}[form](image)
    arc = compu_amd.tar_open(upload(gpu, blob), len(blob))
    want = tarfile_contents(image)
    assert arc.summary.status == compu_amd.TarStatus.Ok and len(arc) == len(want) and arc.content.numel() == len(image)
    assert [n.rstrip(b"/") for n in arc.names] == [n.rstrip(b"/") for n, _ in want]
    for i, (name, body) in enumerate(want):
        assert arc.member(i).cpu().numpy().tobytes() == body, name
    view = arc.member(T.NAME_241)
    assert view.data_ptr() == arc.content.data_ptr() + int(arc.entries[arc.names.index(T.NAME_241)]["data_off"])  # a view, no copy
    assert arc.member("dir/grüße-世界.txt").cpu().numpy().tobytes() == b"non-ASCII name\n"
    assert arc.member(b"size/1").cpu().numpy().tobytes() == b"a repeated name: the last one wins"
    with pytest.raises(KeyError):
        arc.member(b"inner/one")  # a decoy's name
    with pytest.raises(IndexError):
        arc.member(len(want))
    if form != "plain":
        assert compu_amd.tar_open(upload(gpu, image), len(image), fmt=compu_amd.Detection.Unknown).names == arc.names


def test_tar_open_takes_a_plain_tar_whose_first_name_spells_a_zlib_header(gpu):
    """"XG", "HK", "8O" and "x^" are CMF / FLG pairs chip_detect answers with zlib; the magic at 257 says the image is a tar"""
    import compu_amd

    for first in (b"XGBoost-1.0/setup.py", b"HK/data", b"8O", b"x^caret"):
        assert compu_amd.Detection.detect(first[:4].ljust(4, b"\0")) == compu_amd.Detection.Zlib
        image = T.member(first, b"first body") + T.member(b"second", b"2") + T.END
        arc = compu_amd.tar_open(upload(gpu, image), len(image))
        assert arc.names == [first, b"second"] and arc.member(0).cpu().numpy().tobytes() == b"first body"
        assert arc.content.data_ptr() == arc.member(0).data_ptr() - 512  # the image stayed where it was
    z = zlib.compress(T.by_name("zero_blocks_2").data, 6)  # and a real zlib stream still goes through the decoder
    assert compu_amd.tar_open(upload(gpu, z), len(z)).names == [b"first", b"last"]


def test_tar_open_raises_on_a_damaged_image_behind_a_clean_gzip_stream(gpu):
    import compu_amd

    case = T.by_name("flipped_byte_in_a_middle_header")
    blob = gzipped(case.data)
    with pytest.raises(ValueError, match=r"BadHeader at stop_off 1024 "):
        compu_amd.tar_open(upload(gpu, blob), len(blob))
    with pytest.raises(ValueError, match=r"did not finish: status"):
        compu_amd.tar_open(upload(gpu, blob[:-20]), len(blob) - 20)


def test_two_host_threads_on_two_streams_and_trim(gpu, host_plans):
    """Each (device, stream) has a slot of its own: two threads with archives of different sizes, each on its own stream, get
    their own answers every time.  chip_trim() releases the slots and the next call allocates again."""
    import compu_amd

    lib = compu_amd.lib()
    names = ["many_members", "tarfile_pax"]
    cases = [T.by_name(k) for k in names]
    gpu.cuda.synchronize()
    streams = [gpu.cuda.Stream(), gpu.cuda.Stream()]
    errors = []

    def work(k):
        try:
            with gpu.cuda.stream(streams[k]):
                for _ in range(6):
                    assert_plan(gpu, lib, cases[k].data, host_plans[names[k]], stream=streams[k])
                streams[k].synchronize()
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    gpu.cuda.synchronize()
    compu_amd.trim()
    assert_plan(gpu, lib, cases[1].data, host_plans[names[1]])
    assert_plan(gpu, lib, cases[0].data, host_plans[names[0]])
