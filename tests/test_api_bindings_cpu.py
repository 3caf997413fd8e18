"""The Python binding layer (compu_amd/api.py, compu_amd/_ffi.py), without a GPU.

Same surface: tests/golden/api_surface.json was recorded from the commit before the summaries, plans, archive writers and slab
streams were stated once -- the public names (imported modules are not counted), every public function's signature, every
summary's values, as_tuple() and repr() over a raw structure with field i set to i + 1 (a status an enum refuses: the next
lower value it takes), and the record dtypes.  The file is data: the code here must go on answering it.

Bindings against the header: the prototype table of _ffi.py has the functions of include/compu_hip.h, their parameter counts
and the class of their return types.

The slab-stream loop: _slab_stream driven by scripted steps over bytearrays, through each policy of the two formats."""
import ctypes
import inspect
import io
import json
import os
import re
import types

import pytest
from test_abi import _c_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "api_surface.json")) as f:
    SURFACE = json.load(f)


def _public(mod):
    return sorted(n for n in dir(mod) if not n.startswith("_") and not inspect.ismodule(getattr(mod, n)))


# ---- same surface --------------------------------------------------------------------------------


def test_public_names_are_the_recorded_ones():
    import compu_amd
    from compu_amd import api

    assert _public(compu_amd) == SURFACE["package_names"]
    assert _public(api) == SURFACE["api_names"]
    assert len(SURFACE["private_names"]) == 35  # every _*Summary, _*Opts, _*Entry, _*Source, _*Block, _*Cursor, _Xxh64State, _ranges_to_device
    for name in SURFACE["private_names"]:
        assert hasattr(api, name), name
    for name in SURFACE["private_names"]:
        if name != "_ranges_to_device":
            assert issubclass(getattr(api, name), ctypes.Structure), name


def test_signatures_are_the_recorded_ones():
    from compu_amd import api

    assert len(SURFACE["signatures"]) == 88
    for name, sig in SURFACE["signatures"].items():
        assert str(inspect.signature(getattr(api, name))) == sig, name
    assert sorted(SURFACE["signatures"]) == sorted(n for n in _public(api) if inspect.isfunction(getattr(api, n)))


@pytest.mark.parametrize("name", sorted(SURFACE["summaries"]))
def test_summary_is_the_recorded_one(name):
    from compu_amd import api

    rec = SURFACE["summaries"][name]
    cls, raw_cls = getattr(api, name), getattr(api, "_" + name)
    assert len(raw_cls._fields_) == len(rec["raw"])
    for i, (f, _) in enumerate(raw_cls._fields_):
        assert rec["raw"][f] == i + 1 or (f == "status" and 0 < rec["raw"][f] <= i), f
    summ = cls(raw_cls(**rec["raw"]))
    if rec["kind"] == "slots":
        assert list(cls.__slots__) == rec["names"] and not hasattr(summ, "__dict__")
    else:  # the two *NextSummary classes: FIELDS, and values that can be assigned
        assert list(cls.FIELDS) == rec["names"] and not getattr(cls, "__slots__", ())
        summ.in_used += 5
        assert summ.in_used == rec["attrs"]["in_used"] + 5
        summ.in_used -= 5
    for field in rec["names"]:
        v = getattr(summ, field)
        assert type(v).__name__ == rec["types"][field] and int(v) == rec["attrs"][field], field
    if rec["as_tuple"] is None:
        assert not hasattr(summ, "as_tuple")
    else:
        assert summ.as_tuple() == tuple(rec["as_tuple"]) and all(type(v) is int for v in summ.as_tuple())
    assert repr(summ) == rec["repr"]
    assert cls.__doc__ and cls.__doc__.startswith("chip_")  # the documentation of the fields stays


def test_there_are_21_summaries_and_rounds_stays_out_of_one_tuple():
    from compu_amd import api

    assert len(SURFACE["summaries"]) == 21
    assert "rounds" in api.ZstdParallelSummary.__slots__ and len(api.ZstdParallelSummary(api._ZstdParallelSummary()).as_tuple()) == 8
    assert "rounds" in api.ZstdParallelSummary.as_tuple.__doc__


def test_record_dtypes_are_the_recorded_ones():
    from compu_amd import api

    sizes = {"zstd_block_dtype": 48, "zip_entry_dtype": 56, "zip_source_dtype": 32, "tar_entry_dtype": 72, "tar_source_dtype": 64, "lz4_block_dtype": 24}
    assert sorted(SURFACE["dtypes"]) == sorted(sizes)
    for name, rec in SURFACE["dtypes"].items():
        dt = getattr(api, name)()
        assert json.loads(json.dumps(dt.descr)) == rec["descr"], name
        assert dt.itemsize == rec["itemsize"] == sizes[name], name


# ---- bindings against the header -------------------------------------------------------------------


def _c_return_types():
    """{name: return type as written} of every function prototype in include/compu_hip.h (a sibling of test_abi._c_prototypes)."""
    text = open(os.path.join(ROOT, "include", "compu_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    rets = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \t\*]*?)\b(chip_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if m.group(2) not in ("chip_malloc_fn", "chip_free_fn"):
            rets[m.group(2)] = " ".join(m.group(1).replace("*", " * ").split())
    return rets


def _restype_class(restype):
    if restype is None:
        return "void"
    if restype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(restype, ctypes._Pointer):
        return "pointer"
    if issubclass(restype, ctypes.Structure):
        return "struct " + restype.__name__
    if restype is ctypes.c_int:
        return "int"
    if restype in (ctypes.c_size_t, ctypes.c_uint64) and ctypes.sizeof(restype) == 8:
        return "u64"
    return repr(restype)


def _header_class(ret):
    if ret.endswith("*"):
        return "pointer"
    return {"void": "void", "int": "int", "size_t": "u64", "uint64_t": "u64", "chip_decode_result": "struct _DecodeResult",
            "chip_encode_result": "struct _EncodeResult"}[ret]


def test_prototype_table_matches_the_header():
    from compu_amd import _ffi

    protos, rets = _c_prototypes(), _c_return_types()
    assert sorted(protos) == sorted(rets) and len(protos) >= 90
    rows = {name: (restype, argtypes) for name, restype, argtypes in _ffi._PROTOTYPES}
    assert len(rows) == len(_ffi._PROTOTYPES), "a function has two rows"
    assert sorted(rows) == sorted(protos)
    for name, (restype, argtypes) in rows.items():
        assert len(argtypes) == protos[name], f"{name}: {protos[name]} parameters in the header, {len(argtypes)} in the table"
        assert _restype_class(restype) == _header_class(rets[name]), f"{name}: returns {rets[name]} in the header"


def test_lib_applies_every_row():
    """lib() loads on a machine without a GPU; every function carries its row."""
    from compu_amd import _ffi, api

    L = api.lib()
    assert L is _ffi.lib()
    for name, restype, argtypes in _ffi._PROTOTYPES:
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert L.chip_version().startswith(b"compu-hip")


# ---- the count-then-fill protocol --------------------------------------------------------------------


def test_count_then_fill_protocol():
    from compu_amd import api

    calls = []

    def run(max_units, have=3, rc=0):
        calls.clear()

        def call(m, a, b):
            calls.append((m, a, b))
            return rc

        return api._count_then_fill("chip_x", call, lambda: have, lambda m: (list(range(m)), ["r"] * m), lambda a: ("ptr", len(a)), max_units)

    assert run(None) == [[0, 1, 2], ["r"] * 3] and calls == [(0, None, None), (3, ("ptr", 3), ("ptr", 3))]  # count, then fill
    assert run(2) == [[0, 1], ["r"] * 2] and calls == [(2, ("ptr", 2), ("ptr", 2))]  # a number: the one call
    assert run(5) == [[0, 1, 2], ["r"] * 3] and len(calls) == 1  # cut to min(m, count)
    assert run(0) == [[], []] and calls == [(0, None, None)]  # no room: null pointers
    with pytest.raises(RuntimeError, match="^chip_x failed: -7$"):
        run(None, rc=-7)


def test_host_input_of_nothing_is_a_null_pointer():
    import numpy as np

    from compu_amd import api

    for empty in (b"", np.zeros(0, np.uint8)):
        buf, base = api._host_input(empty)
        assert buf.size == 0 and base is None
    buf, base = api._host_input(np.arange(10, dtype=np.uint8)[::2])
    assert buf.flags.c_contiguous and buf.tolist() == [0, 2, 4, 6, 8] and base.value == buf.ctypes.data
    assert api.zip_plan_host(b"")[0].size == 0 and api.tar_plan_host(b"", 4)[0].size == 0


# ---- the slab-stream loop, with scripted steps ---------------------------------------------------------
#
# The toy format both scripted formats decode: a unit is a length byte L and L bytes of content, a unit of length 0 ends the
# stream.  In front of it stands what the continuation rule of the format looks at: a zstd frame header of 6 bytes (the magic,
# the descriptor 0x20 and the content size in one byte), or the gzip magic 1f 8b.  A step takes whole units only.

NEED_INPUT, NEED_OUTPUT, FINISHED = 0, 1, 2
ZSTD_MAGIC, SKIPPABLE = bytes.fromhex("28b52ffd"), bytes.fromhex("502a4d18")


def units(*contents):
    return b"".join(bytes([len(c)]) + c for c in contents) + b"\0"


def zstd_frame(*contents):
    return ZSTD_MAGIC + bytes([0x20, sum(len(c) for c in contents)]) + units(*contents)


def gzip_member(*contents):
    return b"\x1f\x8b" + units(*contents)


class Scripted:
    """The device side of a _Slabs over bytearrays, and the toy decoder as its step; what it was asked is kept."""

    head = 0  # bytes in front of the units
    room_alloc = 1 << 16  # (a room at its clamp is asked for, not allocated)

    def __init__(self, **attrs):
        self.seen, self.rooms = [], []
        self.__dict__.update(attrs)

    def new_cursor(self, fmt=None):
        return types.SimpleNamespace(phase=0, wrap=2, content_size=0, out_total=0)

    def upload(self, pending, n, slab):
        return bytes(pending[:n])

    def room(self, k):
        self.rooms.append(k)
        return bytearray(min(k, self.room_alloc))

    def download(self, out, k):
        return bytes(out[:k])

    def step(self, cur, data, out):
        self.seen.append(len(data))
        p = o = 0
        answer = lambda status, need=0: types.SimpleNamespace(in_used=p, out_len=o, need_out=need, status=status)  # noqa: E731
        if not cur.phase:
            if len(data) < self.head:
                return answer(NEED_INPUT)
            p, cur.phase, cur.content_size = self.head, 1, data[5] if self.head == 6 else 0
        while True:
            if p == len(data):
                return answer(NEED_INPUT)
            size = data[p]
            if size == 0xFF:
                return answer(-20)  # a unit this decoder refuses
            if size == 0:
                p += 1
                return answer(FINISHED)
            if p + 1 + size > len(data):
                return answer(NEED_INPUT)
            if o + size > len(out):
                return answer(NEED_OUTPUT, self.need_out if hasattr(self, "need_out") else size)
            out[o:o + size] = data[p + 1:p + 1 + size]
            p, o, cur.out_total = p + 1 + size, o + size, cur.out_total + size


def scripted_zstd(frames=False, **attrs):
    from compu_amd import api

    cls = type("ScriptedZstd", (Scripted, api._ZstdSlabs), {"head": 6})
    return cls(frames=frames, **attrs)


def scripted_inflate(members=False, **attrs):
    from compu_amd import api

    cls = type("ScriptedInflate", (Scripted, api._InflateSlabs), {"head": 2})
    return cls(members=members, **attrs)


class Drip(io.BytesIO):
    """a file object whose reads are short: one byte at a time"""

    def read(self, n=-1):
        return super().read(min(n, 1))


def test_the_limits_of_the_two_formats():
    from compu_amd import api

    assert (api._ZstdSlabs.slab_max, api._ZstdSlabs.room_max) == (1 << 31, (1 << 31) - 1)
    assert (api._InflateSlabs.slab_max, api._InflateSlabs.room_max) == (api.GZPLAN_WINDOW, 0xFFFFFFF0) and api._InflateSlabs.spare == 4
    assert api._ZstdSlabs.spare == 0


def test_slab_doubles_once_until_a_unit_is_whole():
    from compu_amd import api

    source = units(b"sevenby", b"x")  # 8 + 2 + 1 = 11 bytes
    assert len(source) == 11
    fmt = scripted_inflate(head=0)
    assert api._slab_stream(fmt, source, None, 4, 100) == b"sevenbyx"
    assert fmt.seen == [4, 8, 3]  # nothing used of 4 bytes; the slab of 8 holds the first unit; the rest
    assert fmt.rooms == [100, 100, 100]


@pytest.mark.parametrize("make, rooms", [(scripted_zstd, [3, 3, 4]), (scripted_inflate, [3, 3, 6])])
def test_room_grows_by_the_policy_of_the_format(make, rooms):
    """NeedOutput with need_out 4 above the room of 3: zstd goes to max(room, need_out), inflate to max(2 * room, need_out)"""
    from compu_amd import api

    fmt = make()
    source = (zstd_frame if make is scripted_zstd else gzip_member)(b"four")
    assert api._slab_stream(fmt, source, None, 64, 3) == b"four"
    assert fmt.rooms == rooms  # the call that takes the header, the call that stalls, the call with the grown room


def test_inflate_room_takes_need_out_when_it_is_above_the_double():
    from compu_amd import api

    fmt = scripted_inflate()
    assert api._slab_stream(fmt, gzip_member(b"0123456789"), None, 64, 3) == b"0123456789"
    assert fmt.rooms == [3, 3, 10]


def test_zstd_room_of_a_frame_comes_from_its_header_and_what_is_left():
    from compu_amd import api

    fmt = scripted_zstd()
    assert api._slab_stream(fmt, zstd_frame(b"abc", b"de"), None, 10, 100) == b"abcde"
    assert fmt.seen == [10, 4] and fmt.rooms == [5, 2]  # content_size 5 of the header; 5 - 3 inside the frame


def test_room_at_its_clamp_is_an_error():
    from compu_amd import api
    from compu_amd.api import DecodeError

    with pytest.raises(DecodeError) as e:  # zstd: a block that needs more than a call can be given
        api._slab_stream(scripted_zstd(need_out=1 << 31), zstd_frame(b"four"), None, 64, 3)
    assert e.value.code == -5
    fmt = scripted_inflate(room_alloc=0)
    with pytest.raises(DecodeError) as e:  # inflate: the room already stands at its clamp
        api._slab_stream(fmt, gzip_member(b"four"), None, 64, 1 << 40)
    assert e.value.code == -5 and fmt.rooms == [0xFFFFFFF0] * 2


@pytest.mark.parametrize("make, frame, text", [(scripted_zstd, zstd_frame, "the source ends inside the frame"),
                                               (scripted_inflate, gzip_member, "the source ends inside the stream")])
def test_source_that_ends_inside_a_unit(make, frame, text):
    from compu_amd import api

    whole = frame(b"abc", b"defgh")
    for cut in (1, len(whole) - 1, len(whole) - 3):
        with pytest.raises(EOFError, match=f"^{text}$"):
            api._slab_stream(make(), whole[:cut], None, 4, 100)
        with pytest.raises(EOFError, match=f"^{text}$"):
            api._slab_stream(make(), Drip(whole[:cut]), None, 4, 100)


def test_error_status_raises_decode_error_with_its_code():
    from compu_amd import api
    from compu_amd.api import DecodeError

    sink = io.BytesIO()
    with pytest.raises(DecodeError) as e:
        api._slab_stream(scripted_inflate(), b"\x1f\x8b\x02ok\xffrest", sink, 64, 100)
    assert e.value.code == -20 and sink.getvalue() == b"ok"  # what the call delivered in front of the error is written


def test_slab_at_its_clamp_that_still_stalls():
    from compu_amd import api
    from compu_amd.api import DecodeError

    for make in (scripted_zstd, scripted_inflate):
        fmt = make(slab_max=8, head=0)
        with pytest.raises(DecodeError) as e:
            api._slab_stream(fmt, units(b"a unit of 20 bytes.."), None, 3, 100)
        assert e.value.code == -5 and fmt.seen == [3, 6, 8]  # doubled, clamped, and no further


@pytest.mark.parametrize("make, frame", [(scripted_zstd, zstd_frame), (scripted_inflate, gzip_member)])
def test_short_reads_and_sinks(make, frame):
    from compu_amd import api

    contents = [bytes([65 + i]) * (i % 7 + 1) for i in range(30)]
    source, want = frame(*contents), b"".join(contents)
    assert api._slab_stream(make(), source, None, 5, 3) == want  # (5-byte slabs, 3-byte rooms)
    assert api._slab_stream(make(), bytearray(source), None, 64, 100) == want
    assert api._slab_stream(make(), io.BytesIO(source), None, 5, 3) == want
    assert api._slab_stream(make(), Drip(source), None, 5, 3) == want
    sink = io.BytesIO()
    assert api._slab_stream(make(), Drip(source), sink, 5, 3) == len(want) and sink.getvalue() == want
    assert api._slab_stream(make(), frame(), io.BytesIO(), 5, 3) == 0


def test_zstd_frames_continue_over_skippable_frames():
    from compu_amd import api

    skip = SKIPPABLE + (3).to_bytes(4, "little") + b"???"
    source = zstd_frame(b"one") + skip + skip + zstd_frame(b"two", b"2") + skip + b"trailing bytes that are no frame"
    assert api._slab_stream(scripted_zstd(frames=True), source, None, 7, 100) == b"onetwo2"
    assert api._slab_stream(scripted_zstd(frames=True), Drip(source), None, 7, 100) == b"onetwo2"
    assert api._slab_stream(scripted_zstd(frames=False), source, None, 7, 100) == b"one"
    for cut in (len(zstd_frame(b"one")) + 5, len(zstd_frame(b"one")) + 9):  # inside the 8 bytes; inside what they announce
        with pytest.raises(EOFError, match="^the source ends inside a skippable frame$"):
            api._slab_stream(scripted_zstd(frames=True), source[:cut], None, 7, 100)
    assert api._slab_stream(scripted_zstd(frames=True), zstd_frame(b"one") + b"\x28\xb5", None, 7, 100) == b"one"  # (no whole magic: the end)


def test_gzip_members_continue_on_1f_8b_one_byte_per_read():
    from compu_amd import api

    source = gzip_member(b"one") + gzip_member(b"two", b"2") + b"\x1f\x00no member"
    assert api._slab_stream(scripted_inflate(members=True), Drip(source), None, 7, 100) == b"onetwo2"
    assert api._slab_stream(scripted_inflate(members=True), source, None, 7, 100) == b"onetwo2"
    assert api._slab_stream(scripted_inflate(members=False), source, None, 7, 100) == b"one"
    assert api._slab_stream(scripted_inflate(members=True), gzip_member(b"one") + b"\x1f", None, 7, 100) == b"one"
    # behind a stream that is no gzip member (the cursor's wrap says so) nothing is begun
    fmt = scripted_inflate(members=True)
    fmt.new_cursor = lambda fmt=None: types.SimpleNamespace(phase=0, wrap=1, content_size=0, out_total=0)
    assert api._slab_stream(fmt, source, None, 7, 100) == b"one"
