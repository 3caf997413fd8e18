"""Hand-built DEFLATE / zlib / gzip streams (tests/deflate_cases.py) on the CPU: the system zlib checks the writer, and the oracle
(oracle/oracle_inflate.c) must give every case zlib's result, call by call, in one piece and in many.  No GPU needed."""
import os
import re
import zlib

import pytest

import deflate_cases as K
import deflate_writer as W
import zstd_ref
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return K.all_cases()


def _room(c):
    return len(c.content) + 64


def _zlib_error(e):
    m = re.match(r"Error (-?\d+) while decompressing data(?:: (.*))?$", str(e))
    return int(m.group(1)), m.group(2)


def _zlib_call(z):
    """one zlib.decompressobj call, mapped as compu maps inflate()'s return (src/decoder/mod.rs:475-483): Z_OK is NeedInput when
    the input is used up and NeedOutput when it is not, Z_BUF_ERROR (no progress) NeedOutput.  An error comes with zlib's message
    in place of the output."""
    def call(chunk, room):
        try:
            out = z.decompress(chunk, room)
        except zlib.error as e:
            code, msg = _zlib_error(e)
            return None, code, msg, 0, 0
        if z.eof:
            return 2, 0, out, len(z.unused_data), room - len(out)
        rem = len(z.unconsumed_tail)
        st = 1 if (rem == len(chunk) and not out) or rem else 0
        return st, 0, out, rem, room - len(out)
    return call


def _oracle_call(d):
    def call(chunk, room):
        got, ir, orr, st, err = d.decode(chunk, room)
        if err:
            return None, err, d.msg(), 0, 0
        return st, err, got, ir, orr
    return call


def _result(calls):
    st, err = calls[-1][0], calls[-1][1]
    if st is None:
        return K.Err(err, calls[-1][2])
    out = b"".join(c[2] for c in calls)
    return out if st == 2 else K.Cut(out)


def _matches(c, got, calls):
    if isinstance(c.want, K.Cut):
        return isinstance(got, K.Cut) and c.want.content.startswith(got.content)
    if isinstance(c.want, bytes):
        return got == c.want and calls[-1][3] == c.tail
    return got == c.want


def test_zlib_decodes_every_case_to_the_writers_content(cases):
    for c in cases:
        calls = zstd_ref.drive(_zlib_call(zlib.decompressobj(K.MODES[c.fmt])), c.data, [], _room(c))
        got = _result(calls)
        assert _matches(c, got, calls), (c.name, got if not isinstance(got, bytes) else len(got))


def _runs(c):
    runs = [([], _room(c)), (c.cuts, _room(c))]
    if len(c.content) <= 20000:
        runs += [(c.cuts, 13), ([], 4096)]
    if len(c.data) <= 4096 and len(c.content) <= 65536 and "hdr_cut" not in c.tags:
        runs += [(range(1, len(c.data)), _room(c)), (range(7, len(c.data), 7), 13)]
    return runs


def test_oracle_calls_are_zlibs(cases):
    """every call of the oracle against the same call of zlib: status, error and message, output, input_remain, output_remain --
    whole, cut at the blocks, in 1- and 7-byte pieces, with output rooms from 13 bytes to the whole content"""
    for c in cases:
        for cuts, room in _runs(c):
            a = zstd_ref.drive(_zlib_call(zlib.decompressobj(K.MODES[c.fmt])), c.data, cuts, room)
            b = zstd_ref.drive(_oracle_call(O.InflateDecoder(K.MODES[c.fmt])), c.data, cuts, room)
            assert len(a) == len(b), (c.name, len(cuts), room, a[-1][:2], b[-1][:2])
            for k, (x, y) in enumerate(zip(a, b)):
                assert x == y, (c.name, len(cuts), room, k, x[:2], x[3:], y[:2], y[3:])


def test_oracle_batch_form_gives_every_case_its_result(cases):
    """orc_inflate_units (the batch form the GPU tests compare with): one call per unit with room for the content"""
    for c in cases:
        got, ir, orr, st, err = O.InflateDecoder(K.MODES[c.fmt]).decode(c.data, _room(c))
        if isinstance(c.want, bytes):
            assert (got, st, ir) == (c.want, O.FINISHED, c.tail), c.name
        elif isinstance(c.want, K.Cut):
            assert st == O.NEED_INPUT and not err and c.want.content.startswith(got), c.name
        else:
            assert err == c.want.code, (c.name, err)


def test_every_feature_is_reached_and_holds(cases):
    """each case's tags are facts: the feature's predicate over the layout records holds; and every feature is reached"""
    names = [c.name for c in cases]
    assert len(names) == len(set(names))
    reached = set()
    for c in cases:
        assert c.tags <= K.FEATURES, (c.name, c.tags - K.FEATURES)
        for t in c.tags:
            assert K.PREDICATES[t](c), (c.name, t)
        reached |= c.tags
    assert K.FEATURES - reached == set(), "features no case reaches"


def _src(path):
    with open(os.path.join(ROOT, path)) as f:
        return f.read()


def test_geometry_constants_are_the_kernels():
    """the edges the cases are placed around move with the kernel's geometry: a change there must fail here, not quietly"""
    inf, api = _src("compu_amd/csrc/inflate_unit.h"), _src("compu_amd/csrc/api.hip")

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", inf).group(1))

    def const(name, src=inf):
        return re.search(rf"constexpr (?:int|uint32_t|size_t) {name} = ([^;/]+);", src).group(1).strip()

    assert define("CHIP_S_BITS") == K.S_BITS
    assert define("CHIP_XT_BITS") == K.XT_BITS
    assert define("CHIP_XT_BITS_FIXED") == K.XT_BITS_FIXED
    assert define("CHIP_ROW_TOKENS") == K.ROW_TOKENS
    assert define("CHIP_CHUNK_BYTES") == K.CHUNK_BYTES
    assert int(const("MQ_CAP")) == K.MQ_CAP
    assert int(const("LIT_ROOT")) == K.LIT_ROOT and int(const("DIST_ROOT")) == K.DIST_ROOT
    assert "C.tok[64u * slot_r + lane]" in inf and K.GROUP == 64  # one token per lane of a 64-lane wave
    assert re.search(r"DEC_DROP_OUT = \(size_t\)1 << 20;", api) and K.DEC_DROP_OUT == 1 << 20
    assert "keep_from > 32768 ? ((keep_from - 32768)" in api and K.WINDOW == 32768


def test_writer_basics():
    """the writer's own pieces: canonical codes (RFC 1951 3.2.2's example), LSB-first packing, code-length runs"""
    assert W.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == {0: (2, 3), 1: (3, 3), 2: (4, 3), 3: (5, 3), 4: (6, 3), 5: (0, 2), 6: (14, 4), 7: (15, 4)}
    w = W.BitWriter()
    w.put(1, 1)
    w.put_code(0b110, 3)
    w.align()
    w.put(0xABC, 12)
    assert w.bytes() == bytes([0b0111, 0xBC, 0x0A]) and w.n == 20
    lens = [0] * 140 + [5] * 9 + [0, 0, 0, 7]
    assert W.expand_cl_seq(W.rle_lengths(lens)) == lens
    assert W.len_sym(258) == 285 and W.len_sym(257) == 284 and W.dist_sym(32768) == 29
