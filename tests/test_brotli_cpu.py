"""Brotli data without a GPU: the static dictionary, the RFC 7932 tables of compu_amd/csrc/brotli_tables.h against the system's
libbrotlicommon, the error strings against libbrotlidec, and the format tag in every mirror."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

import brotli_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compu_amd", "csrc")
DICT_SHA256 = "20e42eb1b511c21806d4d227d07e5dd06877d8ce7b3a817f378f313653f35c70"


class _Dict(C.Structure):
    _fields_ = [("size_bits_by_length", C.c_uint8 * 32), ("offsets_by_length", C.c_uint32 * 32), ("data_size", C.c_size_t),
                ("data", C.POINTER(C.c_uint8))]


class _Transforms(C.Structure):
    _fields_ = [("prefix_suffix_size", C.c_uint16), ("prefix_suffix", C.POINTER(C.c_uint8)), ("prefix_suffix_map", C.POINTER(C.c_uint16)),
                ("num_transforms", C.c_uint32), ("transforms", C.POINTER(C.c_uint8)), ("params", C.POINTER(C.c_uint8)),
                ("cutOffTransforms", C.c_int16 * 10)]


def _common():
    c = C.CDLL("libbrotlicommon.so.1")
    c.BrotliGetDictionary.restype = C.POINTER(_Dict)
    c.BrotliGetTransforms.restype = C.POINTER(_Transforms)
    c.BrotliTransformDictionaryWord.restype = C.c_int
    c.BrotliTransformDictionaryWord.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(_Transforms), C.c_int]
    return c


def test_dictionary_file():
    with open(os.path.join(CSRC, "brotli_dict.bin"), "rb") as f:
        data = f.read()
    assert len(data) == 122784
    assert hashlib.sha256(data).hexdigest() == DICT_SHA256
    d = _common().BrotliGetDictionary().contents
    assert C.string_at(d.data, d.data_size) == data


# The test program prints the header's tables and applies every transform the way brotli.hip does (prefix, word with its
# omissions and RFC 7932 uppercasing, suffix)
_PROG = r'''
#include "brotli_tables.h"
#include <cstdio>
#include <cstring>
using namespace brotli_tab;
static int upper(unsigned char *p) {
    if (p[0] < 0xc0) { if (p[0] >= 'a' && p[0] <= 'z') p[0] ^= 32; return 1; }
    if (p[0] < 0xe0) { p[1] ^= 32; return 2; }
    p[2] ^= 5; return 3;
}
int main(int argc, char **argv) {
    for (int i = 0; i < 2048; i++) printf("%d ", CONTEXT_LUT.v[i]);
    printf("\n");
    for (int i = 0; i < 26; i++) printf("%d %d ", BLOCK_LEN_BASE[i], BLOCK_LEN_EXTRA[i]);
    printf("\n");
    for (int i = 4; i <= 24; i++) printf("%d %u ", DICT_NDBITS[i], DICT_OFFSET[i]);
    printf("\n");
    for (int a = 1; a < argc; a++) {
        const unsigned char *w = (const unsigned char *)argv[a];
        int len = (int)strlen(argv[a]);
        for (int t = 0; t < NUM_TRANSFORMS; t++) {
            unsigned char buf[64] = {0};
            const Transform &T = TRANSFORMS[t];
            int n = 0, skip = 0, wl = len;
            memcpy(buf, T.prefix, T.prefix_len); n = T.prefix_len;
            if (T.type >= 1 && T.type <= 9) wl = len > T.type ? len - T.type : 0;
            if (T.type >= 12 && T.type <= 20) { skip = T.type - 11; wl = len > skip ? len - skip : 0; }
            memcpy(buf + n, w + skip, wl);
            if (wl && T.type == 10) upper(buf + n);
            if (wl && T.type == 11) { unsigned char *p = buf + n; int left = wl; while (left > 0) { int s = upper(p); p += s; left -= s; } }
            n += wl;
            memcpy(buf + n, T.suffix, T.suffix_len); n += T.suffix_len;
            printf("=");  // an empty result still makes a field
            for (int k = 0; k < n; k++) printf("%02x", buf[k]);
            printf(" ");
        }
        printf("\n");
    }
}
'''

_WORDS = [b"time", b"people", b"Hello", b"\xc3\xa9t\xc3\xa9s", b"\xe4\xb8\xad\xe6\x96\x87\xe5\xad\x97", b"abcdefghijklmnopqrstuvwx",
          b"tree", b"x\xd0\xb4\xd0\xb0y"]


@pytest.fixture(scope="module")
def header_dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("brotli_tables")
    src = d / "t.cpp"
    src.write_text(_PROG)
    exe = d / "t"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    out = subprocess.check_output([os.fsencode(exe)] + _WORDS)
    return out.decode().split("\n")


def test_context_lut_matches_libbrotlicommon(header_dump):
    lib = (C.c_uint8 * 2048).in_dll(_common(), "_kBrotliContextLookupTable")
    assert [int(x) for x in header_dump[0].split()] == list(lib)


def test_block_length_ranges_match_libbrotlicommon(header_dump):
    class R(C.Structure):
        _fields_ = [("offset", C.c_uint16), ("nbits", C.c_uint8)]

    r = (R * 26).in_dll(_common(), "_kBrotliPrefixCodeRanges")
    want = []
    for x in r:
        want += [x.offset, x.nbits]
    assert [int(x) for x in header_dump[1].split()] == want


def test_dictionary_layout_matches_libbrotlicommon(header_dump):
    d = _common().BrotliGetDictionary().contents
    want = []
    for n in range(4, 25):
        want += [d.size_bits_by_length[n], d.offsets_by_length[n]]
    assert [int(x) for x in header_dump[2].split()] == want


def test_all_121_transforms_match_libbrotlicommon(header_dump):
    c = _common()
    tr = c.BrotliGetTransforms()
    assert tr.contents.num_transforms == 121
    for w, line in zip(_WORDS, header_dump[3:]):
        got = line.split()
        assert len(got) == 121
        for t in range(121):
            dst = C.create_string_buffer(64)
            n = c.BrotliTransformDictionaryWord(dst, w, len(w), tr, t)
            assert bytes.fromhex(got[t][1:]) == dst.raw[:n], (w, t)


def test_strerror_matches_libbrotlidec():
    import compu_amd

    lib = compu_amd.lib()
    for code in range(-31, 4):
        assert lib.chip_decoder_strerror(compu_amd.FMT_BROTLI, code).decode() == B.error_string(code), code


def test_format_tag_in_every_mirror():
    import compu_amd

    assert compu_amd.FMT_BROTLI == 101
    with open(os.path.join(ROOT, "include", "compu_hip.h")) as f:
        assert "CHIP_FMT_BROTLI = 101" in f.read()
    with open(os.path.join(ROOT, "compu_amd", "host", "compu.hpp")) as f:
        s = f.read()
        assert "brotli_hip" in s and "CHIP_FMT_BROTLI" in s
    with open(os.path.join(ROOT, "integration", "src", "hip_sys.rs")) as f:
        assert "pub const CHIP_FMT_BROTLI: c_int = 101;" in f.read()
    with open(os.path.join(ROOT, "integration", "src", "decoder", "hip.rs")) as f:
        s = f.read()
        assert "pub fn brotli_hip()" in s and "describe_brotli_error_fn" in s and "BatchFormat::Brotli" in s
    assert hasattr(compu_amd.decoder_interface, "brotli_hip")
