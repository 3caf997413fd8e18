"""The brotli encoder core (compu_amd/csrc/brotli_enc_core.h) built for the host with g++, and a reader of a stream's first
metablock header: what the CPU tests check the encoder's streams with, and what the GPU tests compare the kernel's bytes against."""
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compu_amd", "csrc")

# Reads records <u32 n_segments> <u32 len> * n_segments <data> from stdin and writes <u32 status> <u32 len> <stream> for each:
# the segments are encoded one after the other into one stream (first: WBITS, last: closed), as the streaming encoder does
# between flushes.  argv: quality lgwin.
_DRIVER = r'''
#include "brotli_enc_core.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    const uint32_t q = (uint32_t)atoi(argv[1]), lgwin = (uint32_t)atoi(argv[2]);
    std::vector<uint16_t> ht(zenc::HSIZE);
    std::vector<benc::Cmd> cmd(benc::MAX_CMD);
    std::vector<uint8_t> lit(benc::MB_MAX);
    benc::Work *w = new benc::Work();
    benc::Chunk k;
    const benc::Cfg c = benc::make_cfg(benc::quality_group(q), lgwin);
    benc::Scratch sc = {ht.data(), cmd.data(), lit.data(), w};
    uint32_t nseg;
    while (rd(&nseg, 4)) {
        std::vector<uint32_t> lens(nseg);
        uint64_t total = 0;
        for (uint32_t i = 0; i < nseg; i++) { if (!rd(&lens[i], 4)) return 1; total += lens[i]; }
        std::vector<uint8_t> in(total + 16), out(total + 4 * (total / 65536 + 2) * (nseg + 1) + 64);
        if (total && !rd(in.data(), total)) return 1;
        uint32_t ring[4] = {4, 11, 15, 16}, pos = 0, ok = 1;
        uint64_t at = 0;
        for (uint32_t i = 0; i < nseg && ok; i++) {
            for (auto &h : ht) h = 0;
            benc::Out o = {out.data() + pos, 0, (uint32_t)(out.size() - pos), false};
            ok = benc::compress_segment(c, sc, k, in.data() + at, lens[i], i == 0, i + 1 == nseg, lgwin, ring, o);
            pos += o.pos;
            at += lens[i];
        }
        fwrite(&ok, 4, 1, stdout);
        fwrite(&pos, 4, 1, stdout);
        fwrite(out.data(), 1, pos, stdout);
    }
    delete w;
    return 0;
}
'''


def build_driver(dirpath):
    """Compiles the driver into dirpath; returns its path."""
    src = os.path.join(dirpath, "benc_driver.cpp")
    exe = os.path.join(dirpath, "benc_driver")
    with open(src, "w") as f:
        f.write(_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, src])
    return exe


def encode(exe, quality, lgwin, jobs):
    """jobs: a list of inputs, each bytes (one segment) or a list of segments.  Returns the list of streams (None where the core
    reported no room, which its generous buffer never does)."""
    blob = bytearray()
    for j in jobs:
        segs = [j] if isinstance(j, (bytes, bytearray)) else list(j)
        blob += struct.pack("<I", len(segs))
        for s in segs:
            blob += struct.pack("<I", len(s))
        for s in segs:
            blob += bytes(s)
    out = subprocess.run([exe, str(quality), str(lgwin)], input=bytes(blob), stdout=subprocess.PIPE, check=True).stdout
    res, p = [], 0
    for _ in jobs:
        ok, n = struct.unpack_from("<II", out, p)
        p += 8
        res.append(out[p:p + n] if ok else None)
        p += n
    assert p == len(out)
    return res


# ---- a reader of the first metablock header (RFC 7932 9.2, 3.4, 3.5) --------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.d = bytes(data) + b"\0" * 8
        self.p = 0

    def get(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v

    def peek(self, n):
        p = self.p
        v = self.get(n)
        self.p = p
        return v


def _canonical(lens):
    """{(length, code read MSB first): symbol} of a canonical prefix code."""
    table, code = {}, 0
    for ln in range(1, 16):
        for s, x in enumerate(lens):
            if x == ln:
                table[(ln, code)] = s
                code += 1
        code <<= 1
    return table


def _read_symbol(r, table, lens):
    if sum(1 for x in lens if x) == 1:
        return next(s for s, x in enumerate(lens) if x)
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | r.get(1)
        if (ln, code) in table:
            return table[(ln, code)]
    raise ValueError("bad prefix code")


_ORDER = [1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15]
_CLL_LEN = [2, 2, 2, 3, 2, 2, 2, 4, 2, 2, 2, 3, 2, 2, 2, 4]
_CLL_VAL = [0, 4, 3, 2, 0, 4, 3, 1, 0, 4, 3, 2, 0, 4, 3, 5]


def _read_code(r, alphabet, abits):
    """('simple' | 'complex', code lengths of the alphabet)."""
    hskip = r.get(2)
    lens = [0] * alphabet
    if hskip == 1:
        nsym = r.get(2) + 1
        syms = [r.get(abits) for _ in range(nsym)]
        shape = {1: [0], 2: [1, 1], 3: [1, 2, 2]}.get(nsym)
        if nsym == 4:
            shape = [1, 2, 3, 3] if r.get(1) else [2, 2, 2, 2]
        for s, ln in zip(syms, shape):
            lens[s] = ln
        if nsym == 1:
            lens[syms[0]] = 1  # (read with 0 bits; marks the symbol as used)
        return "simple", lens
    cl, space, num = [0] * 18, 32, 0
    for i in range(hskip, 18):
        v = r.peek(4)
        r.get(_CLL_LEN[v])
        cl[_ORDER[i]] = _CLL_VAL[v]
        if _CLL_VAL[v]:
            space -= 32 >> _CLL_VAL[v]
            num += 1
            if space <= 0:
                break
    table = _canonical(cl)
    sym, prev, repeat, rlen, space = 0, 8, 0, 0, 32768
    while sym < alphabet and space > 0:
        s = _read_symbol(r, table, cl)
        if s < 16:
            repeat = 0
            lens[sym] = s
            if s:
                prev = s
                space -= 32768 >> s
            sym += 1
            continue
        bits, new = (2, prev) if s == 16 else (3, 0)
        if rlen != new:
            repeat, rlen = 0, new
        old = repeat
        if repeat > 0:
            repeat = (repeat - 2) << bits
        repeat += r.get(bits) + 3
        for _ in range(repeat - old):
            lens[sym] = new
            sym += 1
            if new:
                space -= 32768 >> new
    assert space == 0, "incomplete code"
    return "complex", lens


def first_metablock(data, wbits=True):
    """The stream's WBITS and first metablock header: a dict with 'wbits' and either 'empty', 'uncompressed' (with 'mlen') or
    the three prefix codes as (form, lengths): 'lit', 'ic', 'dist'.  wbits=False: `data` starts at a metablock boundary inside
    a stream (behind a flushed segment)."""
    r = _Bits(data)
    if not wbits:
        wbits = None
    elif r.get(1) == 0:
        wbits = 16
    else:
        n = r.get(3)
        if n:
            wbits = 17 + n
        else:
            m = r.get(3)
            wbits = 8 + m if m else 17
    d = {"wbits": wbits}
    islast = r.get(1)
    if islast and r.get(1):
        d["empty"] = True
        return d
    mnib = r.get(2)
    assert mnib != 3, "metadata first"
    d["mlen"] = r.get(4 * (mnib + 4)) + 1
    if not islast and r.get(1):
        d["uncompressed"] = True
        return d
    assert r.get(3) == 0, "one block type per category"
    d["npostfix"], d["ndirect"] = r.get(2), r.get(4)
    d["cmode"] = r.get(2)
    assert r.get(2) == 0, "one literal and one distance tree"
    d["lit"] = _read_code(r, 256, 8)
    d["ic"] = _read_code(r, 704, 10)
    d["dist"] = _read_code(r, 64, 6)
    return d
