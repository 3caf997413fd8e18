"""The zstd encoder core (compu_amd/csrc/zstd_enc_core.h) built for the host with g++: the host form of the kernel's encode_unit
(zstd_enc.hip), which the CPU tests check with libzstd and the GPU tests compare the kernel's bytes against.  Also the mirrors of
the level -> group mapping and of how the streaming encoder cuts its input into segments."""
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compu_amd", "csrc")
SEGMENT = 1 << 20  # ENC_SEGMENT of chip_encode
NO_CAP = 0xFFFFFFFF

# Reads records <u32 n_segments> <u32 capacity, 0xffffffff = ample> <u32 len> * n_segments <data> from stdin and writes
# <u32 ok> <u32 canary intact> <u32 len> <frame> for each.  The segments are encoded one after the other into one frame as
# encode_unit does: hash table cleared per segment, frame header before the first, repeat offsets and the XXH64 state carried on,
# the digest behind the last.  A capacity is the room of the whole job; 64 canary bytes lie behind it.
# argv: group skip_shift wlog_single wlog_window oneshot.
_DRIVER = r'''
#include "zstd_enc_core.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }
int main(int argc, char **argv) {
    if (argc < 6) return 1;
    const uint32_t group = (uint32_t)atoi(argv[1]), skip_shift = (uint32_t)atoi(argv[2]);
    const uint32_t wlog_single = (uint32_t)atoi(argv[3]), wlog_window = (uint32_t)atoi(argv[4]);
    const bool oneshot_arg = atoi(argv[5]) != 0;
    std::vector<uint16_t> ht(zenc::HSIZE);
    std::vector<zenc::Seq> seq(zenc::MAX_SEQ);
    std::vector<uint8_t> lit(zenc::BLOCK_MAX);
    zenc::Work *w = new zenc::Work();
    zenc::Chunk k;
    zenc::Scratch sc = {ht.data(), seq.data(), lit.data(), w};
    uint32_t nseg, cap_in;
    while (rd(&nseg, 4)) {
        if (!rd(&cap_in, 4)) return 1;
        std::vector<uint32_t> lens(nseg);
        uint64_t total = 0;
        for (uint32_t i = 0; i < nseg; i++) { if (!rd(&lens[i], 4)) return 1; total += lens[i]; }
        // every segment in a buffer of exactly its size, as the kernel gets it
        std::vector<std::vector<uint8_t>> segs(nseg);
        for (uint32_t i = 0; i < nseg; i++) {
            segs[i].resize(lens[i]);
            if (lens[i] && !rd(segs[i].data(), lens[i])) return 1;
        }
        const uint32_t cap = cap_in != 0xffffffffu ? cap_in : (uint32_t)(total + total / 256 + 64 * ((uint64_t)nseg + 1));
        std::vector<uint8_t> out((size_t)cap + 64, 0xA5);
        const bool oneshot = oneshot_arg && nseg == 1;
        uint32_t rep[3] = {1, 4, 8}, pos = 0, ok = 1;
        zenc::Xxh x;
        zenc::xxh_init(x);
        for (uint32_t i = 0; i < nseg && ok; i++) {
            const uint32_t n = lens[i];
            const bool first = i == 0, last = i + 1 == nseg;
            for (auto &h : ht) h = 0;
            zenc::Out o = {out.data() + pos, 0, cap - pos, false};
            const bool single = oneshot && (uint64_t)n <= (1ull << wlog_single);
            zenc::Cfg c;
            c.group = group;
            c.skip_shift = skip_shift;
            const uint32_t window = single ? n : 1u << wlog_window;
            c.maxdist = window;
            c.block_max = window < zenc::BLOCK_MAX ? (window ? window : 1u) : zenc::BLOCK_MAX;
            if (first) zenc::frame_header(o, single, n, wlog_window);
            bool good = zenc::compress_segment(c, sc, k, segs[i].data(), n, last, rep, o);
            zenc::xxh_update(x, segs[i].data(), n);
            if (last) o.put_le((uint32_t)zenc::xxh_digest(x), 4);
            good = good && !o.ovf;
            ok = good ? 1 : 0;
            if (good) pos += o.pos;
        }
        if (!ok) pos = 0;
        uint32_t canary = 1;
        for (size_t i = cap; i < out.size(); i++) canary &= out[i] == 0xA5 ? 1u : 0u;
        fwrite(&ok, 4, 1, stdout);
        fwrite(&canary, 4, 1, stdout);
        fwrite(&pos, 4, 1, stdout);
        fwrite(out.data(), 1, pos, stdout);
    }
    delete w;
    return 0;
}
'''


def build_driver(dirpath, extra_flags=()):
    """Compiles the driver into dirpath; returns its path."""
    src = os.path.join(dirpath, "zenc_driver.cpp")
    exe = os.path.join(dirpath, "zenc_driver")
    with open(src, "w") as f:
        f.write(_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *extra_flags, "-I", CSRC, "-o", exe, src])
    return exe


def encode(exe, group, skip_shift, wlog_single, wlog_window, oneshot, jobs, caps=None):
    """jobs: a list of inputs, each bytes (one segment) or a list of segments; caps: the output capacity of each job (None:
    ample).  Returns the list of frames, None where the core reported no room.  The canary behind every capacity is asserted."""
    blob = bytearray()
    for i, j in enumerate(jobs):
        segs = [j] if isinstance(j, (bytes, bytearray)) else list(j)
        cap = NO_CAP if caps is None or caps[i] is None else caps[i]
        blob += struct.pack("<II", len(segs), cap)
        for s in segs:
            blob += struct.pack("<I", len(s))
        for s in segs:
            blob += bytes(s)
    args = [exe, str(group), str(skip_shift), str(wlog_single), str(wlog_window), str(int(bool(oneshot)))]
    out = subprocess.run(args, input=bytes(blob), stdout=subprocess.PIPE, check=True).stdout
    res, p = [], 0
    for i in range(len(jobs)):
        ok, canary, n = struct.unpack_from("<III", out, p)
        p += 12
        assert canary == 1, f"job {i}: the host core wrote past its capacity"
        res.append(out[p:p + n] if ok else None)
        p += n
    assert p == len(out)
    return res


# ---- the API's parameters ----------------------------------------------------------------------------------------------------------
def group_of(level, strategy=0):
    """(group, skip_shift) of a level and strategy: zstd_enc_group of zstd_enc.hip."""
    if level == 0:
        level = 3
    level = min(level, 22)
    skip_shift = (2 if level < -6 else 8 + level) if level < 0 else 8
    by_strategy = {1: 0, 2: 1, 3: 1, 4: 2, 5: 2, 6: 3, 7: 3, 8: 3, 9: 3}
    if strategy in by_strategy:
        return by_strategy[strategy], skip_shift
    return (0 if level < 3 else 1 if level < 6 else 2 if level < 13 else 3), skip_shift


def batch_params():
    """(wlog_single, wlog_window, oneshot) of chip_encode_batch."""
    return 27, 27, True


def stream_params(window_log):
    """(wlog_single, wlog_window, oneshot) of the streaming encoder (enc_segment of api.hip); the driver applies `oneshot` only
    to a job of one segment, the first that is also the last."""
    return min(window_log, 27), min(window_log, 20), True


def encode_level(exe, level, strategy, jobs, params=None, caps=None):
    g, ss = group_of(level, strategy)
    ws, ww, one = params or batch_params()
    return encode(exe, g, ss, ws, ww, one, jobs, caps)


PROCESS, FLUSH, FINISH = "process", "flush", "finish"


def segments_of(script):
    """The segments chip_encode cuts a stream into when the caller's room is ample.  script: (piece, op) calls, the last a FINISH.
    Buffered input becomes a non-final segment whenever it reaches 1 MiB and more input of the same call follows or the call is a
    Process; a Flush or Finish makes one segment of what is buffered if that is non-empty, or the call is a Finish, or nothing has
    been written yet."""
    segs, buf, started = [], bytearray(), False
    for piece, op in script:
        taken = 0
        while taken < len(piece):
            k = min(len(piece) - taken, SEGMENT - len(buf))
            buf += piece[taken:taken + k]
            taken += k
            if len(buf) >= SEGMENT and taken < len(piece):
                segs.append(bytes(buf))
                buf, started = bytearray(), True
        if len(buf) >= SEGMENT and op == PROCESS:
            segs.append(bytes(buf))
            buf, started = bytearray(), True
        if op in (FLUSH, FINISH) and (buf or op == FINISH or not started):
            segs.append(bytes(buf))
            buf, started = bytearray(), True
    assert script and script[-1][1] == FINISH
    return segs
