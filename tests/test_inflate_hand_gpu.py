"""Inflate on the GPU against hand-built DEFLATE / zlib / gzip streams (tests/deflate_cases.py): every case in one batch launch at
several capacities, with and without CHIP_F_COMPU_STATUS, and through the streaming decoder call by call -- whole, cut at its
blocks, in small pieces, with small output rooms -- against the oracle, which tests/test_deflate_writer_cpu.py pins to the system
zlib.  The wrapped cases also go through one CHIP_FMT_DETECT batch together with the zstd hand frames."""
import pytest

import deflate_cases as K
import zstd_ref
from oracle import oracle as O
from test_inflate_gpu import oracle_batch, run_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return K.all_cases()


def _ref_len(c):
    """output the oracle produces with room for everything (for an error: the bytes in front of it)"""
    return len(O.InflateDecoder(K.MODES[c.fmt]).decode(c.data, len(c.content) + 64)[0])


def _caps(c):
    n = _ref_len(c)
    caps = {n, n + 4096} | ({n - 1} if n else set())
    for r in c.layout:  # room that ends inside a match or a stored block, or exactly at a chunk's end
        if r.kind == "match" and r.length >= 4 and r.out + r.length <= n:
            caps.add(r.out + r.length // 2)
            break
    for r in c.layout:
        if r.kind == "stored" and r.nbits >= 16 and r.out + r.nbits // 8 <= n:
            caps.add(r.out + r.nbits // 16)
            break
    if n > K.CHUNK_BYTES:
        caps |= {K.CHUNK_BYTES, 2 * K.CHUNK_BYTES}
    return sorted(caps)


def _batch(gpu, cases, flags):
    import compu_amd

    by_fmt = {}
    for c in cases:
        for cap in _caps(c):
            by_fmt.setdefault(K.MODES[c.fmt], []).append((c, cap))
    for fmt, units in by_fmt.items():
        parts, caps = [c.data for c, _ in units], [cap for _, cap in units]
        outs, ol, iu, st = run_batch(gpu, fmt, parts, caps, flags=flags)
        ref = oracle_batch(fmt, parts, caps)
        for j, (c, cap) in enumerate(units):
            r_out, r_used, r_st = ref[j]
            if r_st == 2 and c.want == K.Err(2, None):  # zlib's Z_NEED_DICT is the batch status CHIP_NEED_DICT (3)
                r_st = 3
            where = (c.name, cap, int(st[j]), r_st, int(iu[j]), r_used)
            assert outs[j] == r_out, where + (len(outs[j]), len(r_out))
            if flags & compu_amd.F_COMPU_STATUS:
                assert int(st[j]) == r_st, where
                if r_st in (1, 2):
                    assert int(iu[j]) == r_used, where
                continue
            # the two documented batch deviations (include/compu_hip.h, chip_decode_batch), as test_inflate_gpu pins them
            if r_st == 0 and len(r_out) == cap and r_used == len(c.data) and st[j] != 0:
                assert st[j] == 1, where
                continue
            assert int(st[j]) == r_st, where
            if r_st == 2:
                assert int(iu[j]) == r_used, where


def test_hand_built_batch(gpu, cases):
    _batch(gpu, cases, 0)


def test_hand_built_batch_compu_status(gpu, cases):
    import compu_amd

    _batch(gpu, cases, compu_amd.F_COMPU_STATUS)


def _oracle_call(d):
    def call(chunk, room):
        got, ir, orr, st, err = d.decode(chunk, room)
        return (None if err else st), err, got, ir, orr
    return call


def _gpu_call(dec, room):
    buf = bytearray(room)

    def call(chunk, room):
        r = dec.decode(chunk, buf)
        if r.is_ok():
            return int(r.status), 0, bytes(buf[: room - r.output_remain]), r.input_remain, r.output_remain
        return None, r.status.as_raw(), bytes(buf[: room - r.output_remain]), r.input_remain, r.output_remain
    return call


def _stream_runs(c):
    n = len(c.content) + 64
    runs = [([], n), (c.cuts, n)]
    if len(c.content) <= (1 << 20):  # (a single large block is decoded again from its start on every call)
        runs += [([], 4096), (c.cuts, 4096)]
    if len(c.content) <= 20000:
        runs.append((c.cuts, 13))
    if "hdr_cut" in c.tags or "gz_header_cut" in c.tags:
        runs.append((range(1, len(c.data)), 13))  # the header itself in 1-byte pieces
    elif len(c.data) <= 4096 and len(c.content) <= 4096:
        runs += [(range(1, len(c.data)), n), (range(7, len(c.data), 7), 13), ([], 1), (range(7, len(c.data), 7), 1)]
    return runs


def test_hand_built_streaming(gpu, cases):
    import compu_amd

    decs = {}
    for c in cases:
        if c.fmt not in decs:
            decs[c.fmt] = compu_amd.decoder_interface.zlib_hip(compu_amd.ZlibMode(K.MODES[c.fmt]))
        dec = decs[c.fmt]
        for cuts, room in _stream_runs(c):
            dec.reset()
            got = zstd_ref.drive(_gpu_call(dec, room), c.data, cuts, room)
            want = zstd_ref.drive(_oracle_call(O.InflateDecoder(K.MODES[c.fmt])), c.data, cuts, room)
            where = (c.name, len(cuts), room)
            for k, (x, y) in enumerate(zip(got, want)):
                if x[0] is None and y[0] == 1 and y[4] == 0 and c.want == K.FAR and x[2] == y[2] and want[k + 1][:3] == (None, -3, b""):
                    # (open) the streaming decoder reports a match too far back in the call whose output fills the
                    # room in front of it; zlib only tests the distance once there is room, so the error comes one call later
                    break
                if y[0] == 0 and x[0] == 1 and x[2] == y[2] and x[4] == y[4] == 0:
                    # the output filled as the input ran out: zlib's Z_OK with avail_in == 0 is NeedInput to compu (and its loop stops
                    # at the end of the input), the streaming decoder names the limit it hit, as the batch API does.
                    # The runs part here; what the decoder goes on to produce must still be the content
                    out = b"".join(r[2] for r in got)
                    assert c.content.startswith(out) and (got[-1][0] != 2 or out == c.want), where
                    break
                # on NeedOutput zlib keeps the input of the token it could not finish, the streaming decoder takes all of it
                # (DESIGN.md sec. 4.4); an erroring call's input_remain is left open: everything else of every
                # call is the oracle's
                same = x == y or (y[0] in (1, None) and x[:3] == y[:3] and x[4] == y[4])
                assert same, where + (k, x[:2], x[3:], len(x[2]), y[:2], y[3:], len(y[2]))
            else:
                assert len(got) == len(want), where + (len(got), len(want))


def test_wrapped_cases_route_like_single_format_runs(gpu, cases):
    """CHIP_FMT_DETECT over the zlib / gzip cases mixed with the zstd hand frames: each unit is routed by Detection and decodes as
    in a batch of its own format"""
    import compu_amd
    import zstd_cases
    from test_zstd_gpu import FMT_ZSTD

    wrapped = [c for c in cases if c.fmt in ("zlib", "gzip", "auto")]
    frames = zstd_cases.all_cases()
    parts, caps, fmts = [], [], []
    for i in range(max(len(wrapped), len(frames))):
        if i < len(wrapped):
            c = wrapped[i]
            parts.append(c.data)
            caps.append(_ref_len(c) + 4096)
            fmts.append(K.MODES["auto"])
        if i < len(frames):
            f = frames[i]
            parts.append(f.frame)
            caps.append((len(f.want) if isinstance(f.want, bytes) else 1 << 18) + 4096)
            fmts.append(FMT_ZSTD)
    outs, ol, iu, st = run_batch(gpu, 0, parts, caps, check_tail=False)
    routed = 0
    for fmt in (K.MODES["auto"], FMT_ZSTD):
        idx = [j for j in range(len(parts)) if fmts[j] == fmt]
        kinds = [compu_amd.Detection.detect(parts[j]) for j in idx]
        mine = [j for j, k in zip(idx, kinds) if k in ((compu_amd.Detection.Zstd,) if fmt == FMT_ZSTD else (compu_amd.Detection.Gzip, compu_amd.Detection.Zlib))]
        o2, ol2, iu2, st2 = run_batch(gpu, fmt, [parts[j] for j in mine], [caps[j] for j in mine], check_tail=False)
        for k, j in enumerate(mine):
            assert (outs[j], int(ol[j]), int(iu[j]), int(st[j])) == (o2[k], int(ol2[k]), int(iu2[k]), int(st2[k])), (fmt, j)
        routed += len(mine)
    assert routed >= 0.9 * len(parts)
