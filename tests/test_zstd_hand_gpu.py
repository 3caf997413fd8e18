"""zstd on the GPU against hand-built frames (tests/zstd_cases.py): every case in one batch launch at three capacities, and
every case through the streaming decoder -- whole, cut at its blocks (so that treeless and repeat-mode blocks start a call from
the checkpoint), and in 1- and 7-byte pieces -- call by call against the oracle, which tests/test_zstd_writer_cpu.py pins to
the system libzstd."""
import pytest

import zstd_cases as K
import zstd_ref
from oracle import oracle as O
from test_inflate_gpu import run_batch
from test_zstd_gpu import FMT_ZSTD, oracle_zstd_batch

pytestmark = pytest.mark.gpu
ERR_CAP = 1 << 18  # output capacity of the cases that end in an error


@pytest.fixture(scope="module")
def cases():
    return K.all_cases()


def _size(c):
    return len(c.want) if isinstance(c.want, bytes) else ERR_CAP


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


def test_hand_built_batch(gpu, cases):
    parts, caps, idx = [], [], []
    for i, c in enumerate(cases):
        n = _size(c)
        for cap in {n, n + 4096} | ({n - 1} if n > 0 and isinstance(c.want, bytes) else set()):
            parts.append(c.frame)
            caps.append(cap)
            idx.append(i)
    outs, ol, iu, st = run_batch(gpu, FMT_ZSTD, parts, caps, check_tail=False)  # (the poison behind every range is checked there)
    ref = oracle_zstd_batch(parts, caps)
    for j, (i, cap) in enumerate(zip(idx, caps)):
        c = cases[i]
        r_out, r_used, r_st = ref[j]
        if cap >= _size(c):
            assert (r_out if r_st == 2 else r_st) == c.want, (c.name, cap, r_st)
        if r_st == 1:
            # not enough room: the batch kernel works on whole blocks (include/compu_hip.h, chip_decode_batch) -- the same NeedOutput
            # with the whole blocks that fit, or the verdict on a block that does not fit and is itself broken
            big = oracle_zstd_batch([c.frame], [cap + (1 << 20)])[0]
            assert st[j] == 1 or (big[2] < 0 and st[j] == big[2]), (c.name, cap, int(st[j]), big[2])
            assert len(outs[j]) <= cap and outs[j] == r_out[: len(outs[j])], (c.name, cap)
            continue
        assert int(st[j]) == r_st, (c.name, cap, int(st[j]), r_st)
        if r_st in (0, 2):
            assert outs[j] == r_out, (c.name, cap, len(outs[j]), len(r_out))
        if r_st == 2:
            assert int(iu[j]) == r_used, (c.name, cap, int(iu[j]), r_used)


def test_hand_built_streaming(gpu, cases):
    import compu_amd

    dec = compu_amd.decoder_interface.zstd_hip()
    for c in cases:
        n = _size(c) + 64
        runs = [([], n), ([], 4096), (c.cuts, n), (c.cuts, 4096)] + ([(c.cuts, 13)] if _size(c) <= 20000 else [])
        if len(c.frame) <= 4096:
            runs += [(range(1, len(c.frame)), n), (range(7, len(c.frame), 7), 13)]
        if _size(c) <= 4096:
            runs += [([], 1), (range(7, len(c.frame), 7), 1)]
        for cuts, room in runs:
            dec.reset()
            got = zstd_ref.drive(_gpu_call(dec, room), c.frame, cuts, room)
            want = zstd_ref.drive(_oracle_call(O.ZstdDecoder()), c.frame, cuts, room)
            for k, (x, y) in enumerate(zip(got, want)):
                assert x == y, (c.name, len(cuts), room, k, x[:2], x[3:], len(x[2]), y[:2], y[3:], len(y[2]))
            assert len(got) == len(want), (c.name, len(cuts), room, len(got), len(want))
            end = want[-1]
            assert (end[1] if end[0] is None else b"".join(x[2] for x in want)) == c.want, (c.name, room)
