"""CHIP_F_MEMBERS on the GPU: units that are series of gzip members or zstd frames (tests/members_cases.py), decode and size pass.
Every unit is held against two yardsticks: the walk of include/compu_hip.h with the unflagged chip_decode_batch as decode1 (the
contract to the letter: status, out_len, in_used and bytes), and the same walk over the CPU oracle (tests/members_ref.py: status
always, everything on CHIP_FINISHED).  Without the feature every test here fails: the flag is CHIP_E_INVALID."""
import zlib

import numpy as np
import pytest

import members_cases as MC
import members_ref as R
from test_inflate_gpu import _pack

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F_MEMBERS = 2
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
AMPLE = 1 << 19  # more than any unit here decodes to (the size-pass test aside)


def decode(torch, fmt, units, caps, flags):
    """one launch; result arrays and output are poisoned first.  -> (outputs, out_len, in_used, status)"""
    import compu_amd

    buf, offs, lens = _pack(units)
    n = len(units)
    caps = np.asarray(caps, dtype=np.int64)
    ooff = np.zeros(n, dtype=np.int64)
    ooff[1:] = np.cumsum((caps[:-1] + 15) & ~15)
    total_out = int(ooff[-1] + caps[-1]) + 16
    d_out = torch.full((total_out,), 0xA5, dtype=torch.uint8, device=DEV)
    ol = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    iu = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    st = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    compu_amd.decode_batch(fmt, torch.from_numpy(buf).to(DEV), torch.from_numpy(offs).to(DEV), torch.from_numpy(lens).to(DEV), d_out,
                           torch.from_numpy(ooff).to(DEV), torch.from_numpy(caps.astype(np.int32)).to(DEV), ol, iu, st, flags=flags)
    torch.cuda.synchronize()
    h = d_out.cpu().numpy()
    ol, iu, st = ol.cpu().numpy(), iu.cpu().numpy(), st.cpu().numpy()
    assert (ol != POISON32).all() and (iu != POISON32).all() and (st != POISON32).all(), "a result entry was not written"
    for i in range(n):  # nothing behind the unit's capacity is touched (inside it zstd may park literals: documented scratch use)
        assert (h[ooff[i] + caps[i]: ooff[i] + ((caps[i] + 15) & ~15)] == 0xA5).all(), f"unit {i}: wrote past its output range"
        if fmt != R.ZSTD and fmt != 0:
            assert (h[ooff[i] + ol[i]: ooff[i] + caps[i]] == 0xA5).all(), f"unit {i}: wrote behind its output"
    return [bytes(h[ooff[i]: ooff[i] + ol[i]]) for i in range(n)], ol, iu, st


def sizes(torch, fmt, units, flags):
    import compu_amd

    buf, offs, lens = _pack(units)
    n = len(units)
    size = torch.full((n,), POISON64, dtype=torch.int64, device=DEV)
    used = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    st = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    compu_amd.decode_batch_sizes(fmt, torch.from_numpy(buf).to(DEV), torch.from_numpy(offs).to(DEV), torch.from_numpy(lens).to(DEV), size, used, st, flags=flags)
    torch.cuda.synchronize()
    size, used, st = size.cpu().numpy(), used.cpu().numpy(), st.cpu().numpy()
    assert (size != POISON64).all() and (used != POISON32).all() and (st != POISON32).all(), "a result entry was not written"
    return size, used, st


def gpu_walk(torch, fmt, units, caps):
    """the walk with the unflagged chip_decode_batch as decode1, all units abreast: one launch per member depth"""
    n = len(units)
    p, total, outs, first = [0] * n, [0] * n, [b""] * n, [b""] * n
    ans, active = [None] * n, list(range(n))
    while active:
        o, ol, iu, st = decode(torch, fmt, [units[i][p[i]:] for i in active], [caps[i] - total[i] for i in active], 0)
        nxt = []
        for j, i in enumerate(active):
            total[i] += int(ol[j])
            outs[i] += o[j]
            if st[j] != R.FINISHED:
                ans[i] = (int(st[j]), total[i], len(units[i]) if st[j] == R.NEED_INPUT else p[i] + int(iu[j]), outs[i])
                continue
            first[i] = units[i][p[i]:p[i] + 2]
            p[i] += int(iu[j])
            if iu[j] > 0 and R.starts_member(fmt, units[i], p[i], first[i]):
                nxt.append(i)
            else:
                ans[i] = (R.FINISHED, total[i], p[i], outs[i])
        active = nxt
    return ans


@pytest.fixture(scope="module")
def cases():
    return MC.all_cases()


@pytest.fixture(scope="module")
def oracle_answers(cases):
    return {c.name: R.walk(c.fmt, c.unit, c.cap if c.cap is not None else AMPLE) for c in cases}


def _check(torch, cs, oracle_answers):
    for fmt in sorted({c.fmt for c in cs}):
        sel = [c for c in cs if c.fmt == fmt]
        units, caps = [c.unit for c in sel], [c.cap if c.cap is not None else AMPLE for c in sel]
        o, ol, iu, st = decode(torch, fmt, units, caps, F_MEMBERS)
        want = gpu_walk(torch, fmt, units, caps)
        for j, c in enumerate(sel):
            got = (int(st[j]), int(ol[j]), int(iu[j]), o[j])
            a = oracle_answers[c.name]
            print(c.name, got[:3], want[j][:3], tuple(a[:3]))
            assert got == want[j], c.name
            if (got[0], a.status) == (R.NEED_OUTPUT, R.NEED_INPUT) and c.fmt != R.ZSTD and got[1] == caps[j] and a.in_used == len(c.unit):
                continue  # output full AND every input byte consumed: the batch status names the limit that was hit (tests/test_inflate_gpu.py)
            assert got[0] == a.status, c.name
            if a.status == R.FINISHED:
                assert got[1:] == (a.out_len, a.in_used, a.data), c.name
            elif a.status == R.NEED_INPUT:
                assert got[2] == len(c.unit), c.name


def test_shapes(gpu, oracle_answers):
    cs = MC.shape_cases()
    _check(gpu, cs, oracle_answers)
    assert all(oracle_answers[c.name].status == R.FINISHED or not c.unit for c in cs)


def test_base_reset(gpu, oracle_answers):
    _check(gpu, MC.base_reset_cases(), oracle_answers)
    o, ol, iu, st = decode(gpu, R.GZIP, [c.unit for c in MC.base_reset_cases()[:2]], [AMPLE] * 2, F_MEMBERS)
    assert list(st) == [R.FINISHED, -3] and o[0] == b"abcdefgh" * 4 + b"abcabc" and ol[1] == 32 + 3
    o, ol, iu, st = decode(gpu, R.ZSTD, [c.unit for c in MC.base_reset_cases()[2:]], [AMPLE] * 5, F_MEMBERS)
    assert list(st) == [R.FINISHED, -20, R.FINISHED, R.FINISHED, R.FINISHED]
    assert o[2].endswith(b"ABCDDDDDDEDED") and o[3].endswith(b"ABCDABCDAEAEA") and o[4].endswith(b"ABCDEFGHABCDEIEIE")


def test_what_follows_a_member(gpu, oracle_answers):
    _check(gpu, MC.tail_cases(), oracle_answers)


def test_zstd_frames(gpu, oracle_answers):
    _check(gpu, MC.zstd_cases(), oracle_answers)


def test_damage_in_member_k(gpu, oracle_answers):
    cs = MC.damage_cases()
    _check(gpu, cs, oracle_answers)
    assert all(oracle_answers[c.name].status < 0 for c in cs)


def test_capacity(gpu, oracle_answers):
    cs = MC.capacity_cases()
    _check(gpu, cs, oracle_answers)
    assert oracle_answers["gzip_cap_total"].status == oracle_answers["zstd_cap_total"].status == R.FINISHED


def test_size_pass_equals_the_flagged_decode(gpu, cases):
    """rule 1 on every unit above; rule 3: a decode into exactly out_size never lacks room; rule 4: the check-value cases read
    CHIP_FINISHED"""
    for fmt in (R.GZIP, R.AUTO, R.ZSTD):
        sel = [c for c in cases if c.fmt == fmt]
        units = [c.unit for c in sel]
        size, used, st = sizes(gpu, fmt, units, F_MEMBERS)
        o, ol, iu, dst = decode(gpu, fmt, units, [AMPLE] * len(sel), F_MEMBERS)
        x, xol, xiu, xst = decode(gpu, fmt, units, [int(s) for s in size], F_MEMBERS)
        for j, c in enumerate(sel):
            where = (c.name, int(st[j]), int(size[j]), int(used[j]), int(dst[j]), int(ol[j]), int(iu[j]), int(xst[j]))
            print(*where)
            if "_bad_crc_" in c.name or "_bad_xxh64_" in c.name:  # rule 4: the whole series is counted, the decode reports the fault
                assert int(st[j]) == R.FINISHED and int(dst[j]) in (-3, -22) and int(size[j]) >= int(ol[j]), where
            else:
                assert (int(st[j]), int(size[j]), int(used[j])) == (int(dst[j]), int(ol[j]), int(iu[j])), where
            if st[j] == R.FINISHED:
                assert int(xst[j]) != R.NEED_OUTPUT, where


def test_size_pass_counts_past_4_gib(gpu):
    """2112 members of 2 MiB of zeros each (about 4.3 MB of input): the 64-bit total is above 2^32"""
    count, n = 2112, 2 << 20
    member = MC.gz(b"\0" * n, 9)
    unit = member * count
    assert count * n > 1 << 32 and len(unit) < 512 << 20
    size, used, st = sizes(gpu, R.GZIP, [unit, member], F_MEMBERS)
    assert (int(st[0]), int(size[0]), int(used[0])) == (R.FINISHED, count * n, len(unit))
    assert (int(st[1]), int(size[1]), int(used[1])) == (R.FINISHED, n, len(member))


def test_single_member_units_answer_the_same_with_and_without_the_flag(gpu):
    units = [MC.gz_kind(MC.payload(n * 37 % 3000, n), ("stored", "fixed", "dynamic")[n % 3]) for n in range(300)]
    units[7], units[8] = units[7][:-3], units[8][:10] + b"\xff" + units[8][11:]  # a cut and a damaged one among them
    caps = [n * 37 % 3000 + (0 if n % 5 else -1 if n * 37 % 3000 else 0) for n in range(300)]
    zunits = [MC.zframe(MC.payload(n * 41 % 3000, n), checksum=bool(n & 1), fcs=bool(n & 2))[0] for n in range(300)]
    for fmt, us in ((R.GZIP, units), (R.AUTO, units), (R.ZSTD, zunits), (0, units[:150] + zunits[:150])):
        a = decode(gpu, fmt, us, caps, 0)
        b = decode(gpu, fmt, us, caps, F_MEMBERS)
        assert a[0] == b[0] and all((x == y).all() for x, y in zip(a[1:], b[1:])), fmt
        sa, sb = sizes(gpu, fmt, us, 0), sizes(gpu, fmt, us, F_MEMBERS)
        assert all((x == y).all() for x, y in zip(sa, sb)), fmt


def test_routed_batch(gpu, cases):
    """CHIP_FMT_DETECT: a multi-member gzip unit, a multi-frame zstd unit, a single zlib unit and an unknown unit, each as in a batch of
    its own format"""
    by = {c.name: c for c in cases}
    g, z = by["gzip_dynamic_all_lengths"].unit, by["zstd_golden"].unit
    zl, unk = zlib.compress(MC.payload(5000, 3)) + MC.gz(b"not continued"), b"what is this" * 3
    units = [g, z, zl, unk, by["gzip_bad_crc_in_2"].unit, by["zstd_skippable_between"].unit]
    o, ol, iu, st = decode(gpu, 0, units, [AMPLE] * len(units), F_MEMBERS)
    size, used, sst = sizes(gpu, 0, units, F_MEMBERS)
    for j, fmt in ((0, R.GZIP), (1, R.ZSTD), (2, R.AUTO), (4, R.GZIP), (5, R.ZSTD)):
        o1, ol1, iu1, st1 = decode(gpu, fmt, [units[j]], [AMPLE], F_MEMBERS)
        assert (o[j], int(ol[j]), int(iu[j]), int(st[j])) == (o1[0], int(ol1[0]), int(iu1[0]), int(st1[0])), j
        s1, u1, t1 = sizes(gpu, fmt, [units[j]], F_MEMBERS)
        assert (int(size[j]), int(used[j]), int(sst[j])) == (int(s1[0]), int(u1[0]), int(t1[0])), j
    assert st[0] == st[1] == st[2] == R.FINISHED and len(o[0]) == sum(MC.LENGTHS) and o[2] == MC.payload(5000, 3)
    o0, ol0, iu0, st0 = decode(gpu, 0, units, [AMPLE] * len(units), 0)  # the unknown unit: as without the flag
    assert (o[3], int(ol[3]), int(iu[3]), int(st[3])) == (o0[3], int(ol0[3]), int(iu0[3]), int(st0[3]))
