"""The hand-built brotli streams of tests/brotli_form_cases.py on the GPU against libbrotlidec: every form and every error in one
batch, every byte-cut prefix, every output capacity, every input alignment, and the streaming decoder call for call.
tests/test_brotli_forms_cpu.py checks the same cases against libbrotlidec alone and that they cover every form."""
import numpy as np
import pytest

import brotli_cases as K
import brotli_form_cases as F
import brotli_ref as B
from test_brotli_gpu import FMT_BROTLI, _batch, _check_parity
from test_brotli_hand_gpu import _gpu_calls

pytestmark = pytest.mark.gpu
ERR_CAP = 2048  # no error stream has as much output


@pytest.fixture(scope="module")
def cases():
    return F.all_cases()


@pytest.fixture(scope="module")
def units(cases):
    """(name, stream, capacity, output or None) of the batch of all cases: valid ones at exact capacity and 16 above, and the
    unit of 256 trees per category from tests/brotli_cases.py, whose tables take the second launch"""
    us = []
    for c in cases:
        if c.err is None:
            us.append((c.name, c.stream, len(c.out), c.out))
            us.append((c.name + "+16", c.stream, len(c.out) + 16, c.out))
        else:
            us.append((c.name, c.stream, ERR_CAP, None))
    comp, out = K.many_trees()
    us.insert(len(us) // 2, ("many_trees", comp, len(out), out))
    return us


@pytest.fixture(scope="module")
def unit_refs(units):
    return [B.decode(p, cap) for _, p, cap, _ in units]


def _small(cases):
    return [c for c in cases if c.err is not None or len(c.stream) < 300]


def _check_units(units, refs, got):
    for (name, p, cap, out), ref, g in zip(units, refs, got):
        _check_parity(g, ref, name)
        if out is not None:
            assert g[1] == B.FINISHED and g[0] == out and g[2] == len(p), (name, g[1])
        else:
            assert g[1] < 0, (name, g[1])


def test_all_cases_one_batch(gpu, units, unit_refs):
    got = _batch(gpu, [p for _, p, _, _ in units], [cap for _, _, cap, _ in units])
    _check_units(units, unit_refs, got)


def _run_at(torch, parts, caps, mis):
    """run_batch of test_inflate_gpu with every unit's input `mis` bytes behind a dword boundary"""
    import compu_amd

    offs, o = [], 0
    for p in parts:
        o = ((o + 3) & ~3) + mis
        offs.append(o)
        o += len(p)
    buf = np.full(((o + 3) & ~3) + 8, 0xEE, np.uint8)  # what lies between the units is not zero
    for p, at in zip(parts, offs):
        buf[at:at + len(p)] = np.frombuffer(p, np.uint8)
    caps = np.asarray(caps, dtype=np.int32)
    ooff = np.zeros(len(parts), dtype=np.int64)
    ooff[1:] = np.cumsum((caps[:-1].astype(np.int64) + 15) & ~15)
    dev = "cuda:0"
    d_out = torch.full((int(ooff[-1] + caps[-1]) + 16,), 0xA5, dtype=torch.uint8, device=dev)
    ol, iu, st = compu_amd.decode_batch(FMT_BROTLI, torch.from_numpy(buf).to(dev), torch.from_numpy(np.array(offs, np.int64)).to(dev),
                                        torch.from_numpy(np.array([len(p) for p in parts], np.int32)).to(dev), d_out,
                                        torch.from_numpy(ooff).to(dev), torch.from_numpy(caps).to(dev))
    torch.cuda.synchronize()
    h_out = d_out.cpu().numpy()
    ol, iu, st = ol.cpu().numpy(), iu.cpu().numpy(), st.cpu().numpy()
    got = []
    for i in range(len(parts)):
        tail = h_out[ooff[i] + ol[i]: ooff[i] + ((caps[i] + 15) & ~15)]
        assert (tail == 0xA5).all(), f"unit {i}: wrote past its output range"
        got.append((bytes(h_out[ooff[i]: ooff[i] + ol[i]]), int(st[i]), int(iu[i])))
    return got


@pytest.mark.parametrize("mis", [1, 2, 3])
def test_input_alignment(gpu, units, unit_refs, mis):
    """each unit's input 1, 2 and 3 bytes into a dword: the kernel reads from the aligned address below it"""
    got = _run_at(gpu, [p for _, p, _, _ in units], [cap for _, _, cap, _ in units], mis)
    _check_units(units, unit_refs, got)
    # and cut short there, where the bytes behind the unit's end are not zero
    small = [u for u in units if len(u[1]) < 300 and not u[0].endswith("+16")]
    parts, caps = [], []
    for name, p, cap, _ in small:
        for cut in range(0, len(p), 3):
            parts.append(p[:cut])
            caps.append(cap)
    got = _run_at(gpu, parts, caps, mis)
    for p, cap, g in zip(parts, caps, got):
        ref = B.decode(p, cap)
        _check_parity(g, ref, p.hex())


def test_every_cut_prefix(gpu, cases):
    """every prefix of every small valid stream and of every error stream: whatever libbrotlidec says of it"""
    parts, caps, names = [], [], []
    for c in _small(cases):
        cap = len(c.out) + 16 if c.err is None else ERR_CAP
        for cut in range(len(c.stream)):
            parts.append(c.stream[:cut])
            caps.append(cap)
            names.append("%s cut %d" % (c.name, cut))
    assert len(parts) < 20000
    got = _batch(gpu, parts, caps)
    for p, cap, name, g in zip(parts, caps, names, got):
        ref = B.decode(p, cap)
        _check_parity(g, ref, name)
        if ref[0] == B.FINISHED:  # a stream that is whole before its last byte (the bits left are padding)
            assert g[0] == ref[1]


def _sweep_caps(c):
    n = len(c.out)
    if n < 2000:
        return list(range(n))
    caps = {0, 1, n - 1}
    for b in c.bounds:
        caps |= {b - 1, b, b + 1}
    caps = {x for x in caps if 0 <= x < n}
    k = 0
    while len(caps) < 32:  # filled up to 32 with capacities spread over the output
        caps.add((n * (2 * k + 1)) // 64 + k)
        k += 1
    return sorted(caps)


def test_capacity_sweep(gpu, cases):
    """every capacity short of the output gives NEED_OUTPUT and exactly that much of the output"""
    parts, caps, names = [], [], []
    for c in cases:
        if c.err is None and c.out:
            for cap in _sweep_caps(c):
                parts.append(c.stream)
                caps.append(cap)
                names.append("%s cap %d" % (c.name, cap))
    got = _batch(gpu, parts, caps)
    for c, name, g in zip(caps, names, got):
        assert g[1] == B.NEED_OUTPUT, (name, g[1])
    by = {c.name: c for c in cases}
    for cap, name, g in zip(caps, names, got):
        assert g[0] == by[name.split(" cap ")[0]].out[:cap], name


def test_streaming_call_for_call(gpu, cases):
    """Decoder::decode of brotli_hip() with room for everything and with 61 bytes: each call's status and bytes are libbrotlidec's"""
    import compu_amd

    dec = compu_amd.decoder_interface.brotli_hip()
    for c in _small(cases):
        for cap in (1 << 20, 61):
            want = B.stream_calls(c.stream, cap)
            got = _gpu_calls(dec, c.stream, cap)
            assert [(st, o) for st, o, _ in got] == [(st, o) for st, o, _ in want], (c.name, cap)
            if want[-1][0] == B.FINISHED:
                assert got[-1][2] == want[-1][2] and b"".join(o for _, o, _ in got) == c.out, (c.name, cap)
