"""The built inputs of the LZ4 encoder tests, shared by the CPU and the GPU tests, and the sequence lister that proves the duties of
the block format on an encoded block (include/compu_hip.h, "LZ4: encoding").  An input is (name, bytes)."""
import functools
import os

import lz4_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_LEVELS = (1, 4, 9)  # one level of each finder group: 1-2, 3-5, 6-12
S_BCHK, S_NO_CCHK, S_ID_SHIFT = 1, 2, 4  # CHIP_LZ4_S_*
FAR = (65534, 65535, 65536, 65537, 70000)  # distances of the repeated word: the first two may be used, the others must not


def alice():
    with open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb") as f:
        return f.read()


def mix(n, seed):
    """stretches of text and of random bytes"""
    out, k = bytearray(), 0
    while len(out) < n:
        out += K.text(40000, seed + k) if k % 2 == 0 else K.noise(25000, seed + k)
        k += 1
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def inputs():
    c = []
    for n in (0, 1, 4, 5, 11, 12, 13, 14, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 65535, 65536, 65537):
        c.append((f"text{n}", K.text(n, n + 1)))
    for n in (14, 15, 16, 269, 270, 271, 524, 525, 70000):  # the literal-length extension edges
        c.append((f"noise{n}", K.noise(n, n)))
    for period in (1, 2, 3, 5):  # match-length edges, overlapping copies
        for n in (19, 20, 273, 274, 275, 528, 529, 100000):
            c.append((f"run{period}_{n}", (bytes(range(65, 65 + period)) * (n // period + 1))[:n]))
    word = K.noise(200, 77)
    for d in FAR:
        c.append((f"far{d}", word + K.noise(d - 200, d) + word + b"the end of it."))
    t = K.text(300, 5)
    c.append(("match_to_the_end", t + t))
    c.append(("match_to_the_end_short", K.noise(20, 3) * 2))
    for phase in range(64):  # a repeat that straddles the boundary between two chunks of 64 positions
        w = K.noise(40, 1000 + phase)
        c.append((f"straddle{phase}", K.noise(108 + phase, phase) + w + K.noise(30, 64 + phase) + w + K.noise(20, 128 + phase)))
    a = alice()
    c.append(("alice", a))
    c.append(("alice64k", a[:65536]))
    c.append(("mix1m", mix(1 << 20, 9)))
    return tuple(c)


def frame_inputs():
    """the inputs on which frames of every option and block size are made"""
    pick = ("text0", "text1", "text13", "text65535", "text65536", "text65537", "noise70000", "run3_100000", "alice")
    return tuple(x for x in inputs() if x[0] in pick) + (("mix300k", mix(300000, 4)),)


def frame_options():
    """every option combination with every block-size id"""
    return tuple(bits | (i << S_ID_SHIFT) for i in (0, 4, 5, 6, 7) for bits in (0, S_BCHK, S_NO_CCHK, S_BCHK | S_NO_CCHK))


def sequences(block):
    """[(literal length, offset, match length)] of a well-formed block; the last has offset None (the closing literal run)"""
    n, p, out = len(block), 0, []

    def ext(p, v):
        while True:
            b = block[p]
            p += 1
            v += b
            if b != 255:
                return p, v

    while True:
        token = block[p]
        p += 1
        ll = token >> 4
        if ll == 15:
            p, ll = ext(p, ll)
        p += ll
        assert p <= n, "literals beyond the block"
        if p == n:
            out.append((ll, None, 0))
            return out
        off = block[p] | (block[p + 1] << 8)
        p += 2
        ml = token & 15
        if ml == 15:
            p, ml = ext(p, ml)
        out.append((ll, off, ml + 4))


def check_duties(block, n):
    """the duties liblz4's decoders rely on, for a block that encodes n bytes: offsets 1 .. 65535 that reach no further back than the
    bytes produced so far; no match starts within the last 12 bytes or ends within the last 5; fewer than 13 bytes are one run"""
    o = 0
    seqs = sequences(block)
    for ll, off, ml in seqs:
        o += ll
        if off is None:
            break
        assert 1 <= off <= 65535 and off <= o, (off, o)
        assert o + 12 <= n, ("a match starts at", o, n)
        assert o + ml + 5 <= n, ("a match ends at", o + ml, n)
        o += ml
    assert o == n, (o, n)
    if n < 13:
        assert len(seqs) == 1
    return seqs
