"""Built inputs for the zstd encoder, each with the condition it must reach: a predicate over what zstd_frame_reader.read_frame says
about the frame.  Every input is ordinary data; what makes it a case is that the frame it encodes to sits on a threshold of RFC 8878
(a field that changes width, a code with extra bits at its end, a block that exactly fills 128 KiB) or of the encoder itself (the
64 KiB reach of the hash table, the 16-literal floor of the Huffman stage, the 11-bit depth limit).  The CPU test asserts every
condition on the host core's frame, the GPU test on the kernel's, so a case that stops reaching its threshold fails loudly.

all_cases() -> [(name, data, groups, condition)]: `groups` are the match-finder groups (0..3) the condition holds in; an entry
(0, skip_shift) names group 0 at that skip_shift alone, where a faster skip steps over what the case is about (holds_in)."""
import functools
import random

from conftest import golden

ALL = (0, 1, 2, 3)
BLOCK = 128 << 10


def holds_in(groups, group, skip_shift):
    return group in groups or (group, skip_shift) in groups


# ---- what conditions look at -------------------------------------------------------------------------------------------------------
def cblocks(info):
    return [b for b in info["blocks"] if b["type"] == "compressed"]


def types(info):
    return [b["type"] for b in info["blocks"]]


def all_seqs(info):
    """(llc, ll, mlc, ml, ofv, resolved offset) of every sequence of the frame"""
    return [s + (o,) for b in cblocks(info) for s, o in zip(b["seqs"], b["offsets"])]


def huffman_depth(literals):
    """The depth of the (unlimited) Huffman tree the encoder's construction gives for these literals: leaves sorted by count then
    symbol, two queues, a leaf preferred to an internal node of the same weight."""
    cnt = {}
    for b in literals:
        cnt[b] = cnt.get(b, 0) + 1
    leaves = sorted((c, s) for s, c in cnt.items())
    weight = [c for c, _ in leaves]
    n = len(weight)
    parent = {}
    li, ni = 0, n
    for _ in range(n - 1):
        pick = []
        for _t in range(2):
            if li < n and (ni >= len(weight) or weight[li] <= weight[ni]):
                pick.append(li)
                li += 1
            else:
                pick.append(ni)
                ni += 1
        weight.append(weight[pick[0]] + weight[pick[1]])
        parent[pick[0]] = parent[pick[1]] = len(weight) - 1
    depth = {len(weight) - 1: 0}
    for i in range(len(weight) - 2, -1, -1):
        depth[i] = depth[parent[i]] + 1
    return max(depth[i] for i in range(n)) if n > 1 else 0


# ---- builders ------------------------------------------------------------------------------------------------------------------------
def word_stream(nwords, seed=1):
    """Eight 4-byte words over 32 distinct byte values; each next word differs from the current one and from the word that followed
    the current word's previous occurrence, so a match of a word against its previous occurrence is exactly 4 bytes long and the next
    one starts right behind it (literal length 0).  The words come in one or two at a time between words already seen, so that no run
    of literals is longer than 8 and no setting of the match finder steps over a word."""
    rnd = random.Random(seed)
    vals = rnd.sample(range(256), 32)
    words = [bytes(vals[4 * i:4 * i + 4]) for i in range(8)]
    out, follow = [0, 1, 0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5, 7, 6], {}
    for a, b in zip(out, out[1:]):
        assert a != b and follow.get(a) != b
        follow[a] = b
    cur = out[-1]
    while len(out) < nwords:
        nxt = rnd.choice([w for w in range(8) if w != cur and w != follow.get(cur)])
        follow[cur] = nxt
        out.append(nxt)
        cur = nxt
    return b"".join(words[w] for w in out[:nwords])


def no_repeat(n, alphabet, seed):
    """n bytes over `alphabet` in which no 4 bytes occur twice, also not across the seam of two copies laid end to end: encoded as
    x + x, the first copy is n literals and the second one match, whatever the match finder"""
    alphabet = list(alphabet)
    for attempt in range(1000):
        rnd = random.Random(seed * 1000 + attempt)
        out, seen, dead = bytearray(rnd.choice(alphabet) for _ in range(min(n, 3))), set(), False
        while len(out) < n and not dead:
            cand = alphabet[:]
            rnd.shuffle(cand)
            for c in cand:
                g = bytes(out[-3:]) + bytes([c])
                if g not in seen:
                    seen.add(g)
                    out.append(c)
                    break
            else:
                dead = True
        if dead:
            continue
        seam = [bytes((out + out)[n - 3 + i:n + 1 + i]) for i in range(3)] if n >= 4 else []
        if len(set(seam)) == len(seam) and not any(g in seen for g in seam):
            return bytes(out)
    raise AssertionError("no such sequence found")


def doubled(n, alphabet, seed):
    x = no_repeat(n, alphabet, seed)
    return x + x


def chunked(n, alphabet, seed):
    """n literals that no setting of the match finder skips over: pieces of 8 literals (then 4 and less), each followed by a copy
    of the 8 bytes before it.  No 4 bytes that begin at a literal occur earlier, the literal behind a copy differs from what the copy
    would go on with, and the literal before a copy from the byte 9 back, so the matches are these copies exactly."""
    alphabet = list(alphabet)
    lens = [8] * (n // 8) + {0: [], 1: [1], 2: [2], 3: [3], 4: [4], 5: [4, 1], 6: [4, 2], 7: [4, 3]}[n % 8]
    rnd = random.Random(seed)
    out, seen = bytearray(), set()
    for k in lens:
        for _attempt in range(10000):
            piece = bytearray(rnd.choice(alphabet) for _ in range(k))
            if len(out) >= 8 and (piece[0] == out[-8] or piece[-1] == (out + piece)[-9]):
                continue
            new = out[-3:] + piece
            new += (out + piece)[-8:]
            grams = [bytes(new[i:i + 4]) for i in range(len(new) - 3)]
            fresh = grams[:len(grams) - 5]  # those that begin before the copy's first byte
            if len(set(fresh)) == len(fresh) and not any(g in seen for g in fresh):
                out += new[len(new) - k - 8:]
                seen.update(grams)
                break
        else:
            raise AssertionError("no such piece found")
    return bytes(out)


def _fresh(rnd, avoid):
    """a byte that is none of `avoid`"""
    while True:
        b = rnd.randrange(256)
        if b not in avoid:
            return b


def repeat_runs(nruns, seed):
    """Runs copied from a distance that is one of the three last distances used, or the last minus one, or a new one, with 0, 1 or
    2 fresh literals between runs: every way a sequence can name a repeat offset (RFC 8878 3.1.2.5)."""
    rnd = random.Random(seed)
    out = bytearray(rnd.randbytes(600))
    rep = [97, 211, 331]
    for _ in range(nruns):
        ll = rnd.choice([0, 0, 1, 2])
        kind = rnd.randrange(5)
        if kind == 4:
            off = rnd.choice([61, 97, 151, 211, 263, 331, 409, 523])
        elif ll:
            off = rep[kind % 3]
        else:
            off = rep[1] if kind % 3 == 0 else rep[2] if kind % 3 == 1 else max(rep[0] - 1, 40)
        # the literals (and with none, the run's first byte) must end the last run: differ from what its source went on with
        for _i in range(ll):
            out.append(_fresh(rnd, {out[-rep[0]], out[-off]}))
        n = rnd.randrange(8, 40)
        if ll == 0 and out[-off] == out[-rep[0]]:
            out.append(_fresh(rnd, {out[-rep[0]], out[-off]}))
        for _i in range(n):
            out.append(out[-off])
        if off != rep[0]:
            rep = [off, rep[0], rep[2]] if off == rep[1] else [off, rep[0], rep[1]]
    return bytes(out)


def rle_literals(nlit, seed):
    """A first block that ends in stretches of 48 random bytes between zeros (short enough that no setting of the match finder
    steps over any of them), then the same bytes 16 at a time with the byte q in front: the second block's literals are `nlit`
    times q (RLE literals), everything else matches of 16 bytes"""
    rnd = random.Random(seed)
    q = 0xEE
    ts = [bytes(rnd.choice([b for b in range(1, 256) if b != q]) for _ in range(48)) for _ in range((nlit + 2) // 3)]
    body = b"".join(t + b"\0" * 16 for t in ts)
    pieces = [t[i:i + 16] for t in ts for i in (0, 16, 32)][:nlit]
    return b"\0" * (BLOCK - len(body)) + body + b"".join(bytes([q]) + p for p in pieces)


def rle_literals_many(nlit, seed, period=16384, first=64, per=512):
    """A first block that ends in `period` random bytes and a copy of them with 64 bytes turned into q; then further copies, each
    with up to 512 more bytes turned into q, at least 7 apart, that stay q in every later copy.  In the second block every match is
    the repeat offset `period` and every literal the byte q: `nlit` of them (RLE literals)."""
    rnd = random.Random(seed)
    q = 0xEE

    def more(cur, n):
        free = [i for i in range(8, period - 16) if cur[i] != q]
        rnd.shuffle(free)
        taken = set()
        for i in free:
            if len(taken) < n and not any(i + d in taken for d in range(-6, 7)):
                taken.add(i)
        assert len(taken) == n
        return bytearray(q if i in taken else c for i, c in enumerate(cur))

    base = bytearray(rnd.choice([x for x in range(1, 256) if x != q]) for _ in range(period))
    cur = more(base, first)
    out = bytearray(b"\0" * (BLOCK - 2 * period)) + base + cur
    left = nlit
    while left:
        cur = more(cur, min(per, left))
        left -= min(per, left)
        out += cur
    return bytes(out)


def raw_between(seed):
    """A compressed block that ends with matches at the distances 64, 63, 62; a block of random bytes (Raw); a block of 70 fresh
    bytes and a copy from 63 back.  63 is the second repeat offset only if the Raw block left the history alone."""
    rnd = random.Random(seed)
    u = bytes(rnd.sample(range(1, 256), 64))
    x = [b for b in range(1, 256) if b not in u]
    tail = u + u[0:28] + bytes(x[0:1]) + u[30:42] + bytes(x[1:2]) + u[44:56]
    v = bytes(rnd.sample(range(1, 256), 70))
    return b"\0" * (BLOCK - len(tail)) + tail + rnd.randbytes(BLOCK) + v + v[7:47]


def periodic(period, total, seed):
    rnd = random.Random(seed)
    r = rnd.randbytes(period)
    return (r * (total // period + 1))[:total]


def sparse_periodic(period, total, seed):
    """64 random bytes and zeros, repeated: nothing competes with the 64 for their slots of the hash table, so each is found again
    exactly one period on if the table reaches that far"""
    rnd = random.Random(seed)
    r = bytes(rnd.sample(range(1, 256), 64)) + b"\0" * (period - 64)
    return (r * (total // period + 1))[:total]


def ab_run(match, seed=3):
    """40 random bytes, a run of "ab" whose first two bytes are literals and the rest one match of `match` bytes, 30 random bytes"""
    rnd = random.Random(seed)
    run = (b"ab" * (match // 2 + 2))[:match + 2]
    head = rnd.randbytes(39) + b"\x01"
    tail = bytes([_fresh(rnd, {ord("a"), ord("b")})]) + rnd.randbytes(29)
    return head + run + tail


def tail_repeat(n, seed, back=200, extra=20):
    rnd = random.Random(seed)
    r = rnd.randbytes(n)
    return r + r[-back:] + rnd.randbytes(extra)


def permutations(n, seed):
    rnd = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        p = list(range(256))
        rnd.shuffle(p)
        out += bytes(p)
    return bytes(out[:n])


def skewed(nsym, n, seed):
    """n random bytes over 0..nsym-1, low values more often, every value present"""
    rnd = random.Random(seed)
    body = bytes(min(nsym - 1, int(rnd.triangular(0, nsym, 0))) for _ in range(n - nsym))
    return bytes(range(nsym)) + body


# ---- conditions ----------------------------------------------------------------------------------------------------------------------
def _one(info):
    b = cblocks(info)
    assert len(b) == 1 and len(info["blocks"]) == 1, types(info)
    return b[0]


def nseq_is(n, nbytes):
    def cond(info):
        b = _one(info)
        return b["nseq"] == n and b["nseq_bytes"] == nbytes

    return cond


def has_seq(pred):
    return lambda info: any(pred(*s) for s in all_seqs(info))


def types_are(*want):
    return lambda info: types(info) == list(want)


def lit_is(lit_type, regen, header=None, streams=None, size_format=None):
    def cond(info):
        b = cblocks(info)[-1]
        return (b["lit_type"] == lit_type and b["lit_regen"] == regen and (header is None or b["lit_header"] == header)
                and (streams is None or b["streams"] == streams) and (size_format is None or b["size_format"] == size_format))

    return cond


def depth_limited(info):
    return any(b["lit_type"] == "huf" and b["longest_code"] == 11 and huffman_depth(b["literals"]) > 11 for b in cblocks(info))


def tree_is(form, n_weights):
    return lambda info: any(b["lit_type"] == "huf" and b["tree"] == form and b["n_weights"] == n_weights for b in cblocks(info))


def six_repeat_codes(info):
    n = {}
    for _llc, ll, _mlc, _ml, ofv, _off in all_seqs(info):
        if ofv <= 3:
            n[(ofv, ll > 0)] = n.get((ofv, ll > 0), 0) + 1
    return all(n.get((v, pos), 0) >= 3 for v in (1, 2, 3) for pos in (False, True))


def reach(period):
    def cond(info):
        offs = [s[5] for s in all_seqs(info)]
        return all(o <= 65536 for o in offs) and (period > 65536 or period in offs)

    return cond


def header_is(fcs_bytes):
    return lambda info: info["single"] and info["fcs_bytes"] == fcs_bytes


def _raw_between_cond(info):
    if types(info) != ["compressed", "raw", "compressed"]:
        return False
    b1, b3 = info["blocks"][0], info["blocks"][2]
    return b1["offsets"][-3:] == [64, 63, 62] and b3["seqs"][0][1] == 70 and b3["seqs"][0][4] == 2 and b3["offsets"][0] == 63


def _second_block_starts_with_match(info):
    b = info["blocks"]
    first = b[1]["seqs"][0] if len(b) == 2 and b[1].get("seqs") else None
    return types(info) == ["compressed", "compressed"] and b[0]["seqs"] == [(2, 2, 52, 131070, 5)] and first[1] == 0 and first[3] == 200


# ---- the list --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_cases():
    alice = golden("alice29.txt")
    letters13, letters20 = b"etaoinshrdlcu", b"etaoinshrdlcumwfgypb"
    c = []

    def add(name, data, groups, cond):
        assert len(data) <= 400000
        c.append((name, bytes(data), tuple(groups), cond))

    # Number_of_Sequences: 1, 2 and 3 bytes (RFC 8878 3.1.1.3.2.1); every match 4 bytes long, a block that is full of them
    for nwords, nseq, nbytes in ((136, 127, 1), (137, 128, 2), (32520, 0x7EFF, 2), (32521, 0x7F00, 3)):
        add(f"nseq_{nseq}", word_stream(nwords), (0,), nseq_is(nseq, nbytes))
    add("nseq_full_block", word_stream(32768), (0,), nseq_is(32759, 3))
    add("nseq_full_block_other_groups", word_stream(32768), (1, 2, 3), lambda info: _one(info)["regen"] == BLOCK)

    # literal length code 35 (16 extra bits) and the top of code 34
    for n in (65536, 70000, 131060):
        add(f"ll_code35_{n}", tail_repeat(n, n), (1, 2, 3), has_seq(lambda llc, ll, mlc, ml, ofv, off, n=n: llc == 35 and ll == n))
    # in group 0 the walk steps over 200 bytes by then: a longer copy, found at skip_shift 8
    add("ll_code35_group0", tail_repeat(70000, 70000, back=8000), ((0, 8),),
        has_seq(lambda llc, ll, mlc, ml, ofv, off: llc == 35 and ll == 70000))
    add("ll_code34_top", tail_repeat(65535, 5), (1, 2, 3), has_seq(lambda llc, ll, mlc, ml, ofv, off: llc == 34 and ll == 65535))

    # match length codes 51 (top) and 52
    add("ml_code51_top", ab_run(65538), ALL, has_seq(lambda llc, ll, mlc, ml, ofv, off: mlc == 51 and ml == 65538))
    add("ml_code52_bottom", ab_run(65539), ALL, has_seq(lambda llc, ll, mlc, ml, ofv, off: mlc == 52 and ml == 65539))
    add("ml_full_block", b"ab" * 65536, ALL, lambda info: _one(info)["seqs"] == [(2, 2, 52, 131070, 5)])
    add("ml_full_block_and_more", b"ab" * 65536 + b"ab" * 100, ALL, _second_block_starts_with_match)

    # block types at the block edge
    for n, want in ((131071, ["rle"]), (131072, ["rle"]), (131073, ["rle", "raw"]), (262145, ["rle", "rle", "raw"])):
        add(f"zeros_{n}", b"\0" * n, ALL, types_are(*want))
    for n, want in ((131071, ["compressed"]), (131072, ["rle", "raw"]), (131073, ["rle", "raw"]), (262145, ["rle", "rle", "raw"])):
        add(f"zeros_{n}_one", b"\0" * n + b"\1", ALL, types_are(*want))
    for n, want in ((131071, ["compressed"]), (131072, ["compressed", "raw"]), (131073, ["compressed", "rle"]),
                    (262145, ["compressed", "rle", "rle"])):
        add(f"one_zeros_{n}", b"\1" + b"\0" * n, ALL, types_are(*want))
    # 256 equal counts: one weight for all, which no tree description can hold, so the block is Raw
    add("permutations_8192", permutations(8192, 1), ALL, types_are("raw"))
    add("permutations_block", permutations(BLOCK, 2), ALL, types_are("raw"))
    p = permutations(8192, 1)
    add("permutations_8192_and_copy", p + p[-1000:-700], (1, 2, 3), lambda info: _one(info)["lit_type"] == "raw")
    p = permutations(512, 3)
    add("permutations_512_and_copy", p + p[-400:-100], ALL, lambda info: _one(info)["lit_type"] == "raw")
    p = permutations(BLOCK - 300, 2)
    add("permutations_block_and_copy", p + p[-1000:-700], (1, 2, 3), lambda info: _one(info)["lit_type"] == "raw")

    # Huffman code lengths limited to 11 bits
    rnd = random.Random(11)
    add("depth_expo", bytes(min(255, 100 + int(rnd.expovariate(0.05))) for _ in range(6000)), ALL, depth_limited)
    add("depth_alice", alice[:BLOCK], ALL, depth_limited)

    # the tree description: 128 weights is the most the direct form holds
    add("weights_128_direct", skewed(129, 3000, 1), ALL, tree_is("direct", 128))
    add("weights_129_fse", skewed(130, 3000, 2), ALL, tree_is("fse", 129))
    add("weights_130_fse", skewed(131, 3000, 3), ALL, tree_is("fse", 130))

    # literals section: Raw with a header of 1, 2 and 3 bytes
    for n, hdr in ((31, 1), (32, 2), (4095, 2), (4096, 3)):
        add(f"lit_raw_{n}", doubled(n, range(256), n), (1, 2, 3), lit_is("raw", n, header=hdr))
        add(f"lit_raw_{n}_chunked", chunked(n, range(256), 1), ALL, lit_is("raw", n, header=hdr))
    # RLE literals with a header of 1 and 2 bytes
    for n, hdr in ((31, 1), (32, 2)):
        add(f"lit_rle_{n}", rle_literals(n, 1), ALL, lit_is("rle", n, header=hdr))
    # ... and of 3 bytes: 4096 equal literals, which only the lazy groups' repeat-offset matches leave alone
    for n, hdr in ((4095, 2), (4096, 3)):
        add(f"lit_rle_{n}", rle_literals_many(n, 1), (2, 3), lit_is("rle", n, header=hdr))
    # the Huffman stage starts at 16 literals
    add("lit_15", doubled(15, b"\0\1\2", 1), ALL, lit_is("raw", 15))
    add("lit_16", doubled(16, b"\0\1\2", 1), ALL, lit_is("huf", 16, streams=1))
    add("lit_15_chunked", chunked(15, b"\0\1\2\3", 1), ALL, lit_is("raw", 15))
    add("lit_16_chunked", chunked(16, b"\0\1\2\3", 1), ALL, lit_is("huf", 16, streams=1))
    # one stream up to 1023 literals, four with 14-bit sizes up to 16383, then 18-bit sizes; every remainder of n / 4
    for n, streams, sf in ((1023, 1, 0), (1024, 4, 2), (1025, 4, 2), (1026, 4, 2), (1027, 4, 2), (16383, 4, 2), (16384, 4, 3)):
        add(f"lit_{n}", doubled(n, letters13, n), (1, 2, 3), lit_is("huf", n, streams=streams, size_format=sf))
        add(f"lit_{n}_chunked", chunked(n, letters20, 2), ALL, lit_is("huf", n, streams=streams, size_format=sf))

    # repeat offsets
    add("repeat_codes", repeat_runs(3000, 1), ALL, six_repeat_codes)
    add("raw_block_between_repeat_codes", raw_between(1), ALL, _raw_between_cond)

    # the 64 KiB the hash table reaches back
    for period in (65535, 65536, 65537, 32768):
        add(f"period_{period}", periodic(period, 200000, period), (1, 2), reach(period))
        add(f"sparse_period_{period}", sparse_periodic(period, 200000, period), ALL, reach(period))

    # inputs around the 8 bytes the match finder looks ahead
    for n in (0, 1, 7, 8, 9):
        add(f"tiny_{n}", (b"abcd" * 4)[:n], ALL, types_are("raw"))
    for n in (12, 15):
        add(f"tiny_{n}", (b"abcd" * 4)[:n], ALL, lambda info, n=n: _one(info)["seqs"] == [(4, 4, n - 4 - 3, n - 4, 2)])

    # Frame_Content_Size of 1, 2 and 4 bytes
    for n, fb in ((255, 1), (256, 2), (65791, 2), (65792, 4)):
        add(f"fcs_{n}", alice[:n], ALL, header_is(fb))
    return c


# ---- streaming ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_scripts():
    """[(name, script)]: calls (piece, op) of the streaming encoder, op one of zstd_enc_host.PROCESS / FLUSH / FINISH; the caller's
    room is ample, so zstd_enc_host.segments_of(script) says which segments the encoder compresses"""
    from zstd_enc_host import FINISH, FLUSH, PROCESS, SEGMENT

    alice = golden("alice29.txt")
    runs = repeat_runs(400, 2)
    cut = len(runs) // 2 + 3
    return [
        # segments of 1 byte and of none among ordinary ones; a Flush with nothing new writes nothing
        ("flushes", [(alice[:5000], PROCESS), (b"", FLUSH), (b"", FLUSH), (alice[5000:5001], FLUSH), (alice[5001:9000], FLUSH), (b"", FINISH)]),
        ("first_flush_is_empty", [(b"", FLUSH), (alice[:100], FINISH)]),
        # the repeat offsets go on across the cut, the matches do not
        ("cut_inside_repeat_runs", [(runs[:cut], FLUSH), (runs[cut:], FINISH)]),
        ("segments_of_several_blocks", [(alice[:140000], FLUSH), ((alice * 2)[:300000], FLUSH), (b"", FINISH)]),
        # one call that crosses the 1 MiB at which buffered input becomes a segment
        ("crosses_the_segment_cut", [((alice * 8)[:SEGMENT + 5000], FINISH)]),
        ("exactly_one_segment_then_process", [((alice * 7)[:SEGMENT], PROCESS), (alice[:10], FINISH)]),
        ("nothing_new_to_flush_or_finish", [(alice[:3000], PROCESS), (b"", FLUSH), (b"", FINISH)]),
        # the first segment is the last: a one-shot frame (single-segment header if it fits the window)
        ("finish_only", [(alice[:20000], FINISH)]),
        ("finish_only_small", [(alice[:700], FINISH)]),
        ("finish_only_empty", [(b"", FINISH)]),
    ]
