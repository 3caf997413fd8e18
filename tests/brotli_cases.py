"""Hand-built brotli streams (tests/brotli_writer.py): (name, stream, output it stands for)."""
import random

import brotli_writer as W


def many_trees():
    """256 literal, 256 insert-and-copy and 256 distance trees in one metablock, with block switches in all three categories: the
    literal tables alone take 256 x 256 entries (128 KiB), more than the kernel's first-pass slot, so the unit is decoded by the
    second launch"""
    rnd = random.Random(1)
    s = W.Stream(16)
    ncmd = 600
    cmds = []
    for i in range(ncmd):
        lits = bytes(rnd.randrange(97, 123) for _ in range(rnd.randrange(1, 6)))
        cmds.append((lits, ("dist", rnd.randrange(1, 4), rnd.randrange(2, 9)) if i else None) if i < ncmd - 1 else (lits, None))
    cmds[0] = (b"abcdefgh", ("dist", 3, 4))
    nlit = sum(len(l) for l, _ in cmds)
    lblocks = [(k % 4, 5) for k in range(nlit // 5 + 2)]
    iblocks = [(k % 256, 1) for k in range(ncmd)]
    ndist = sum(1 for _, c in cmds if c)
    dblocks = [(k % 64, 2) for k in range(ndist // 2 + 2)]
    s.compressed(cmds, islast=True, nbl=(4, 256, 64), blocks=(lblocks, iblocks, dblocks), lmap=list(range(256)), ntl=256,
                 dmap=list(range(256)), ntd=256)
    return s.finish()


def distances(npostfix, ndirect, seed):
    rnd = random.Random(seed)
    s = W.Stream(18)
    cmds = [(bytes(rnd.randrange(256) for _ in range(3000)), ("dist", 2500, 10))]
    s.compressed(cmds, nbl=(1, 1, 1), npostfix=npostfix, ndirect=ndirect)
    cmds = []
    for i in range(300):
        lits = bytes(rnd.randrange(256) for _ in range(rnd.randrange(0, 4)))
        kind = rnd.randrange(4)
        if kind == 0 and ndirect:
            c = ("dist", rnd.randrange(1, ndirect + 1), rnd.randrange(2, 30))
        elif kind == 1:
            c = ("code", rnd.randrange(0, 4), rnd.randrange(2, 30))
        elif kind == 2:
            c = ("last", rnd.randrange(2, 12))
        else:
            c = ("dist", rnd.randrange(1, 3000), rnd.randrange(2, 300))
        cmds.append((lits, c))
    cmds.append((b"z", None))
    s.compressed(cmds, islast=True, nbl=(2, 3, 2), blocks=([(0, 100), (1, 5000)], [(0, 50), (2, 40), (1, 400)], [(0, 30), (1, 1000)]),
                 npostfix=npostfix, ndirect=ndirect, modes=[0, 0], lmap=[0] * 64 + [1] * 64, ntl=2, dmap=[0, 1, 0, 1, 1, 1, 1, 0], ntd=2)
    return s.finish()


def transforms(clen_seed):
    """every transform id on dictionary words of several lengths"""
    rnd = random.Random(clen_seed)
    s = W.Stream(16)
    s.compressed([(b"Lorem ipsum ", ("dist", 6, 6))], nbl=(1, 1, 1))
    cmds = []
    pos = len(s.out)
    for tidx in range(121):
        clen = rnd.randrange(4, 25)
        widx = rnd.randrange(1 << W.NDBITS[clen])
        max_dist = min(pos, (1 << 16) - 16)
        cmds.append((b"", ("dist", max_dist + 1 + (tidx << W.NDBITS[clen]) + widx, clen)))
        word = W.dictionary()[W.DICT_OFFSET[clen] + widx * clen:][:clen]
        pos += len(W.transform(word, tidx))
    cmds.append((b".", None))
    s.compressed(cmds, islast=True)
    return s.finish()


def metadata_and_empty():
    s = W.Stream(20)
    s.metadata(b"")
    s.metadata(b"skipped bytes")
    s.uncompressed(b"stored metablock ")
    s.metadata(bytes(300))
    s.compressed([(b"then compressed ", ("dist", 17, 6)), (b"!", None)])
    s.last_empty()
    return s.finish()


def all_cases():
    out = [("many_trees",) + many_trees()]
    for k, (p, d) in enumerate([(3, 120), (0, 0), (3, 0), (1, 30), (2, 60), (0, 15)]):
        out.append((f"npostfix{p}_ndirect{d}",) + distances(p, d, k))
    for seed in range(3):
        out.append((f"transforms{seed}",) + transforms(seed))
    out.append(("metadata_and_empty",) + metadata_and_empty())
    return out
