"""What chip_decode_batch_sizes must answer for the hand-built DEFLATE cases (tests/deflate_cases.py) and zstd frames
(tests/zstd_cases.py), derived from the oracle and from the one rule that sets the size pass apart from a decode: it makes every check
except those that need decoded bytes (deflate: Adler-32 / CRC-32, zlib's "incorrect data check"; zstd: the contents of Huffman-coded
literal streams and the XXH64 comparison).  Shared by tests/test_sizes_cpu.py, which pins the exception list
without a GPU, and tests/test_sizes_gpu.py."""
import deflate_cases as K
from oracle import oracle as O

FINISHED, NEED_INPUT, NEED_DICT = 2, 0, 3
DATA_CHECK = "incorrect data check"
# the cases the rule exempts -- named here, and test_sizes_cpu asserts the rule produces exactly these
DEFLATE_EXCEPTIONS = frozenset({"zlib_adler", "gzip_crc"})


def oracle_triple(c):
    """(status, decoded length, input consumed) of the oracle with room for everything (len(content) + 64, as
    test_inflate_hand_gpu._ref_len); Z_NEED_DICT reads as the batch status CHIP_NEED_DICT"""
    got, ir, _orr, st, err = O.InflateDecoder(K.MODES[c.fmt]).decode(c.data, len(c.content) + 64)
    status = err if err else st
    if status == 2 and c.want == K.Err(2, None):
        status = NEED_DICT
    return status, len(got), len(c.data) - ir


def by_rule_exempt(c):
    """the fault lies in the check value alone: the oracle says -3 and the case's message is zlib's for that check"""
    return isinstance(c.want, K.Err) and c.want.msg == DATA_CHECK


def expected(c):
    """(status, size, in_used or None): in_used is pinned by the oracle only on CHIP_FINISHED (elsewhere the yardstick is the
    unchanged decode path)"""
    status, size, used = oracle_triple(c)
    if by_rule_exempt(c):
        assert status == -3 and size == len(c.content), c.name
        return FINISHED, len(c.content), len(c.data) - c.tail
    return status, size, used if status == FINISHED else None


# ---- zstd: a case is exempt when its fault lies in the CONTENT of a Huffman literal stream (too many / too few bits for the stated
# regenerated size: the stream's stated sizes are consistent, only decoding it shows the fault) or in the checksum value
ZSTD_CONTENT_TAGS = frozenset({"checksum_wrong", "bad_huf_leftover", "bad_huf_overread", "bad_huf_size"})
ZSTD_EXCEPTIONS = frozenset({"checksum_wrong", "huf_regen_short", "lit_extra_5_1s", "lit_extra_5_4s", "lit_drop_2_1s", "lit_drop_2_4s"})
ZSTD_ERR_CAP = 1 << 18  # ample room for the cases that end in an error (tests/test_zstd_hand_gpu.py)


def zstd_exempt(c):
    return bool(c.tags & ZSTD_CONTENT_TAGS) and not isinstance(c.want, bytes)


def zstd_expected(c):
    """(status, size, in_used or None) of the oracle with ample room; None for the exempt cases (the fault is one the pass cannot see: it
    reads CHIP_FINISHED and the decode that follows reports it, unless Frame_Content_Size gives the fault away)"""
    if zstd_exempt(c):
        return None
    cap = (len(c.want) if isinstance(c.want, bytes) else ZSTD_ERR_CAP) + 4096
    got, ir, _orr, st, err = O.ZstdDecoder().decode(c.frame, cap)
    status = err if err else st
    return status, len(got), (len(c.frame) - ir) if status == FINISHED else None
