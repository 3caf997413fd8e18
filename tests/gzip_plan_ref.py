"""The walk that defines chip_gzip_plan (include/compu_hip.h), in Python: the rows and the summary of a buffer, given `size1` -- what
chip_decode_batch_sizes(CHIP_FMT_GZIP, flags 0) answers for the unit in[p .. p + room): (status, out_size, in_used).

size1 defaults to the CPU oracle's InflateDecoder(31) over the case's TWIN (the file with its wrong CRC-32s repaired), read as
members_ref.oracle_decode1 reads it: the size pass makes every check but the CRC comparison, and this is how that rule enters
without guessing.  A GPU test passes the size pass itself and thereby checks the contract to the letter.  Shared by
tests/test_gzip_plan_cpu.py and tests/test_gzip_plan_gpu.py."""
import functools

import gzip_plan_cases as G
import members_ref as M

WINDOW = (1 << 29) - 64  # CHIP_GZPLAN_WINDOW
AMPLE = 1 << 22          # room for the largest member of gzip_plan_cases.all_cases()


def oracle_size1(twin):
    decode1 = M.oracle_decode1(M.GZIP)

    def size1(p, room):
        st, got, iu = decode1(twin[p:p + room], AMPLE)
        assert st != M.NEED_OUTPUT
        return st, len(got), len(twin[p:p + room]) if st == M.NEED_INPUT else iu

    return size1


def walk(data, size1):
    """(rows, summary): rows = [(in_off, in_len, out_off, out_cap)], summary = (n_members, total_out, in_used, status,
    member_status).  `data` decides the header test; size1 decides the rest."""
    length = len(data)
    p, total, rows = 0, 0, []

    def stop(status, member_status=0):
        return rows, (len(rows), total, p, status, member_status)

    while True:
        if p == length:
            return stop(G.OK)
        if length - p < 4:
            return stop(G.TRUNCATED)
        if data[p:p + 3] != b"\x1f\x8b\x08" or data[p + 3] & 0xE0:
            return stop(G.BAD_HEADER)
        room = min(length - p, WINDOW)
        st, size, iu = size1(p, room)
        if st == M.NEED_INPUT:
            return stop(G.TOO_LARGE if room < length - p else G.TRUNCATED)
        if st != M.FINISHED:
            return stop(G.BAD_MEMBER, st)
        if size > 0xFFFFFFFE:
            return stop(G.TOO_LARGE)
        rows.append((p, iu, total, size))
        total += size
        p += iu


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference plan of a case of gzip_plan_cases.all_cases(), computed once"""
    c = G.by_name(name)
    return walk(c.twin, oracle_size1(c.twin))
