"""The definition of "reading ranges" (include/compu_hip.h) restated in plain Python: lists, bisect, unbounded integers.  What
chip_select_units_host, chip_select_units and chip_read_ranges are compared with.  Shared range sets live here too."""
import bisect
import random

OK, OUTSIDE, BAD_UNIT = 0, 1, 2  # CHIP_RANGE_*
READ_OK, READ_NEED_OUTPUT, READ_BAD_LAYOUT = 0, 1, 2  # CHIP_READ_*
UNSIZED = 0xFFFFFFFF  # CHIP_ZPLAN_UNSIZED
U64 = 1 << 64


class Selection:
    """Every array and the summary of one answer; on BAD_LAYOUT the arrays are empty and only bad_index is set."""

    def __init__(self):
        self.sel_unit, self.sel_in_off, self.sel_in_len, self.sel_out_off, self.sel_out_cap = [], [], [], [], []
        self.src_off, self.dst_off, self.status = [], [], []
        self.first, self.last = [], []  # per range: the span of units, None where it touches none
        self.n_sel = self.scratch_bytes = self.out_len = self.n_outside = self.bad_index = 0
        self.read_status = READ_OK

    def summary(self):
        return (self.n_sel, self.scratch_bytes, self.out_len, self.n_outside, self.bad_index, self.read_status)


def select(in_off, in_len, out_off, out_cap, ranges):
    """ranges: (lo, len) pairs"""
    s = Selection()
    n = len(out_cap)
    if not ranges:
        return s
    for i in range(n):
        end_i = out_off[i] + out_cap[i]
        if out_cap[i] == UNSIZED or end_i >= U64 or (i + 1 < n and out_off[i + 1] != end_i):
            s.read_status, s.bad_index = READ_BAD_LAYOUT, i + 1
            return s
    begin, end = (out_off[0], out_off[-1] + out_cap[-1]) if n else (0, 0)
    cover = [0] * (n + 1)
    for lo, ln in ranges:
        s.dst_off.append(s.out_len)
        if ln == 0:
            s.status.append(OK)
            s.first.append(None), s.last.append(None)
        elif lo < begin or lo + ln > end:
            s.status.append(OUTSIDE)
            s.first.append(None), s.last.append(None)
            s.n_outside += 1
        else:
            s.status.append(OK)
            f, l = bisect.bisect_right(out_off, lo) - 1, bisect.bisect_right(out_off, lo + ln - 1) - 1
            s.first.append(f), s.last.append(l)
            for u in range(f, l + 1):  # (plain, not clever: the reference)
                cover[u] += 1
            s.out_len += ln
    image = [0] * n  # per unit: the selected bytes in front of it
    for u in range(n):
        image[u] = s.scratch_bytes
        if cover[u] and out_cap[u] > 0:
            s.sel_unit.append(u), s.sel_in_off.append(in_off[u]), s.sel_in_len.append(in_len[u])
            s.sel_out_off.append(s.scratch_bytes), s.sel_out_cap.append(out_cap[u])
            s.scratch_bytes += out_cap[u]
    s.n_sel = len(s.sel_unit)
    for (lo, ln), f in zip(ranges, s.first):
        s.src_off.append(0 if f is None else image[f] + lo - out_off[f])
    return s


def layout(caps, begin=0, seed=0):
    """(in_off, in_len, out_off, out_cap) of a chained layout with the given caps; the input side is made up"""
    rng = random.Random(seed)
    in_off, in_len, out_off, p, q = [], [], [], 0, begin
    for c in caps:
        ln = rng.randrange(18, 400)
        in_off.append(p), in_len.append(ln), out_off.append(q)
        p, q = p + ln, q + c
    return in_off, in_len, out_off, list(caps)


def boundary_ranges(out_off, out_cap):
    """The boundary set: unit boundaries, first and last byte, one byte, everything, empty units, duplicates, nesting, overlap in
    descending order, len 0 and len 1 at the end, no wrap at 2^64 - 1, in front of the content."""
    n = len(out_cap)
    begin, end = out_off[0], out_off[-1] + out_cap[-1]
    full = [u for u in range(n) if out_cap[u] > 0]
    empty = [u for u in range(n) if out_cap[u] == 0]
    a, b, c = full[0], full[len(full) // 2], full[-1]
    r = [(out_off[b], out_cap[b]),                              # exactly one unit, boundary to boundary
         (out_off[a], out_off[b] + out_cap[b] - out_off[a]),    # boundary to boundary over many units
         (begin, 1), (end - 1, 1),                              # the first and the last byte
         (out_off[b] + out_cap[b] - 1, 1), (out_off[b] + out_cap[b] - 1, 2),  # the last byte of a unit; across the boundary
         (begin, min(end - begin, 0xFFFFFFFF)),                 # the whole content
         (end, 0), (end, 1),                                    # OK and OUTSIDE at the end
         (U64 - 1, 2), (U64 - 1, 0), (U64 - 1, 1),              # no wrap
         (end - 1, 2), (end + 5, 0), (end + 5, 3)]
    if begin > 0:
        r += [(begin - 1, 1), (begin - 1, 2), (0, 1)]           # in front of the content
    for u in empty:
        if out_off[u] < end:
            r += [(out_off[u], 1)]                              # starts at the position of an empty unit
        if begin < out_off[u] < end:
            r += [(out_off[u] - 1, 2)]                          # spans it
        r += [(out_off[u], 0)]
    third = (end - begin) // 3
    r += [(begin + third, third), (begin + third, third),       # duplicated
          (begin + third + 7, 11),                              # nested
          (begin + 2 * third - 5, 40), (begin + third - 20, 40), (begin + 3, 40)]  # overlapping, descending
    return [(lo, ln) for lo, ln in r if ln <= 0xFFFFFFFF]


def random_ranges(rng, begin, end, count, max_len=300, stray=0.05):
    """`count` seeded ranges inside [begin, end) for the most part; a share `stray` is empty, pokes out behind the end or lies
    behind it"""
    out = []
    for _ in range(count):
        if end == begin or rng.random() < stray:
            kind = rng.randrange(3)
            if kind == 0:
                out.append((rng.randrange(begin, end + 1), 0))
            elif kind == 1:
                out.append((max(end - rng.randrange(0, 4), 0), rng.randrange(4, max_len)))
            else:
                out.append((end + rng.randrange(0, 1000), rng.randrange(1, max_len)))
        else:
            lo = rng.randrange(begin, end)
            out.append((lo, rng.randrange(1, min(max_len, end - lo) + 1)))
    return out
