"""A model of the slab protocol of chip_inflate_parallel_next (include/compu_hip.h) over the small inflate and
the finder of tests/inflate_parallel_ref.py: given a stream, the bit of its first block, chunk_bytes, a slab size and the room, the
calls a caller makes who always presents the next `slab` bytes from where the last call ended.  Shared by
tests/test_inflate_stream_cpu.py and tests/test_inflate_stream_gpu.py."""
import inflate_parallel_ref as R

SERIAL, PARALLEL = 0, 1
NEED_INPUT, NEED_OUTPUT, FINISHED = 0, 1, 2
PASS_MAX = 8  # CHIP_PAR_PASS_MAX


class Call:
    """one call: the stream byte its slab begins at, the slab's length, the cursor's bit in the slab, the finder's starts (bits of the
    slab), the path, where it ends (a bit of the STREAM), the bytes it delivers and its status"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "Call(" + ", ".join(f"{k}={v}" for k, v in self.__dict__.items() if k != "starts") + f", n_starts={len(self.starts)})"


def boundaries(data, first_bit, trailer):
    """([bit of every block boundary of the stream, and behind them the bit of the byte behind the final block], {bit: content bytes
    in front of it}, content).  The end is known to the byte: the trailer's first."""
    bounds, content = R.walk_cached(data, first_bit)
    end = 8 * (len(data) - trailer)
    out_at = {b: o for b, o, _, _ in bounds}
    out_at[end] = len(content)
    return [b for b, _, _, _ in bounds] + [end], out_at, content


def calls(data, first_bit, chunk_bytes, slab, room=1 << 40, trailer=0, find=R.find_starts):
    """The calls of a decode of `data` whose first block header is at first_bit (what stands in front is the wrapper) and whose
    last `trailer` bytes are the trailer.  A call is PARALLEL iff its slab has at least one start that the chain from the cursor
    reaches (a wave that walks over more than PASS_MAX starts gives up); it delivers the chain members that ended at a start or in
    the final block, while they fit the room.  Otherwise one wave advances to the last boundary inside slab and room.  A call
    that cannot move doubles the slab (a slab that holds the rest of the stream cannot grow: the model stops)."""
    bits, out_at, content = boundaries(data, first_bit, trailer)
    end = bits[-1]
    out, pos, cur = [], 0, first_bit  # pos: the stream byte the slab begins at; cur: the cursor, a bit of the stream
    header = True
    while True:
        piece = data[pos:pos + slab]
        if header and len(piece) < (first_bit >> 3):
            out.append(Call(pos=pos, slab=len(piece), bit=0, starts=[], path=SERIAL, end=0, out_len=0, status=NEED_INPUT, links=0))
            assert pos + slab < len(data), "the stream ends inside its header"
            slab *= 2
            continue
        header = False
        fb, lim = cur - 8 * pos, 8 * len(piece)
        starts = find(piece, fb, chunk_bytes) if len(piece) > chunk_bytes else []
        inside = [b - 8 * pos for b in bits if cur <= b and b - 8 * pos <= lim]  # the boundaries the slab holds, the cursor first
        sset = set(starts)
        # the chain: members [(first, last)] in bits of the slab.  At every boundary behind its first a wave asks, in this order: the
        # final block's end?  a start?  more than PASS_MAX starts walked over?
        members, at, finished = [], fb, False
        while True:
            link = None
            for b in (b for b in inside if b > at):
                if b + 8 * pos == end:
                    finished = True
                    members.append((at, b))
                    break
                if b in sset:
                    link = b
                    break
                if sum(1 for s in starts if at < s < b) > PASS_MAX:
                    break
            if link is None:
                break
            members.append((at, link))
            at = link
        links = len(members) - (1 if finished else 0)
        size = lambda m: out_at[m[1] + 8 * pos] - out_at[m[0] + 8 * pos]  # noqa: E731
        if members and not (finished and len(members) == 1):
            path, given, n = PARALLEL, 0, 0
            while n < len(members) and given + size(members[n]) <= room:
                given += size(members[n])
                n += 1
            stop = members[n - 1][1] if n else fb
            status = NEED_OUTPUT if n < len(members) else NEED_INPUT
            done = finished and n == len(members)
        else:
            path = SERIAL
            ok = [b for b in inside if out_at[b + 8 * pos] - out_at[cur] <= room]
            stop = ok[-1] if ok else fb
            done = stop + 8 * pos == end
            status = NEED_INPUT if len(ok) == len(inside) else NEED_OUTPUT
            links = 0
        new = stop + 8 * pos
        used = (new + 7) >> 3 if done else new >> 3
        if done and pos + len(piece) - used >= trailer:
            status, used = FINISHED, used + trailer
        elif done:
            status = NEED_INPUT
        out.append(Call(pos=pos, slab=len(piece), bit=fb, starts=starts, path=path, end=new, out_len=out_at[new] - out_at[cur], status=status,
                        links=links))
        if status == FINISHED:
            return out, content
        if done:  # the trailer alone is left
            assert pos + slab < len(data) or used > pos, "the stream ends inside its trailer"
            pos, cur = used, 8 * used
            out.append(Call(pos=pos, slab=len(data[pos:pos + slab]), bit=0, starts=[], path=SERIAL, end=8 * used, out_len=0, status=FINISHED, links=0))
            assert len(data) - pos >= trailer
            return out, content
        if new == cur and used == pos:
            assert pos + slab < len(data) and status == NEED_INPUT, "the model cannot move"
            slab *= 2
            continue
        pos, cur = used, new
