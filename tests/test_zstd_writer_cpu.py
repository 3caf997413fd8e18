"""Hand-built zstd frames (tests/zstd_cases.py) on the CPU: the system libzstd checks the writer, and the oracle
(oracle/oracle_zstd.c) must give every case its expected bytes or verdict, in one call and in pieces.  No GPU needed."""
import pytest

import zstd_cases as K
import zstd_ref
from oracle import oracle as O

Z = zstd_ref.load()
needs_libzstd = pytest.mark.skipif(Z is None, reason="no system libzstd to cross-check against")
# cases on which libzstd 1.4.x gives another verdict than RFC 8878 (and the decoders here): each carries its reason
LAX = 9


@pytest.fixture(scope="module")
def cases():
    return K.all_cases()


def _result(calls):
    """-> the content, or the error code, at the end of a run of calls"""
    st, err = calls[-1][0], calls[-1][1]
    if st is None:
        return err
    return b"".join(c[2] for c in calls) if st == 2 else ("status", st)


def _oracle_call(d):
    def call(chunk, room):
        got, ir, orr, st, err = d.decode(chunk, room)
        return (None if err else st), err, got, ir, orr
    return call


def _room(c):
    return (len(c.want) if isinstance(c.want, bytes) else 1 << 18) + 64


@needs_libzstd
def test_libzstd_decodes_every_case_to_the_writers_content(cases):
    lax = []
    for c in cases:
        got = _result(zstd_ref.stream_calls(Z, c.frame, [], _room(c)))
        if c.lax:
            assert got != c.want, (c.name, "no longer laxer: drop the mark")
            lax.append(c.name)
            continue
        assert got == c.want, (c.name, got if not isinstance(got, bytes) else len(got))
    assert len(lax) == LAX, lax


@needs_libzstd
def test_libzstd_agrees_in_pieces_where_its_single_pass_differs(cases):
    """the FCS cases marked lax: cut at the blocks, libzstd takes its buffered path and gives the verdict the decoders here give"""
    for c in cases:
        if c.lax and "single pass" in c.lax:
            assert _result(zstd_ref.stream_calls(Z, c.frame, c.cuts, _room(c))) == c.want, c.name


def test_oracle_gives_every_case_its_result(cases):
    for c in cases:
        for cuts, room in (([], _room(c)), (c.cuts, _room(c)), (c.cuts, 4096), ([], 13)):
            got = _result(zstd_ref.drive(_oracle_call(O.ZstdDecoder()), c.frame, cuts, room))
            assert got == c.want, (c.name, len(cuts), room, got if not isinstance(got, bytes) else len(got))


def test_oracle_in_small_pieces(cases):
    for c in cases:
        if len(c.frame) > 4096:
            continue
        for piece, room in ((1, 1 << 20), (7, 13)):
            got = _result(zstd_ref.drive(_oracle_call(O.ZstdDecoder()), c.frame, range(piece, len(c.frame), piece), room))
            assert got == c.want, (c.name, piece, room)


@needs_libzstd
def test_oracle_calls_are_libzstds_where_it_holds_all_input(cases):
    """every call's (status, err, bytes, output_remain) against libzstd's, and input_remain on all but NeedOutput calls (there
    libzstd keeps the input of a block it cannot flush yet, test_oracle_zstd.py), with the output room that a call never fills"""
    for c in cases:
        if c.lax or "bad_nseq" in c.tags:  # (libzstd 1.4 executes the over-read extra sequence in its buffered path: -70)
            continue
        for cuts in ([], c.cuts):
            a = zstd_ref.stream_calls(Z, c.frame, cuts, _room(c))
            b = zstd_ref.drive(_oracle_call(O.ZstdDecoder()), c.frame, cuts, _room(c))
            assert len(a) == len(b), (c.name, len(cuts), a[-1][:2], b[-1][:2])
            for x, y in zip(a, b):
                assert x[:3] == y[:3] and x[4] == y[4] and (x[0] == 1 or x[3] == y[3]), (c.name, len(cuts), x[:2], x[3:], y[:2], y[3:])


def test_every_feature_is_reached(cases):
    """the declared feature matrix (zstd_cases.FEATURES): pruning a case later must fail here"""
    tags = set().union(*(c.tags for c in cases))
    assert tags - K.FEATURES == set(), "tags outside the matrix (a typo?)"
    assert K.FEATURES - tags == set(), "features no case reaches"
    names = [c.name for c in cases]
    assert len(names) == len(set(names))


def test_writer_round_trip_basics():
    """the writer's own pieces: the backward bitstream closes with a 1 bit, the FSE encoder walks back through the decoding
    table, the canonical Huffman codes are the decoding table's"""
    import zstd_writer as W

    assert W.back_stream([]) == b"\x01" and W.back_stream([(5, 3)]) == bytes([0b1101])
    t = W.Fse(W.LL_DEF, 6)
    for s in range(36):
        u = t.state_for(s)
        assert t.sym[u] == s
        for nxt in range(64):
            v = t.state_for(s, nxt)
            assert t.base[v] <= nxt < t.base[v] + (1 << t.nb[v])
    h = W.Huf(W.weights_of_lengths({0: 1, 1: 2, 2: 3, 3: 3}))
    assert h.codes == {2: (0, 3), 3: (1, 3), 1: (1, 2), 0: (1, 1)}
