"""The hand-built brotli streams of tests/brotli_form_cases.py against libbrotlidec on the CPU: every valid stream decodes to
exactly what the writer says it stands for, every error stream gives the error it is named for, and the forms the writer recorded
cover the table below -- so the GPU tests over the same cases (test_brotli_forms_gpu.py) cannot silently lose a form."""
import hashlib

import pytest

import brotli_cases as K
import brotli_form_cases as F
import brotli_ref as B
import brotli_writer as W

CATS = ["lit", "ic", "dist"]
MAPS = ["lmap", "dmap", "lmapN"]  # literal map of one block type, distance map, literal map of several block types

# every form the case list has to contain, as the writer's tags
REQUIRED = (
    ["wbits%d" % n for n in range(10, 25)]
    + ["mlen_nib4", "mlen_nib5", "mlen_nib6", "uncompressed", "mskip0", "mskip1", "mskip2", "mskip3", "meta_last", "last_empty_midbyte"]
    + ["simple%s_%s" % (f, a) for f in ("2", "3", "4", "4t") for a in ("lit", "ic", "dist", "bt", "bl", "cmap")] + ["simple_desc"]
    + ["hskip0", "hskip2", "hskip3", "cl_single_len8", "cl_single_len7", "rep16_first", "rep16_chain2", "rep16_chain3", "rep17_chain",
       "rep17_ge64", "rep17_ge138", "rep16_after17", "rep17_after16", "depth15", "subtable_widths3", "complex_lit", "complex_ic"]
    + ["mode_%s" % m for m in W.MODE_NAMES] + ["mode_%s_ctx64" % m for m in ("msb6", "utf8", "signed")] + ["mode_switch", "ctx_from_stored"]
    + ["mode_%s_not_%s" % (m, o) for m in W.MODE_NAMES for o in W.MODE_NAMES if m != o]
    + ["%s_%s" % (f, m) for f in ("rlemax1", "rlemax16", "cm_run_to_end", "imtf", "rle_imtf", "tree255") for m in MAPS]
    + ["%s_%s" % (f, c) for f in ("bt_code0_first", "bt_code1_wrap", "bt_code0_twice", "bt_code0", "bt_code1", "bt_code0_not_code1",
                                  "bt_code1_not_code0", "bt_explicit", "nbl2", "nbl256", "bl_code0", "bl_code1", "bl_code2", "bl_code3", "bl_code5", "bl_code25") for c in CATS]
    + ["cell%d" % k for k in range(11)] + ["insert_code23", "copy_code23", "insert0", "end_after_literals", "end_after_copy"]
    + ["ring_code%d" % k for k in range(16)] + ["ring_carried", "edge_window_back", "edge_window_dict", "edge_pos_back", "edge_pos_dict",
                                                "overlap_d1", "overlap_d63", "overlap_d64", "overlap_d65"]
    + ["dict_len4", "dict_len24", "dict_empty", "dict_upfirst_c0", "dict_upfirst_e0", "dict_upall_c0", "dict_upall_e0",
       "dict_upall_mb_end", "dict_t120", "dict_last_index"]
)
# every error and the places it is raised at, as the names of the error cases
REQUIRED_ERRORS = {
    "RESERVED": ["reserved"],
    "EXUBERANT_NIBBLE": ["exuberant_nibble_5", "exuberant_nibble_6"],
    "EXUBERANT_META_NIBBLE": ["exuberant_meta_nibble_2", "exuberant_meta_nibble_3"],
    "PADDING_1": ["padding_1_metadata", "padding_1_uncompressed"],
    "PADDING_2": ["padding_2_last_empty", "padding_2_compressed"],
    "WINDOW_BITS": ["window_bits"],
    "SIMPLE_HUFFMAN_ALPHABET": ["alphabet_704", "alphabet_nbltypes", "alphabet_context_map", "alphabet_distance_520", "alphabet_block_count"],
    "SIMPLE_HUFFMAN_SAME": ["same_2_01", "same_3_01", "same_3_02", "same_3_12", "same_4_01", "same_4_02", "same_4_03", "same_4_12",
                            "same_4_13", "same_4_23"],
    "CL_SPACE": ["cl_space_all_zero", "cl_space_over", "cl_space_space_left"],
    "HUFFMAN_SPACE": ["huffman_space_single_9", "huffman_space_repeat_past_end", "huffman_space_over", "huffman_space_space_left"],
    "CONTEXT_MAP_REPEAT": ["context_map_repeat_literal", "context_map_repeat_distance"],
    "BLOCK_LENGTH_2": ["block_length_2_insert", "block_length_2_copy", "block_length_2_dictionary"],
    "BLOCK_LENGTH_1": ["block_length_1_input_ends", "block_length_1_ring_insert", "block_length_1_ring_copy",
                       "block_length_1_ring_dictionary"],
    "DISTANCE": ["distance_code4", "distance_code14"],
    "DICTIONARY": ["dictionary_length_2", "dictionary_length_3", "dictionary_length_25"],
    "TRANSFORM": ["transform_121", "transform_127"],
}


@pytest.fixture(scope="module")
def cases():
    return F.all_cases()


def _passes(c):
    """the two checks of a case against libbrotlidec"""
    if c.err is None:
        st, out, used = B.decode(c.stream, len(c.out))
        return st == B.FINISHED and out == c.out and used == len(c.stream)
    return B.decode(c.stream, 1 << 16)[0] == c.err


def test_valid_streams_decode_to_the_writers_output(cases):
    for c in cases:
        if c.err is None:
            st, out, used = B.decode(c.stream, len(c.out))
            assert st == B.FINISHED, (c.name, st)
            assert out == c.out, c.name
            assert used == len(c.stream), c.name


def test_error_streams_give_the_named_code(cases):
    for c in cases:
        if c.err is not None:
            st = B.decode(c.stream, 1 << 16)[0]
            assert st == c.err, (c.name, st, B.error_string(st) if st < 0 else st)


def test_every_form_is_covered(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    good = [c for c in cases if _passes(c)]
    seen = set().union(*[c.tags for c in good])
    missing = [t for t in REQUIRED if t not in seen]
    assert not missing, missing
    by_name = {c.name: c for c in good}
    for code, wanted in REQUIRED_ERRORS.items():
        for name in wanted:
            assert name in by_name and by_name[name].err == F.ERR[code] and "err:" + name in by_name[name].tags, (code, name)
    assert {c.err for c in good if c.err is not None} == set(range(-16, 0))  # all sixteen codes of the decoder


def test_existing_hand_cases_keep_their_bytes():
    """the extended writer writes tests/brotli_cases.py as the writer before it did"""
    h = hashlib.sha256()
    for name, comp, out in K.all_cases():
        h.update(name.encode() + comp + out)
    assert h.hexdigest() == "fc370b7f089371738e9d4a80b05e6ceff01b0de5ced5a9d5fd3b7e5c3502fe2c"


def test_writer_context_ids_follow_the_rfc_ranges():
    """spot values of Section 7.1's tables written out by hand (not the decoder's table)"""
    assert W.context_id(0, 0xC5, 9) == 5 and W.context_id(1, 0xC5, 9) == 0x31
    assert W.context_id(2, ord(" "), ord("a")) == 8 | 3 and W.context_id(2, ord("e"), ord("Z")) == 56 | 2
    assert W.context_id(2, 0x85, 0xE2) == 1 | 2 and W.context_id(2, 0xC3, ord("1")) == 3 | 2
    assert W.context_id(3, 0, 255) == 7 and W.context_id(3, 255, 0) == 56 and W.context_id(3, 0x40, 0x0F) == (3 << 3) | 1
