"""The ctypes face of libcompu_hip.so: the structures of include/compu_hip.h, one table of its prototypes, and lib(), which loads
the library and applies the table.  compu_amd/api.py imports all of it back under the same names."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libcompu_hip.so"


def lib_path():
    # COMPU_HIP_LIB selects another build of the same library (diagnostic builds); never a CPU stand-in
    return os.environ.get("COMPU_HIP_LIB") or os.path.join(_HERE, _LIB_NAME)


class _DecodeResult(C.Structure):
    _fields_ = [("input_remain", C.c_size_t), ("output_remain", C.c_size_t), ("status", C.c_int32), ("err", C.c_int32)]


class _EncodeResult(C.Structure):
    _fields_ = [("input_remain", C.c_size_t), ("output_remain", C.c_size_t), ("status", C.c_int32)]


class _DecoderOpts(C.Structure):
    _fields_ = [("window_log_max", C.c_int32), ("device", C.c_int32)]


class _EncoderOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("compression", C.c_int32), ("device", C.c_int32), ("strategy", C.c_int32), ("mem_level", C.c_int32)]


class _ZstdEncoderOpts(C.Structure):
    _fields_ = [("level", C.c_int32), ("strategy", C.c_int32), ("window_log", C.c_int32), ("device", C.c_int32)]


class _BrotliEncoderOpts(C.Structure):
    _fields_ = [("quality", C.c_int32), ("mode", C.c_int32), ("lgwin", C.c_int32), ("device", C.c_int32)]


class _BgzfSummary(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("total_out", C.c_uint64), ("in_used", C.c_uint64), ("status", C.c_int32), ("eof", C.c_uint32)]


class _ZstdPlanSummary(C.Structure):
    _fields_ = [("n_frames", C.c_uint64), ("n_skippable", C.c_uint64), ("n_unsized", C.c_uint64), ("total_out", C.c_uint64),
                ("in_used", C.c_uint64), ("status", C.c_int32), ("pad", C.c_uint32)]


class _ZstdBlock(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("size", C.c_uint32), ("lit_regen", C.c_uint32), ("lit_comp", C.c_uint32), ("n_seq", C.c_uint32),
                ("type", C.c_uint8), ("flags", C.c_uint8), ("lit_type", C.c_uint8), ("mode", C.c_uint8 * 3), ("pad", C.c_uint8 * 2),
                ("src", C.c_int32 * 4)]


class _ZstdBlocksSummary(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("in_used", C.c_uint64), ("content_size", C.c_uint64), ("window_size", C.c_uint64),
                ("status", C.c_int32), ("descriptor", C.c_uint32), ("header_bytes", C.c_uint32), ("pad", C.c_uint32)]


class _ZstdParallelSummary(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("n_sequences", C.c_uint64), ("out_len", C.c_uint64), ("in_used", C.c_uint64), ("total_out", C.c_uint64),
                ("status", C.c_int32), ("path", C.c_uint32), ("rounds", C.c_uint32), ("check", C.c_uint32)]


class _Xxh64State(C.Structure):
    _fields_ = [("acc", C.c_uint64 * 4), ("total", C.c_uint64), ("tail", C.c_uint8 * 32), ("tail_n", C.c_uint32), ("pad", C.c_uint32)]


class _ZstdCursor(C.Structure):
    _fields_ = [("in_total", C.c_uint64), ("out_total", C.c_uint64), ("window_size", C.c_uint64), ("content_size", C.c_uint64),
                ("hist", C.c_uint64), ("ring", C.c_uint64), ("carry_at", C.c_uint64 * 4), ("carry_len", C.c_uint32 * 4), ("rep", C.c_uint32 * 3),
                ("phase", C.c_uint32), ("descriptor", C.c_uint32), ("waived", C.c_uint32), ("error", C.c_int32), ("pad", C.c_uint32),
                ("xxh", _Xxh64State)]


class _ZstdNextSummary(C.Structure):
    _fields_ = [("in_used", C.c_uint64), ("out_len", C.c_uint64), ("need_out", C.c_uint64), ("need_state", C.c_uint64), ("n_blocks", C.c_uint64),
                ("n_sequences", C.c_uint64), ("status", C.c_int32), ("rounds", C.c_uint32)]


class _ZstdSlabSummary(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("in_used", C.c_uint64), ("status", C.c_int32), ("last", C.c_uint32)]


class _GzipPlanSummary(C.Structure):
    _fields_ = [("n_members", C.c_uint64), ("total_out", C.c_uint64), ("in_used", C.c_uint64), ("status", C.c_int32),
                ("member_status", C.c_int32)]


class _ZipEntry(C.Structure):
    _fields_ = [("header_off", C.c_uint64), ("data_off", C.c_uint64), ("comp_size", C.c_uint64), ("size", C.c_uint64), ("name_off", C.c_uint64),
                ("crc32", C.c_uint32), ("name_len", C.c_uint16), ("method", C.c_uint16), ("flags", C.c_uint16), ("pad", C.c_uint16),
                ("status", C.c_int32)]


class _ZipPlanSummary(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("n_ok", C.c_uint64), ("total_size", C.c_uint64), ("cd_off", C.c_uint64), ("cd_size", C.c_uint64),
                ("eocd_off", C.c_uint64), ("bad_index", C.c_uint64), ("status", C.c_int32), ("zip64", C.c_int32)]


class _ZipDecodeSummary(C.Structure):
    _fields_ = [("n_sel", C.c_uint64), ("n_ok", C.c_uint64), ("n_bad", C.c_uint64), ("first_bad", C.c_uint64), ("total_out", C.c_uint64),
                ("status", C.c_int32), ("pad", C.c_int32)]


class _ZipSource(C.Structure):
    _fields_ = [("data_off", C.c_uint64), ("size", C.c_uint64), ("name_off", C.c_uint64), ("name_len", C.c_uint16), ("method", C.c_uint16),
                ("dos_time", C.c_uint16), ("dos_date", C.c_uint16)]


class _ZipWriteSummary(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("n_deflated", C.c_uint64), ("out_len", C.c_uint64), ("cd_off", C.c_uint64), ("cd_size", C.c_uint64),
                ("eocd_off", C.c_uint64), ("bad_index", C.c_uint64), ("status", C.c_int32), ("zip64", C.c_int32)]


class _TarEntry(C.Structure):
    _fields_ = [("group_off", C.c_uint64), ("header_off", C.c_uint64), ("data_off", C.c_uint64), ("size", C.c_uint64), ("name_off", C.c_uint64),
                ("link_off", C.c_uint64), ("mtime", C.c_int64), ("name_len", C.c_uint32), ("link_len", C.c_uint32), ("mode", C.c_uint32),
                ("prefix_len", C.c_uint16), ("typeflag", C.c_uint8), ("flags", C.c_uint8)]


class _TarPlanSummary(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("n_global", C.c_uint64), ("total_size", C.c_uint64), ("stop_off", C.c_uint64), ("bad_off", C.c_uint64),
                ("status", C.c_int32), ("zero_blocks", C.c_int32)]


class _TarSource(C.Structure):
    _fields_ = [("data_off", C.c_uint64), ("size", C.c_uint64), ("name_off", C.c_uint64), ("link_off", C.c_uint64), ("mtime", C.c_int64),
                ("name_len", C.c_uint32), ("link_len", C.c_uint32), ("mode", C.c_uint32), ("uid", C.c_uint32), ("gid", C.c_uint32),
                ("typeflag", C.c_uint8), ("pad", C.c_uint8 * 3)]


class _TarWriteSummary(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("n_ext", C.c_uint64), ("out_len", C.c_uint64), ("end_off", C.c_uint64), ("total_size", C.c_uint64),
                ("bad_index", C.c_uint64), ("status", C.c_int32), ("pad", C.c_int32)]


class _FileSummary(C.Structure):
    _fields_ = [("n_units", C.c_uint64), ("out_len", C.c_uint64), ("table_off", C.c_uint64), ("status", C.c_int32), ("pad", C.c_uint32)]


class _SelectSummary(C.Structure):
    _fields_ = [("n_sel", C.c_uint64), ("scratch_bytes", C.c_uint64), ("out_len", C.c_uint64), ("n_outside", C.c_uint64),
                ("bad_index", C.c_uint64), ("status", C.c_int32), ("pad", C.c_uint32)]


class _ReadSummary(C.Structure):
    _fields_ = [("n_units", C.c_uint64), ("out_len", C.c_uint64), ("n_outside", C.c_uint64), ("n_bad", C.c_uint64),
                ("first_bad", C.c_uint64), ("bad_index", C.c_uint64), ("status", C.c_int32), ("bad_status", C.c_int32)]


class _ZstdSeekSummary(C.Structure):
    _fields_ = [("n_frames", C.c_uint64), ("table_bytes", C.c_uint64), ("frames_bytes", C.c_uint64), ("total_out", C.c_uint64),
                ("bad_index", C.c_uint64), ("status", C.c_int32), ("checksums", C.c_uint32)]


class _InflateIndexSummary(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("out_len", C.c_uint64), ("in_used", C.c_uint64), ("end_bit", C.c_uint64), ("status", C.c_int32),
                ("wrap", C.c_uint32), ("check", C.c_uint32), ("pad", C.c_uint32)]


class _InflateParallelSummary(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("out_len", C.c_uint64), ("in_used", C.c_uint64), ("end_bit", C.c_uint64), ("total_out", C.c_uint64),
                ("n_starts", C.c_uint64), ("n_false", C.c_uint64), ("status", C.c_int32), ("wrap", C.c_uint32), ("check", C.c_uint32),
                ("path", C.c_uint32)]


class _InflateCursor(C.Structure):
    _fields_ = [("in_total", C.c_uint64), ("out_total", C.c_uint64), ("bit", C.c_uint32), ("phase", C.c_uint32), ("wrap", C.c_uint32),
                ("check", C.c_uint32), ("hist", C.c_uint32), ("error", C.c_int32)]


class _InflateNextSummary(C.Structure):
    _fields_ = [("in_used", C.c_uint64), ("out_len", C.c_uint64), ("need_out", C.c_uint64), ("n_chunks", C.c_uint64), ("n_starts", C.c_uint64),
                ("n_false", C.c_uint64), ("status", C.c_int32), ("path", C.c_uint32)]


class _Lz4Block(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("size", C.c_uint32), ("flags", C.c_uint32), ("checksum", C.c_uint32), ("pad", C.c_uint32)]


class _Lz4BlocksSummary(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("in_used", C.c_uint64), ("content_size", C.c_uint64), ("block_max", C.c_uint32), ("flg", C.c_uint32),
                ("bd", C.c_uint32), ("header_bytes", C.c_uint32), ("content_checksum", C.c_uint32), ("status", C.c_int32)]


class _Lz4ParallelSummary(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("out_len", C.c_uint64), ("in_used", C.c_uint64), ("total_out", C.c_uint64), ("status", C.c_int32),
                ("path", C.c_uint32), ("check", C.c_uint32), ("pad", C.c_uint32)]


class _SnappyChunk(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("size", C.c_uint32), ("type", C.c_uint32), ("crc", C.c_uint32), ("pad", C.c_uint32)]


class _SnappyChunksSummary(C.Structure):
    _fields_ = [("n_chunks", C.c_uint64), ("n_skipped", C.c_uint64), ("in_used", C.c_uint64), ("status", C.c_int32), ("pad", C.c_uint32)]


class _SnappyParallelSummary(C.Structure):
    _fields_ = [("n_chunks", C.c_uint64), ("out_len", C.c_uint64), ("in_used", C.c_uint64), ("total_out", C.c_uint64), ("status", C.c_int32),
                ("path", C.c_uint32), ("n_skipped", C.c_uint32), ("pad", C.c_uint32)]


# ---- the prototypes of include/compu_hip.h: (name, restype, argtypes) ------------------------------
# restype as the header states it: None for void, a pointer type, a 64-bit type for size_t / uint64_t, c_int for int, the
# structure where one comes back by value.

vp, sz, u64, u32, i32, ci, cstr = C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_int32, C.c_int, C.c_char_p
P = C.POINTER

_PROTOTYPES = [
    ("chip_device_count", ci, []),
    ("chip_set_device", ci, [ci]),
    ("chip_version", cstr, []),
    ("chip_set_allocator", None, [vp, vp, vp]),
    ("chip_device_alloc", vp, [sz]),
    ("chip_device_free", None, [vp]),
    ("chip_pinned_alloc", vp, [sz]),
    ("chip_pinned_free", None, [vp]),
    ("chip_memcpy_h2d", ci, [vp, vp, sz, vp]),
    ("chip_memcpy_d2h", ci, [vp, vp, sz, vp]),
    ("chip_stream_sync", ci, [vp]),
    ("chip_trim", ci, []),
    ("chip_decoder_new", vp, [ci, P(_DecoderOpts)]),
    ("chip_decode", _DecodeResult, [vp, vp, sz, vp, sz]),
    ("chip_decoder_reset", vp, [vp]),
    ("chip_decoder_free", None, [vp]),
    ("chip_decoder_footprint", None, [vp, P(sz), P(sz)]),
    ("chip_decoder_strerror", cstr, [ci, i32]),
    ("chip_decode_batch", ci, [ci, sz] + [vp] * 10),
    ("chip_decode_batch_ex", ci, [ci, u32, sz] + [vp] * 10),
    ("chip_decode_batch_sizes", ci, [ci, u32, sz] + [vp] * 7),
    ("chip_decode_batch_host", ci, [ci, sz] + [vp] * 9 + [ci, sz]),
    ("chip_decode_batch_multi", ci, [ci, sz] + [vp] * 9 + [vp, ci, sz]),
    ("chip_partition_units", ci, [sz, vp, vp, ci, vp]),
    ("chip_detect", ci, [vp, sz]),
    ("chip_detect_batch", ci, [sz, vp, vp, vp, vp, vp]),
    ("chip_encoder_new", vp, [P(_EncoderOpts)]),
    ("chip_encoder_new_zstd", vp, [P(_ZstdEncoderOpts)]),
    ("chip_encoder_new_brotli", vp, [P(_BrotliEncoderOpts)]),
    ("chip_encode", _EncodeResult, [vp, vp, sz, vp, sz, ci]),
    ("chip_encoder_reset", vp, [vp]),
    ("chip_encoder_free", None, [vp]),
    ("chip_encode_batch", ci, [ci, ci, sz] + [vp] * 9),
    ("chip_encode_batch_ex", ci, [ci, ci, ci, sz] + [vp] * 9),
    ("chip_encode_bound", sz, [ci, sz]),
    ("chip_encode_batch_host", ci, [ci, ci, sz] + [vp] * 8 + [ci, sz]),
    ("chip_bgzf_plan_host", ci, [vp, u64, u64, vp, vp, vp, vp, P(_BgzfSummary)]),
    ("chip_bgzf_plan", ci, [vp, u64, u64, vp, vp, vp, vp, P(_BgzfSummary), vp]),
    ("chip_bgzf_eof_block", vp, [P(sz)]),
    ("chip_zstd_plan_host", ci, [vp, u64, u64, vp, vp, vp, vp, P(_ZstdPlanSummary)]),
    ("chip_zstd_plan", ci, [vp, u64, u64, vp, vp, vp, vp, P(_ZstdPlanSummary), vp]),
    ("chip_layout_units", ci, [sz, vp, vp, vp, P(u64), P(u64), vp]),
    ("chip_zstd_blocks_host", ci, [vp, u64, u64, vp, P(_ZstdBlocksSummary)]),
    ("chip_zstd_blocks", ci, [vp, u64, u64, vp, P(_ZstdBlocksSummary), vp]),
    ("chip_zstd_parallel", ci, [vp, u64, vp, u64, ci, u32, P(_ZstdParallelSummary), vp]),
    ("chip_zstd_parallel_next", ci, [P(_ZstdCursor), vp, u64, vp, u64, vp, u64, ci, u32, P(_ZstdNextSummary), vp]),
    ("chip_zstd_slab_blocks_host", ci, [vp, u64, u64, u64, vp, P(_ZstdSlabSummary)]),
    ("chip_zstd_cursor_header_host", ci, [P(_ZstdCursor), vp, u64, ci, u32, P(u32), P(u64)]),
    ("chip_xxh64_update_host", ci, [P(_Xxh64State), vp, u64]),
    ("chip_xxh64_digest_host", u64, [P(_Xxh64State)]),
    ("chip_gzip_plan", ci, [vp, u64, u64, vp, vp, vp, vp, P(_GzipPlanSummary), vp]),
    ("chip_zip_plan_host", ci, [vp, u64, u64, vp, P(_ZipPlanSummary)]),
    ("chip_zip_plan", ci, [vp, u64, u64, vp, P(_ZipPlanSummary), vp]),
    ("chip_crc32_batch", ci, [sz, vp, vp, vp, vp, vp]),
    ("chip_zip_decode", ci, [vp, u64, vp, u64, u64, vp, vp, u64, vp, vp, P(_ZipDecodeSummary), vp]),
    ("chip_zip_assemble_host", ci, [u64, vp, vp, u64, vp, u64, vp, u64, vp, vp, vp, u32, vp, u64, vp, P(_ZipWriteSummary)]),
    ("chip_zip_assemble", ci, [u64, vp, vp, u64, vp, u64, vp, u64, vp, vp, vp, u32, vp, u64, vp, P(_ZipWriteSummary), vp]),
    ("chip_zip_write", ci, [ci, u32, u64, vp, vp, u64, vp, u64, vp, u64, vp, P(_ZipWriteSummary), vp]),
    ("chip_zip_write_bound", u64, [u64, u64, u64]),
    ("chip_tar_plan_host", ci, [vp, u64, u64, vp, P(_TarPlanSummary)]),
    ("chip_tar_plan", ci, [vp, u64, u64, vp, P(_TarPlanSummary), vp]),
    ("chip_tar_write_host", ci, [u64, vp, vp, u64, vp, u64, u32, u32, vp, u64, vp, P(_TarWriteSummary)]),
    ("chip_tar_write", ci, [u64, vp, vp, u64, vp, u64, u32, u32, vp, u64, vp, P(_TarWriteSummary), vp]),
    ("chip_tar_write_bound", u64, [u64, u64, u64, u32]),
    ("chip_pack_units", ci, [sz, vp, vp, vp, vp, u64, vp, P(u64), vp]),
    ("chip_encode_file", ci, [ci, ci, u32, u32, vp, u64, vp, u64, P(_FileSummary), vp]),
    ("chip_encode_file_bound", u64, [ci, u32, u32, u64]),
    ("chip_select_units_host", ci, [sz, vp, vp, vp, vp, sz, vp, vp, u64] + [vp] * 8 + [P(_SelectSummary)]),
    ("chip_select_units", ci, [sz, vp, vp, vp, vp, sz, vp, vp, u64] + [vp] * 8 + [P(_SelectSummary), vp]),
    ("chip_read_ranges", ci, [ci, sz, vp, vp, vp, vp, vp, sz, vp, vp, vp, u64, vp, vp, P(_ReadSummary), vp]),
    ("chip_zstd_seek_plan_host", ci, [vp, u64, u64, u64, vp, vp, vp, vp, vp, P(_ZstdSeekSummary)]),
    ("chip_zstd_seek_plan", ci, [vp, u64, u64, u64, vp, vp, vp, vp, vp, P(_ZstdSeekSummary), vp]),
    ("chip_zstd_seek_table_write_host", ci, [u64, vp, vp, vp, vp, u64, P(u64)]),
    ("chip_zstd_seek_table_write", ci, [u64, vp, vp, vp, vp, u64, P(u64), vp]),
    ("chip_xxh64_batch", ci, [sz, vp, vp, vp, vp, vp]),
    ("chip_zstd_seek_read", ci, [sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, u64, vp, vp, P(_ReadSummary), vp]),
    ("chip_lz4_block_decode_host", ci, [vp, u64, vp, u64, P(u64), P(u64)]),
    ("chip_lz4_blocks_host", ci, [vp, u64, u64, vp, P(_Lz4BlocksSummary)]),
    ("chip_lz4_blocks", ci, [vp, u64, u64, vp, P(_Lz4BlocksSummary), vp]),
    ("chip_xxh32_batch", ci, [sz, vp, vp, vp, u32, vp, vp]),
    ("chip_lz4_parallel", ci, [vp, u64, vp, u64, u32, P(_Lz4ParallelSummary), vp]),
    ("chip_lz4_block_encode_host", ci, [vp, u64, ci, vp, u64, P(u64)]),
    ("chip_lz4_frame_encode_host", ci, [vp, u64, ci, ci, vp, u64, P(u64)]),
    ("chip_snappy_block_decode_host", ci, [vp, u64, vp, u64, P(u64), P(u64)]),
    ("chip_snappy_chunks_host", ci, [vp, u64, u64, vp, P(_SnappyChunksSummary)]),
    ("chip_snappy_chunks", ci, [vp, u64, u64, vp, P(_SnappyChunksSummary), vp]),
    ("chip_crc32c_batch", ci, [sz, vp, vp, vp, vp, vp]),
    ("chip_snappy_parallel", ci, [vp, u64, vp, u64, u32, P(_SnappyParallelSummary), vp]),
    ("chip_inflate_index_build", ci, [ci, vp, u64, vp, u64, u32, u64, vp, vp, vp, vp, P(_InflateIndexSummary), vp]),
    ("chip_inflate_index_units_host", ci, [ci, u64, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, P(i32), P(u64)]),
    ("chip_inflate_index_read", ci, [ci, vp, u64, u64, vp, vp, vp, vp, u64, sz, vp, vp, vp, u64, vp, vp, P(_ReadSummary), vp]),
    ("chip_inflate_find_starts_host", ci, [vp, u64, u64, u32, u64, vp, P(u64)]),
    ("chip_inflate_find_starts", ci, [vp, u64, u64, u32, u64, vp, P(u64), vp]),
    ("chip_inflate_parallel", ci, [ci, vp, u64, vp, u64, u32, u64, vp, vp, vp, vp, P(_InflateParallelSummary), vp]),
    ("chip_inflate_parallel_next", ci, [ci, P(_InflateCursor), vp, vp, u64, vp, u64, u32, P(_InflateNextSummary), vp]),
]

_lib = None


def lib():
    """Load libcompu_hip.so.  Raises if it has not been built: there is no fallback codec."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with compu_amd/csrc/build.sh (or __graft_entry__.build()); "
            "compu_amd has no CPU codec to fall back to"
        )
    try:  # share torch's HIP runtime when torch is in the process (same SONAME libamdhip64.so.7)
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing only
        pass
    L = C.CDLL(path)
    for name, restype, argtypes in _PROTOTYPES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L
