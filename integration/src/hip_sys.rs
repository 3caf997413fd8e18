//! Raw bindings of `libcompu_hip.so` (include/compu_hip.h), the MI355X backend.
#![allow(non_camel_case_types)]

use core::ffi::{c_char, c_int, c_void};

#[repr(C)]
pub struct chip_decoder {
    _private: [u8; 0],
}
#[repr(C)]
pub struct chip_encoder {
    _private: [u8; 0],
}

///`chip_decode_result`: `Decode` with the error code split out (`err == 0` means `Ok(status)`)
#[repr(C)]
pub struct chip_decode_result {
    pub input_remain: usize,
    pub output_remain: usize,
    pub status: i32,
    pub err: i32,
}

#[repr(C)]
pub struct chip_encode_result {
    pub input_remain: usize,
    pub output_remain: usize,
    pub status: i32,
}

#[repr(C)]
pub struct chip_decoder_opts {
    pub window_log_max: i32,
    pub device: i32,
}

#[repr(C)]
pub struct chip_encoder_opts {
    pub mode: i32,
    pub compression: i32,
    pub device: i32,
    pub strategy: i32,
    pub mem_level: i32,
}

///`chip_zstd_encoder_opts`: the encoder's `ZstdOptions` (src/encoder/zstd.rs:62-126)
#[repr(C)]
pub struct chip_zstd_encoder_opts {
    pub level: i32,
    pub strategy: i32,
    pub window_log: i32,
    pub device: i32,
}

///`chip_brotli_encoder_opts`: the encoder's `BrotliOptions` (src/encoder/brotli_common.rs) and the window
#[repr(C)]
pub struct chip_brotli_encoder_opts {
    pub quality: i32,
    pub mode: i32,
    pub lgwin: i32,
    pub device: i32,
}

pub const CHIP_FMT_ZSTD: c_int = 100;
pub const CHIP_FMT_BROTLI: c_int = 101;
///`chip_encode_batch` / `_ex` / `_host` and `chip_encode_bound` only: one BGZF block per unit (at most 65280 input bytes each)
pub const CHIP_FMT_BGZF: c_int = 131;
///route every unit of a batch by `Detection::detect` (src/decoder/mod.rs:28-114)
pub const CHIP_FMT_DETECT: c_int = 0;

///`chip_decode_batch_ex` flag: report `DecodeStatus` exactly as compu's `decode_fn` would
pub const CHIP_F_COMPU_STATUS: u32 = 1;
///`chip_decode_batch_ex` / `chip_decode_batch_sizes` flag: a unit is a series of gzip members or zstd frames, decoded one behind the
///other (gzip, auto, zstd and detect batches; not together with `CHIP_F_COMPU_STATUS`).  No compu counterpart.
pub const CHIP_F_MEMBERS: u32 = 2;
///`chip_decode_batch` / `chip_encode_batch` return codes
pub const CHIP_OK: c_int = 0;

///`chip_bgzf_summary::status`
pub const CHIP_BGZF_OK: i32 = 0;
pub const CHIP_BGZF_TRUNCATED: i32 = 1;
pub const CHIP_BGZF_BAD_HEADER: i32 = 2;

///what the BGZF walk found: blocks and decoded bytes of the whole walk, where it stopped and why, whether the last block is empty
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_bgzf_summary {
    pub n_blocks: u64,
    pub total_out: u64,
    pub in_used: u64,
    pub status: i32,
    pub eof: u32,
}

///`chip_zstd_plan_summary::status`
pub const CHIP_ZPLAN_OK: i32 = 0;
pub const CHIP_ZPLAN_TRUNCATED: i32 = 1;
pub const CHIP_ZPLAN_BAD_HEADER: i32 = 2;
pub const CHIP_ZPLAN_TOO_LARGE: i32 = 3;
///`out_cap` of a frame without `Frame_Content_Size`
pub const CHIP_ZPLAN_UNSIZED: u32 = 0xFFFF_FFFF;
///blocks per frame the walk follows
pub const CHIP_ZPLAN_MAX_BLOCKS: u32 = 1 << 20;

///what the zstd frame walk found: frames, skippable frames, frames without a content size and stated content bytes of the whole
///walk, the start of the frame where it stopped and why
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zstd_plan_summary {
    pub n_frames: u64,
    pub n_skippable: u64,
    pub n_unsized: u64,
    pub total_out: u64,
    pub in_used: u64,
    pub status: i32,
    pub pad: u32,
}

///`content_size` of a frame without `Frame_Content_Size`
pub const CHIP_ZBLOCKS_UNSIZED: u64 = u64::MAX;
///`chip_zstd_block::flags`
pub const CHIP_ZBLOCK_LAST: u8 = 1;
pub const CHIP_ZBLOCK_MALFORMED: u8 = 2;
///the columns of `chip_zstd_block::src`
pub const CHIP_ZSRC_HUF: usize = 0;
pub const CHIP_ZSRC_LL: usize = 1;
pub const CHIP_ZSRC_OF: usize = 2;
pub const CHIP_ZSRC_ML: usize = 3;

///one block of a zstd frame as its headers describe it: where it lies, its type, a compressed block's literals and sequences section
///headers, and per table kind the nearest earlier block that defined the table (-1: none)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zstd_block {
    pub offset: u64,
    pub size: u32,
    pub lit_regen: u32,
    pub lit_comp: u32,
    pub n_seq: u32,
    pub r#type: u8,
    pub flags: u8,
    pub lit_type: u8,
    pub mode: [u8; 3],
    pub pad: [u8; 2],
    pub src: [i32; 4],
}

///what the walk over one frame's block headers found: the blocks counted, the frame's end (0 when the walk stopped early), the
///stated content size, the window, why it stopped (`CHIP_ZPLAN_*`), the frame header descriptor and the frame header's length
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zstd_blocks_summary {
    pub n_blocks: u64,
    pub in_used: u64,
    pub content_size: u64,
    pub window_size: u64,
    pub status: i32,
    pub descriptor: u32,
    pub header_bytes: u32,
    pub pad: u32,
}

///`chip_zstd_parallel_summary::path`
pub const CHIP_ZPAR_SERIAL: u32 = 0;
pub const CHIP_ZPAR_PARALLEL: u32 = 1;
pub const CHIP_ZPAR_REFUSED: u32 = 2;
///`chip_zstd_parallel` flag: do not verify `Content_Checksum`
pub const CHIP_ZPAR_NO_CHECKSUM: u32 = 1;
pub const CHIP_ZPAR_ROUNDS_MAX: u32 = 40;

///what `chip_zstd_parallel` did: blocks and sequences of the frame, bytes written, input consumed, the exact size to come back with,
///the batch decode's status, the path taken, the rounds of the jump pass
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zstd_parallel_summary {
    pub n_blocks: u64,
    pub n_sequences: u64,
    pub out_len: u64,
    pub in_used: u64,
    pub total_out: u64,
    pub status: i32,
    pub path: u32,
    pub rounds: u32,
    pub check: u32,
}

///LZ4 (the batch calls, decode and encode; no compu counterpart): one raw block per unit, one frame per unit
pub const CHIP_FMT_LZ4_BLOCK: c_int = 102;
pub const CHIP_FMT_LZ4: c_int = 103;
///per-unit status of an LZ4 unit, beside `CHIP_NEED_INPUT` / `CHIP_NEED_OUTPUT` / `CHIP_FINISHED`
pub const CHIP_LZ4_E_HEADER: i32 = -200;
pub const CHIP_LZ4_E_DICT: i32 = -201;
pub const CHIP_LZ4_E_BLOCK_SIZE: i32 = -202;
pub const CHIP_LZ4_E_BLOCK: i32 = -203;
pub const CHIP_LZ4_E_OFFSET: i32 = -204;
pub const CHIP_LZ4_E_BLOCK_CHECKSUM: i32 = -205;
pub const CHIP_LZ4_E_CONTENT_SIZE: i32 = -206;
pub const CHIP_LZ4_E_CONTENT_CHECKSUM: i32 = -207;
///`chip_lz4_blocks_summary::content_size` of a frame without C.Size
pub const CHIP_LZ4BLOCKS_UNSIZED: u64 = u64::MAX;
///`chip_lz4_block::flags`
pub const CHIP_LZ4BLOCK_STORED: u32 = 1;
pub const CHIP_LZ4BLOCK_LAST: u32 = 2;

///one block of an LZ4 frame as `chip_lz4_blocks` describes it: where its 4-byte header lies, its size, flags, stored checksum
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_lz4_block {
    pub offset: u64,
    pub size: u32,
    pub flags: u32,
    pub checksum: u32,
    pub pad: u32,
}

///what the walk over an LZ4 frame's block headers found; `status` is a `CHIP_ZPLAN_*` value
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_lz4_blocks_summary {
    pub n_blocks: u64,
    pub in_used: u64,
    pub content_size: u64,
    pub block_max: u32,
    pub flg: u32,
    pub bd: u32,
    pub header_bytes: u32,
    pub content_checksum: u32,
    pub status: i32,
}

///`chip_lz4_parallel_summary::path`
pub const CHIP_LZ4PAR_SERIAL: u32 = 0;
pub const CHIP_LZ4PAR_PARALLEL: u32 = 1;
pub const CHIP_LZ4PAR_REFUSED: u32 = 2;
///`chip_lz4_parallel` flag: do not verify the content checksum on the parallel path
pub const CHIP_LZ4PAR_NO_CHECKSUM: u32 = 1;
///`chip_encode_batch_ex` strategy bits for `CHIP_FMT_LZ4`: block checksums, no content checksum, the block-size id (0, 4..7)
pub const CHIP_LZ4_S_BLOCK_CHECKSUM: c_int = 1;
pub const CHIP_LZ4_S_NO_CONTENT_CHECKSUM: c_int = 2;
pub const CHIP_LZ4_S_BLOCK_ID_SHIFT: c_int = 4;
pub const CHIP_LZ4_S_BLOCK_ID_MASK: c_int = 0x70;
///`chip_encode_file` flags for `CHIP_FMT_LZ4`
pub const CHIP_W_LZ4_CONTENT_CHECKSUM: u32 = 2;
pub const CHIP_W_LZ4_BLOCK_CHECKSUM: u32 = 4;

///what `chip_lz4_parallel` did: blocks of the frame, bytes written, input consumed, the exact size to come back with, the one-unit
///decode's status, the path taken, the content checksum computed on the parallel path
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_lz4_parallel_summary {
    pub n_blocks: u64,
    pub out_len: u64,
    pub in_used: u64,
    pub total_out: u64,
    pub status: i32,
    pub path: u32,
    pub check: u32,
    pub pad: u32,
}

///Snappy (the decode batch calls only; no compu counterpart): one raw block per unit, one stream of the framing format per unit
pub const CHIP_FMT_SNAPPY_BLOCK: c_int = 104;
pub const CHIP_FMT_SNAPPY: c_int = 105;
///per-unit status of a Snappy unit, beside `CHIP_NEED_INPUT` / `CHIP_NEED_OUTPUT` / `CHIP_FINISHED`
pub const CHIP_SNAPPY_E_PREAMBLE: i32 = -210;
pub const CHIP_SNAPPY_E_OFFSET: i32 = -211;
pub const CHIP_SNAPPY_E_LENGTH: i32 = -212;
pub const CHIP_SNAPPY_E_HEADER: i32 = -213;
pub const CHIP_SNAPPY_E_CHUNK: i32 = -214;
pub const CHIP_SNAPPY_E_CHUNK_SIZE: i32 = -215;
pub const CHIP_SNAPPY_E_BLOCK: i32 = -216;
pub const CHIP_SNAPPY_E_CHECKSUM: i32 = -217;
///`chip_snappy_parallel_summary::path`
pub const CHIP_SNAPPYPAR_SERIAL: u32 = 0;
pub const CHIP_SNAPPYPAR_PARALLEL: u32 = 1;
pub const CHIP_SNAPPYPAR_REFUSED: u32 = 2;

///one data chunk of a framed Snappy stream as `chip_snappy_chunks` describes it: where its 4-byte header lies, the length `s` behind
///it, its type (0 compressed, 1 uncompressed), the stored masked CRC-32C
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_snappy_chunk {
    pub offset: u64,
    pub size: u32,
    pub r#type: u32,
    pub crc: u32,
    pub pad: u32,
}

///what the walk over a framed Snappy stream's chunk headers found; `status` is a `CHIP_ZPLAN_*` value
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_snappy_chunks_summary {
    pub n_chunks: u64,
    pub n_skipped: u64,
    pub in_used: u64,
    pub status: i32,
    pub pad: u32,
}

///what `chip_snappy_parallel` did: data chunks of the stream, bytes written, input consumed, the exact size to come back with, the
///one-unit decode's status, the path taken, the chunks stepped over
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_snappy_parallel_summary {
    pub n_chunks: u64,
    pub out_len: u64,
    pub in_used: u64,
    pub total_out: u64,
    pub status: i32,
    pub path: u32,
    pub n_skipped: u32,
    pub pad: u32,
}

///`chip_gzip_plan_summary::status`
pub const CHIP_GZPLAN_OK: i32 = 0;
pub const CHIP_GZPLAN_TRUNCATED: i32 = 1;
pub const CHIP_GZPLAN_BAD_HEADER: i32 = 2;
pub const CHIP_GZPLAN_TOO_LARGE: i32 = 3;
pub const CHIP_GZPLAN_BAD_MEMBER: i32 = 4;
///input bytes a gzip member may take: the limit of a unit's input
pub const CHIP_GZPLAN_WINDOW: u32 = (1 << 29) - 64;

///what the gzip member walk found: members and decoded bytes of the whole walk, the start of the member where it stopped, why, and
///the size pass's status of that member when `status` is `CHIP_GZPLAN_BAD_MEMBER`
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_gzip_plan_summary {
    pub n_members: u64,
    pub total_out: u64,
    pub in_used: u64,
    pub status: i32,
    pub member_status: i32,
}

///`chip_zip_plan_summary::status`
pub const CHIP_ZIP_OK: i32 = 0;
pub const CHIP_ZIP_NO_EOCD: i32 = 1;
pub const CHIP_ZIP_BAD_DIRECTORY: i32 = 2;
pub const CHIP_ZIP_UNSUPPORTED: i32 = 3;
///`chip_zip_entry::status`, and what `chip_zip_decode` answers beside the decode statuses
pub const CHIP_ZIPENT_OK: i32 = 0;
pub const CHIP_ZIPENT_UNSUPPORTED: i32 = 16;
pub const CHIP_ZIPENT_ENCRYPTED: i32 = 17;
pub const CHIP_ZIPENT_BAD_LOCAL: i32 = 18;
pub const CHIP_ZIPENT_TOO_LARGE: i32 = 19;
pub const CHIP_ZIPENT_BAD_SIZE: i32 = 20;
pub const CHIP_ZIPENT_BAD_CRC: i32 = 21;
pub const CHIP_ZIPENT_BAD_INDEX: i32 = 22;
///bytes of a piece of a `chip_crc32_batch` range
pub const CHIP_CRC_PIECE: u32 = 65536;

///one entry of a ZIP archive's directory as `chip_zip_plan` lists it (56 bytes, no implicit padding)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zip_entry {
    pub header_off: u64,
    pub data_off: u64,
    pub comp_size: u64,
    pub size: u64,
    pub name_off: u64,
    pub crc32: u32,
    pub name_len: u16,
    pub method: u16,
    pub flags: u16,
    pub pad: u16,
    pub status: i32,
}

///what the directory walk found: entries, OK entries and their decoded bytes of the whole walk, where the directory and the end
///record lie, the entry a `CHIP_ZIP_BAD_DIRECTORY` walk stopped at, why it stopped, whether ZIP64 records were read
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zip_plan_summary {
    pub n_entries: u64,
    pub n_ok: u64,
    pub total_size: u64,
    pub cd_off: u64,
    pub cd_size: u64,
    pub eocd_off: u64,
    pub bad_index: u64,
    pub status: i32,
    pub zip64: i32,
}

///what `chip_zip_decode` did: entries selected, those that are `CHIP_FINISHED`, the others, the lowest position of one of those,
///the bytes of the layout (the exact size needed on `CHIP_READ_NEED_OUTPUT`)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zip_decode_summary {
    pub n_sel: u64,
    pub n_ok: u64,
    pub n_bad: u64,
    pub first_bad: u64,
    pub total_out: u64,
    pub status: i32,
    pub pad: i32,
}

///`chip_zip_source::method`
pub const CHIP_ZIP_STORE: u16 = 0;
pub const CHIP_ZIP_DEFLATE: u16 = 8;
///flags of the ZIP writer's calls: every record in its ZIP64 form; general purpose bit 11, the names are UTF-8
pub const CHIP_ZW_ZIP64: u32 = 1;
pub const CHIP_ZW_UTF8: u32 = 2;
///`chip_zip_write_summary::status`
pub const CHIP_ZIPW_OK: i32 = 0;
pub const CHIP_ZIPW_NEED_OUTPUT: i32 = 1;
pub const CHIP_ZIPW_BAD_SOURCE: i32 = 2;
///`chip_zip_write` stores an entry above this size: the limit of a unit of `chip_encode_file`
pub const CHIP_ZIPW_DEFLATE_MAX: u32 = 1 << 30;

///one entry to be written into a ZIP archive (32 bytes, no implicit padding): where its content and its name lie, the method asked
///for, the DOS time stamp
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zip_source {
    pub data_off: u64,
    pub size: u64,
    pub name_off: u64,
    pub name_len: u16,
    pub method: u16,
    pub dos_time: u16,
    pub dos_date: u16,
}

///what the ZIP writer made: entries, those written deflated, the archive's length (the exact room needed on
///`CHIP_ZIPW_NEED_OUTPUT`), the directory's and the end record's place, the lowest bad record on `CHIP_ZIPW_BAD_SOURCE`
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zip_write_summary {
    pub n_entries: u64,
    pub n_deflated: u64,
    pub out_len: u64,
    pub cd_off: u64,
    pub cd_size: u64,
    pub eocd_off: u64,
    pub bad_index: u64,
    pub status: i32,
    pub zip64: i32,
}

///`chip_tar_plan_summary::status`
pub const CHIP_TAR_OK: i32 = 0;
pub const CHIP_TAR_TRUNCATED: i32 = 1;
pub const CHIP_TAR_BAD_HEADER: i32 = 2;
pub const CHIP_TAR_UNSUPPORTED: i32 = 3;
///extension headers a group may hold, and the bytes of data one of them may have
pub const CHIP_TAR_EXT_MAX: u32 = 16;
pub const CHIP_TAR_EXT_BYTES: u32 = 1 << 20;
///`chip_tar_entry::flags`: where name, link name and size came from
pub const CHIP_TARF_NAME_GNU: u8 = 1;
pub const CHIP_TARF_NAME_PAX: u8 = 2;
pub const CHIP_TARF_LINK_GNU: u8 = 4;
pub const CHIP_TARF_LINK_PAX: u8 = 8;
pub const CHIP_TARF_SIZE_PAX: u8 = 16;
pub const CHIP_TARF_SIZE_BASE256: u8 = 32;

///one member of a tar image as `chip_tar_plan` lists it (72 bytes, no implicit padding): offsets into the image
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_tar_entry {
    pub group_off: u64,
    pub header_off: u64,
    pub data_off: u64,
    pub size: u64,
    pub name_off: u64,
    pub link_off: u64,
    pub mtime: i64,
    pub name_len: u32,
    pub link_len: u32,
    pub mode: u32,
    pub prefix_len: u16,
    pub typeflag: u8,
    pub flags: u8,
}

///what the tar walk found: members, global headers and content bytes of the whole walk, where it stopped, the offending header,
///why, and the all-zero blocks at the stop
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_tar_plan_summary {
    pub n_entries: u64,
    pub n_global: u64,
    pub total_size: u64,
    pub stop_off: u64,
    pub bad_off: u64,
    pub status: i32,
    pub zero_blocks: i32,
}

///flags of the tar writer's calls: GNU long-name headers and base-256 sizes instead of pax records; every size the long way
pub const CHIP_TW_GNU: u32 = 1;
pub const CHIP_TW_FORCE_EXT: u32 = 2;
///`chip_tar_write_summary::status`
pub const CHIP_TARW_OK: i32 = 0;
pub const CHIP_TARW_NEED_OUTPUT: i32 = 1;
pub const CHIP_TARW_BAD_SOURCE: i32 = 2;
///the longest name or link name of a source
pub const CHIP_TARW_NAME_MAX: u32 = 65535;

///one member to be written into a tar image (64 bytes, no implicit padding): where its content, its name and its link name lie,
///and the numbers of its header
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_tar_source {
    pub data_off: u64,
    pub size: u64,
    pub name_off: u64,
    pub link_off: u64,
    pub mtime: i64,
    pub name_len: u32,
    pub link_len: u32,
    pub mode: u32,
    pub uid: u32,
    pub gid: u32,
    pub typeflag: u8,
    pub pad: [u8; 3],
}

///what the tar writer made: members, extension headers, the image's length, where the end blocks start, the sum of the sizes,
///the lowest bad record, why
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_tar_write_summary {
    pub n_entries: u64,
    pub n_ext: u64,
    pub out_len: u64,
    pub end_off: u64,
    pub total_size: u64,
    pub bad_index: u64,
    pub status: i32,
    pub pad: i32,
}

///`chip_encode_file` flag: the seek table of zstd's seekable format follows the last frame (`CHIP_FMT_ZSTD` only)
pub const CHIP_W_SEEK_TABLE: u32 = 1;
///`chip_file_summary::status`
pub const CHIP_FILE_OK: i32 = 0;
pub const CHIP_FILE_NEED_OUTPUT: i32 = 1;

///what `chip_encode_file` wrote: units encoded, the file's length (the exact size needed on `CHIP_FILE_NEED_OUTPUT`), where the seek
///table starts (`out_len` without one)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_file_summary {
    pub n_units: u64,
    pub out_len: u64,
    pub table_off: u64,
    pub status: i32,
    pub pad: u32,
}

///`chip_select_summary::status` / `chip_read_summary::status`
pub const CHIP_READ_OK: i32 = 0;
pub const CHIP_READ_NEED_OUTPUT: i32 = 1;
pub const CHIP_READ_BAD_LAYOUT: i32 = 2;
///`range_status[r]` of `chip_select_units` / `chip_read_ranges`
pub const CHIP_RANGE_OK: i32 = 0;
pub const CHIP_RANGE_OUTSIDE: i32 = 1;
pub const CHIP_RANGE_BAD_UNIT: i32 = 2;

///what the selection found: units selected, their decoded size, the bytes of the ranges, ranges outside the content; on
///`CHIP_READ_BAD_LAYOUT` only `bad_index` (the lowest unit that does not follow its predecessor) is set
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_select_summary {
    pub n_sel: u64,
    pub scratch_bytes: u64,
    pub out_len: u64,
    pub n_outside: u64,
    pub bad_index: u64,
    pub status: i32,
    pub pad: u32,
}

///what `chip_read_ranges` did: units decoded, bytes of ranges (the exact size needed on `CHIP_READ_NEED_OUTPUT`), ranges outside
///the content, selected units that did not decode to their size, the lowest one's index and decode status
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_read_summary {
    pub n_units: u64,
    pub out_len: u64,
    pub n_outside: u64,
    pub n_bad: u64,
    pub first_bad: u64,
    pub bad_index: u64,
    pub status: i32,
    pub bad_status: i32,
}

///`chip_zstd_seek_summary::status`
pub const CHIP_ZSEEK_OK: i32 = 0;
pub const CHIP_ZSEEK_NO_TABLE: i32 = 1;
pub const CHIP_ZSEEK_NEED_TAIL: i32 = 2;
pub const CHIP_ZSEEK_BAD_TABLE: i32 = 3;
pub const CHIP_ZSEEK_TOO_LARGE: i32 = 4;
pub const CHIP_ZSEEK_BAD_LAYOUT: i32 = 5;

///what the walk over a seek table found: entries, the table's size (on `CHIP_ZSEEK_NEED_TAIL` the tail to come back with), the
///sums of the compressed and the content sizes, the lowest entry without a size on `CHIP_ZSEEK_TOO_LARGE`, whether the entries
///carry checksums
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zstd_seek_summary {
    pub n_frames: u64,
    pub table_bytes: u64,
    pub frames_bytes: u64,
    pub total_out: u64,
    pub bad_index: u64,
    pub status: i32,
    pub checksums: u32,
}

///what `chip_inflate_index_build` found: points of the whole walk; `out_len`, `in_used`, `status` as `chip_decode_batch` answers
///them for the unit; `wrap` 0 raw / 1 zlib / 2 gzip; with `CHIP_FINISHED`, `check` the content's CRC-32 / Adler-32 and `end_bit`
///the bit behind the final block
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_inflate_index_summary {
    pub n_points: u64,
    pub out_len: u64,
    pub in_used: u64,
    pub end_bit: u64,
    pub status: i32,
    pub wrap: u32,
    pub check: u32,
    pub pad: u32,
}
///bytes of a window slot of the checkpoint index
pub const CHIP_INDEX_WINDOW: usize = 32768;

///`chip_inflate_parallel_summary::path`
pub const CHIP_PAR_SERIAL: u32 = 0;
pub const CHIP_PAR_PARALLEL: u32 = 1;
///what `chip_inflate_parallel` answers: the index build's fields, `total_out` (with `CHIP_NEED_OUTPUT` and `out_len` 0: the size to
///come back with), the finder's `n_starts`, the `n_false` of them that were no boundaries, and which `path` decoded
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_inflate_parallel_summary {
    pub n_points: u64,
    pub out_len: u64,
    pub in_used: u64,
    pub end_bit: u64,
    pub total_out: u64,
    pub n_starts: u64,
    pub n_false: u64,
    pub status: i32,
    pub wrap: u32,
    pub check: u32,
    pub path: u32,
}

///`chip_inflate_cursor::phase`
pub const CHIP_CUR_HEADER: u32 = 0;
pub const CHIP_CUR_BLOCKS: u32 = 1;
pub const CHIP_CUR_TRAILER: u32 = 2;
pub const CHIP_CUR_DONE: u32 = 3;
pub const CHIP_CUR_ERROR: u32 = 4;
///where a slabbed decode of one stream stands (`chip_inflate_parallel_next`): plain host data, all zero = the beginning of a stream;
///the last `hist` bytes of the content live in 32 768 bytes of device memory beside it
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_inflate_cursor {
    pub in_total: u64,
    pub out_total: u64,
    pub bit: u32,
    pub phase: u32,
    pub wrap: u32,
    pub check: u32,
    pub hist: u32,
    pub error: i32,
}
///what one `chip_inflate_parallel_next` call answers: the bytes it consumed and delivered, the size of the piece that did not fit
///(`need_out`), the slab's chunks, starts and false starts, why it stopped and which `path` decoded
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_inflate_next_summary {
    pub in_used: u64,
    pub out_len: u64,
    pub need_out: u64,
    pub n_chunks: u64,
    pub n_starts: u64,
    pub n_false: u64,
    pub status: i32,
    pub path: u32,
}

///`chip_zstd_cursor::phase`
pub const CHIP_ZCUR_HEADER: u32 = 0;
pub const CHIP_ZCUR_BLOCKS: u32 = 1;
pub const CHIP_ZCUR_CHECKSUM: u32 = 2;
pub const CHIP_ZCUR_DONE: u32 = 3;
pub const CHIP_ZCUR_ERROR: u32 = 4;
///one carry slot of a `chip_zstd_cursor`'s device state, and the four of them in front of the window
pub const CHIP_ZCUR_SLOT_BYTES: usize = 131088;
pub const CHIP_ZCUR_CARRY_BYTES: usize = 4 * CHIP_ZCUR_SLOT_BYTES;
///a running XXH64 (seed 0): accumulators, bytes covered, the bytes behind the last whole stripe; all zero = nothing hashed
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_xxh64_state {
    pub acc: [u64; 4],
    pub total: u64,
    pub tail: [u8; 32],
    pub tail_n: u32,
    pub pad: u32,
}
///where a slabbed decode of one zstd frame stands (`chip_zstd_parallel_next`): plain host data, all zero = the beginning of a
///frame; the carried table definers and the window ring live in device memory beside it
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zstd_cursor {
    pub in_total: u64,
    pub out_total: u64,
    pub window_size: u64,
    pub content_size: u64,
    pub hist: u64,
    pub ring: u64,
    pub carry_at: [u64; 4],
    pub carry_len: [u32; 4],
    pub rep: [u32; 3],
    pub phase: u32,
    pub descriptor: u32,
    pub waived: u32,
    pub error: i32,
    pub pad: u32,
    pub xxh: chip_xxh64_state,
}
///what one `chip_zstd_parallel_next` call answers: the bytes it consumed and delivered, the size of the block that did not fit
///(`need_out`), the state bytes to come back with (`need_state`), the blocks and sequences taken, why it stopped, the jump rounds
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zstd_next_summary {
    pub in_used: u64,
    pub out_len: u64,
    pub need_out: u64,
    pub need_state: u64,
    pub n_blocks: u64,
    pub n_sequences: u64,
    pub status: i32,
    pub rounds: u32,
}
///what the walk from a block boundary found (`chip_zstd_slab_blocks_host`)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct chip_zstd_slab_summary {
    pub n_blocks: u64,
    pub in_used: u64,
    pub status: i32,
    pub last: u32,
}

pub type chip_malloc_fn = unsafe extern "C" fn(opaque: *mut c_void, size: usize) -> *mut c_void;
pub type chip_free_fn = unsafe extern "C" fn(opaque: *mut c_void, ptr: *mut c_void);

#[link(name = "compu_hip")]
extern "C" {
    pub fn chip_device_count() -> c_int;
    pub fn chip_set_allocator(malloc_fn: Option<chip_malloc_fn>, free_fn: Option<chip_free_fn>, opaque: *mut c_void);
    pub fn chip_device_alloc(size: usize) -> *mut c_void;
    pub fn chip_device_free(ptr: *mut c_void);
    pub fn chip_pinned_alloc(size: usize) -> *mut c_void;
    pub fn chip_pinned_free(ptr: *mut c_void);
    pub fn chip_memcpy_h2d(dst_dev: *mut c_void, src_host: *const c_void, size: usize, stream: *mut c_void) -> c_int;
    pub fn chip_memcpy_d2h(dst_host: *mut c_void, src_dev: *const c_void, size: usize, stream: *mut c_void) -> c_int;
    pub fn chip_stream_sync(stream: *mut c_void) -> c_int;

    pub fn chip_set_device(device: c_int) -> c_int;
    pub fn chip_version() -> *const c_char;
    pub fn chip_trim() -> c_int;

    pub fn chip_decoder_new(format: c_int, opts: *const chip_decoder_opts) -> *mut chip_decoder;
    pub fn chip_decode(d: *mut chip_decoder, input: *const u8, input_len: usize, output: *mut u8, output_len: usize) -> chip_decode_result;
    pub fn chip_decoder_reset(d: *mut chip_decoder) -> *mut chip_decoder;
    pub fn chip_decoder_free(d: *mut chip_decoder);
    pub fn chip_decoder_footprint(d: *const chip_decoder, pinned_bytes: *mut usize, device_bytes: *mut usize);
    pub fn chip_decoder_strerror(format: c_int, code: i32) -> *const c_char;

    // ---- the batched hot path (additive API): n independent units per launch, one wavefront per unit
    pub fn chip_decode_batch(format: c_int, n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32, out_base: *mut c_void,
                             out_off: *const u64, out_cap: *const u32, out_len: *mut u32, in_used: *mut u32, status: *mut i32, stream: *mut c_void) -> c_int;
    ///`flags`: `CHIP_F_COMPU_STATUS` makes `status[i]` compu's own reading of the codec's return code (`src/decoder/mod.rs:475-483`,
    ///`src/decoder/zstd.rs:121-133`) where the default names the cause
    pub fn chip_decode_batch_ex(format: c_int, flags: u32, n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32, out_base: *mut c_void,
                                out_off: *const u64, out_cap: *const u32, out_len: *mut u32, in_used: *mut u32, status: *mut i32, stream: *mut c_void) -> c_int;
    ///the size pass: decoded length (64-bit), input consumed and status of every unit, no output buffer; `flags` must be 0
    pub fn chip_decode_batch_sizes(format: c_int, flags: u32, n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32, out_size: *mut u64,
                                   in_used: *mut u32, status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn chip_decode_batch_host(format: c_int, n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32, out_base: *mut c_void,
                                  out_off: *const u64, out_cap: *const u32, out_len: *mut u32, in_used: *mut u32, status: *mut i32, device: c_int,
                                  slice_bytes: usize) -> c_int;
    pub fn chip_decode_batch_multi(format: c_int, n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32, out_base: *mut c_void,
                                   out_off: *const u64, out_cap: *const u32, out_len: *mut u32, in_used: *mut u32, status: *mut i32,
                                   devices: *const c_int, n_devices: c_int, slice_bytes: usize) -> c_int;
    pub fn chip_partition_units(n: usize, in_len: *const u32, out_cap: *const u32, parts: c_int, cuts: *mut usize) -> c_int;
    pub fn chip_detect(bytes: *const u8, len: usize) -> c_int;
    pub fn chip_detect_batch(n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32, kind: *mut i32, stream: *mut c_void) -> c_int;

    // ---- BGZF: the four arrays of chip_decode_batch(CHIP_FMT_GZIP, ..) from a BGZF buffer (no reference counterpart)
    ///the serial walk on host memory; pure host arithmetic, no device needed
    pub fn chip_bgzf_plan_host(input: *const u8, len: u64, max_blocks: u64, in_off: *mut u64, in_len: *mut u32, out_off: *mut u64, out_cap: *mut u32,
                               summary: *mut chip_bgzf_summary) -> c_int;
    ///the same answer for a buffer in device memory (device arrays, host summary); synchronous on `stream`
    pub fn chip_bgzf_plan(in_base: *const c_void, len: u64, max_blocks: u64, in_off: *mut u64, in_len: *mut u32, out_off: *mut u64, out_cap: *mut u32,
                          summary: *mut chip_bgzf_summary, stream: *mut c_void) -> c_int;
    ///htslib's 28-byte EOF marker (static storage)
    pub fn chip_bgzf_eof_block(len: *mut usize) -> *const u8;

    // ---- zstd frames: the four arrays of chip_decode_batch(CHIP_FMT_ZSTD, ..) from a buffer of frames (no reference counterpart)
    ///the serial walk on host memory; pure host arithmetic, no device needed
    pub fn chip_zstd_plan_host(input: *const u8, len: u64, max_frames: u64, in_off: *mut u64, in_len: *mut u32, out_off: *mut u64, out_cap: *mut u32,
                               summary: *mut chip_zstd_plan_summary) -> c_int;
    ///the same answer for a buffer in device memory (device arrays, host summary); synchronous on `stream`
    pub fn chip_zstd_plan(in_base: *const c_void, len: u64, max_frames: u64, in_off: *mut u64, in_len: *mut u32, out_off: *mut u64, out_cap: *mut u32,
                          summary: *mut chip_zstd_plan_summary, stream: *mut c_void) -> c_int;
    ///the blocks of the first frame of a host buffer and their table sources, from headers alone; pure host arithmetic
    pub fn chip_zstd_blocks_host(input: *const u8, len: u64, max_blocks: u64, blocks: *mut chip_zstd_block, summary: *mut chip_zstd_blocks_summary) -> c_int;
    ///the same answer for a buffer in device memory (device records, host summary); synchronous on `stream`
    pub fn chip_zstd_blocks(in_base: *const c_void, len: u64, max_blocks: u64, blocks: *mut chip_zstd_block, summary: *mut chip_zstd_blocks_summary,
                            stream: *mut c_void) -> c_int;
    ///one large zstd frame decoded with a wave per block (token pass, placement, pointer jumping); anything not clean is the one-unit
    ///batch decode's answer; synchronous on `stream`
    pub fn chip_zstd_parallel(in_base: *const c_void, len: u64, out_base: *mut c_void, out_cap: u64, window_log_max: c_int, flags: u32,
                              summary: *mut chip_zstd_parallel_summary, stream: *mut c_void) -> c_int;
    ///the next part of one zstd frame of any length: the same passes over a slab, from a carried cursor and its device state;
    ///synchronous on `stream`
    pub fn chip_zstd_parallel_next(cur: *mut chip_zstd_cursor, state: *mut c_void, state_cap: u64, in_base: *const c_void, len: u64, out_base: *mut c_void,
                                   out_cap: u64, window_log_max: c_int, flags: u32, summary: *mut chip_zstd_next_summary, stream: *mut c_void) -> c_int;
    ///its steps on host memory (no device needed): the walk from a block boundary, the header step, the running XXH64
    pub fn chip_zstd_slab_blocks_host(input: *const u8, len: u64, block_max: u64, max_blocks: u64, blocks: *mut chip_zstd_block,
                                      summary: *mut chip_zstd_slab_summary) -> c_int;
    pub fn chip_zstd_cursor_header_host(cur: *mut chip_zstd_cursor, input: *const u8, len: u64, window_log_max: c_int, flags: u32, header_bytes: *mut u32,
                                        need_state: *mut u64) -> c_int;
    pub fn chip_xxh64_update_host(st: *mut chip_xxh64_state, data: *const u8, len: u64) -> c_int;
    pub fn chip_xxh64_digest_host(st: *const chip_xxh64_state) -> u64;
    ///the member index of a device-resident buffer of gzip members: the size pass over every candidate start, then the chain from 0
    pub fn chip_gzip_plan(in_base: *const c_void, len: u64, max_members: u64, in_off: *mut u64, in_len: *mut u32, out_off: *mut u64, out_cap: *mut u32,
                          summary: *mut chip_gzip_plan_summary, stream: *mut c_void) -> c_int;
    ///the directory of a ZIP archive in host memory as entry records: the walk that defines the plan
    pub fn chip_zip_plan_host(input: *const u8, len: u64, max_entries: u64, entries: *mut chip_zip_entry, summary: *mut chip_zip_plan_summary) -> c_int;
    ///the same over a device-resident archive: end record search, record chain by pointer doubling, one lane per local header
    pub fn chip_zip_plan(in_base: *const c_void, len: u64, max_entries: u64, entries: *mut chip_zip_entry, summary: *mut chip_zip_plan_summary,
                         stream: *mut c_void) -> c_int;
    ///CRC-32 of many device ranges: one wave per `CHIP_CRC_PIECE` bytes, folded per range on the device
    pub fn chip_crc32_batch(n: usize, base: *const c_void, off: *const u64, len: *const u64, crc: *mut u32, stream: *mut c_void) -> c_int;
    ///selected entries of a planned archive decoded (method 8), copied (method 0) and verified against the directory's CRC-32
    pub fn chip_zip_decode(in_base: *const c_void, len: u64, entries: *const chip_zip_entry, n_entries: u64, n_sel: u64, sel: *const u32,
                           out_base: *mut c_void, out_cap: u64, out_off: *mut u64, status: *mut i32, summary: *mut chip_zip_decode_summary,
                           stream: *mut c_void) -> c_int;
    ///a ZIP archive assembled on the host from contents, names and already encoded raw deflate streams: the rules that define the writer
    pub fn chip_zip_assemble_host(n: u64, src: *const chip_zip_source, names: *const u8, names_len: u64, content: *const u8, content_len: u64,
                                  comp: *const u8, comp_all: u64, comp_off: *const u64, comp_len: *const u32, crc: *const u32, flags: u32,
                                  out: *mut u8, out_cap: u64, entries: *mut chip_zip_entry, summary: *mut chip_zip_write_summary) -> c_int;
    ///the same with every array and buffer in device memory (host `summary`): layout by two scans, records, destination-driven copies
    pub fn chip_zip_assemble(n: u64, src: *const chip_zip_source, names: *const c_void, names_len: u64, content: *const c_void, content_len: u64,
                             comp: *const c_void, comp_all: u64, comp_off: *const u64, comp_len: *const u32, crc: *const u32, flags: u32,
                             out: *mut c_void, out_cap: u64, entries: *mut chip_zip_entry, summary: *mut chip_zip_write_summary,
                             stream: *mut c_void) -> c_int;
    ///content to archive in one call: CRC-32, deflate of the eligible entries (one wave each), assembly; synchronous on `stream`
    pub fn chip_zip_write(level: c_int, flags: u32, n: u64, src: *const chip_zip_source, names: *const c_void, names_len: u64,
                          in_base: *const c_void, in_len: u64, out_base: *mut c_void, out_cap: u64, entries: *mut chip_zip_entry,
                          summary: *mut chip_zip_write_summary, stream: *mut c_void) -> c_int;
    ///the room that is always enough for `chip_zip_write`; 0 when it overflows 64 bits
    pub fn chip_zip_write_bound(n: u64, names_total: u64, content_total: u64) -> u64;
    ///the members of a tar image in host memory as entry records: the walk that defines the plan (no reference counterpart)
    pub fn chip_tar_plan_host(input: *const u8, len: u64, max_entries: u64, entries: *mut chip_tar_entry, summary: *mut chip_tar_plan_summary) -> c_int;
    ///the same over a device-resident image: one lane per 512-byte block finds the headers, one per header reads its group, the chain
    ///from 0 is marked by pointer doubling
    pub fn chip_tar_plan(in_base: *const c_void, len: u64, max_entries: u64, entries: *mut chip_tar_entry, summary: *mut chip_tar_plan_summary,
                         stream: *mut c_void) -> c_int;
    ///a tar image (pax or GNU) written on the host from contents, names and link names: the rules that define the writer
    pub fn chip_tar_write_host(n: u64, src: *const chip_tar_source, names: *const u8, names_len: u64, content: *const u8, content_len: u64,
                               flags: u32, record_bytes: u32, out: *mut u8, out_cap: u64, entries: *mut chip_tar_entry,
                               summary: *mut chip_tar_write_summary) -> c_int;
    ///the same with every array and buffer in device memory (host `summary`): check, scan, header blocks by a wave, a copy that
    ///zero-fills; synchronous on `stream`
    pub fn chip_tar_write(n: u64, src: *const chip_tar_source, names: *const c_void, names_len: u64, content: *const c_void, content_len: u64,
                          flags: u32, record_bytes: u32, out: *mut c_void, out_cap: u64, entries: *mut chip_tar_entry,
                          summary: *mut chip_tar_write_summary, stream: *mut c_void) -> c_int;
    ///the room that is always enough for `chip_tar_write`; 0 when it overflows 64 bits or `record_bytes` is refused
    pub fn chip_tar_write_bound(n: u64, names_total: u64, content_total: u64, record_bytes: u32) -> u64;
    ///from a size pass to a decode on the device: offsets (exclusive sum) and clipped capacities of `out_size`; host `total` / `n_over`
    pub fn chip_layout_units(n: usize, out_size: *const u64, out_off: *mut u64, out_cap: *mut u32, total: *mut u64, n_over: *mut u64,
                             stream: *mut c_void) -> c_int;

    pub fn chip_encoder_new(opts: *const chip_encoder_opts) -> *mut chip_encoder;
    pub fn chip_encoder_new_zstd(opts: *const chip_zstd_encoder_opts) -> *mut chip_encoder;
    pub fn chip_encoder_new_brotli(opts: *const chip_brotli_encoder_opts) -> *mut chip_encoder;
    pub fn chip_encode(e: *mut chip_encoder, input: *const u8, input_len: usize, output: *mut u8, output_len: usize, op: c_int) -> chip_encode_result;
    pub fn chip_encoder_reset(e: *mut chip_encoder) -> *mut chip_encoder;
    pub fn chip_encoder_free(e: *mut chip_encoder);
    pub fn chip_encode_batch_ex(format: c_int, level: c_int, strategy: c_int, n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32,
                                out_base: *mut c_void, out_off: *const u64, out_cap: *const u32, out_len: *mut u32, status: *mut i32,
                                stream: *mut c_void) -> c_int;
    pub fn chip_encode_batch(format: c_int, level: c_int, n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32,
                             out_base: *mut c_void, out_off: *const u64, out_cap: *const u32, out_len: *mut u32, status: *mut i32,
                             stream: *mut c_void) -> c_int;
    pub fn chip_encode_bound(format: c_int, in_len: usize) -> usize;
    pub fn chip_encode_batch_host(format: c_int, level: c_int, n: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32,
                                  out_base: *mut c_void, out_off: *const u64, out_cap: *const u32, out_len: *mut u32, status: *mut i32, device: c_int,
                                  slice_bytes: usize) -> c_int;

    // ---- writing files: encoded units end to end, and a whole BGZF / gzip / zstd file from a buffer (no reference counterpart)
    ///device ranges `src_base[src_off[i] .. + src_len[i])` end to end into `dst_base` (device arrays, host `total`); nothing is written
    ///when `total > dst_cap`; synchronous on `stream`
    pub fn chip_pack_units(n: usize, src_base: *const c_void, src_off: *const u64, src_len: *const u32, dst_base: *mut c_void, dst_cap: u64,
                           dst_off: *mut u64, total: *mut u64, stream: *mut c_void) -> c_int;
    ///cut, encode, pack, trailer: device buffers, host summary; synchronous on `stream`
    pub fn chip_encode_file(format: c_int, level: c_int, unit_bytes: u32, flags: u32, in_base: *const c_void, len: u64, out_base: *mut c_void,
                            out_cap: u64, summary: *mut chip_file_summary, stream: *mut c_void) -> c_int;
    ///the output size that is always enough; 0 for arguments `chip_encode_file` refuses
    pub fn chip_encode_file_bound(format: c_int, unit_bytes: u32, flags: u32, len: u64) -> u64;

    // ---- reading ranges: the units that byte ranges of a plan's content touch, decoded once, the ranges end to end (no reference
    // counterpart)
    ///the definition on host memory; pure host arithmetic, no device needed.  `max_sel` 0 with null `sel_*` arrays counts
    pub fn chip_select_units_host(n_units: usize, in_off: *const u64, in_len: *const u32, out_off: *const u64, out_cap: *const u32, n_ranges: usize,
                                  range_lo: *const u64, range_len: *const u32, max_sel: u64, sel_unit: *mut u32, sel_in_off: *mut u64,
                                  sel_in_len: *mut u32, sel_out_off: *mut u64, sel_out_cap: *mut u32, src_off: *mut u64, dst_off: *mut u64,
                                  range_status: *mut i32, summary: *mut chip_select_summary) -> c_int;
    ///the same answer for device arrays (host summary); synchronous on `stream`
    pub fn chip_select_units(n_units: usize, in_off: *const u64, in_len: *const u32, out_off: *const u64, out_cap: *const u32, n_ranges: usize,
                             range_lo: *const u64, range_len: *const u32, max_sel: u64, sel_unit: *mut u32, sel_in_off: *mut u64,
                             sel_in_len: *mut u32, sel_out_off: *mut u64, sel_out_cap: *mut u32, src_off: *mut u64, dst_off: *mut u64,
                             range_status: *mut i32, summary: *mut chip_select_summary, stream: *mut c_void) -> c_int;
    ///select, decode the touched units once, gather: device buffers and arrays, host summary; nothing is written when
    ///`out_len > dst_cap`; synchronous on `stream`
    pub fn chip_read_ranges(format: c_int, n_units: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32, out_off: *const u64,
                            out_cap: *const u32, n_ranges: usize, range_lo: *const u64, range_len: *const u32, dst_base: *mut c_void, dst_cap: u64,
                            dst_off: *mut u64, range_status: *mut i32, summary: *mut chip_read_summary, stream: *mut c_void) -> c_int;

    // ---- seekable zstd files: the seek table as a plan (no reference counterpart)
    ///the seek table at the end of `tail` (the last `tail_len` bytes of a file of `file_len`) as a plan: pure host arithmetic;
    ///`max_frames` 0 with null arrays counts, `checksum` may be null
    pub fn chip_zstd_seek_plan_host(tail: *const u8, tail_len: u64, file_len: u64, max_frames: u64, in_off: *mut u64, in_len: *mut u32,
                                    out_off: *mut u64, out_cap: *mut u32, checksum: *mut u32, summary: *mut chip_zstd_seek_summary) -> c_int;
    ///the same for a tail in device memory at any alignment (device arrays, host summary); synchronous on `stream`
    pub fn chip_zstd_seek_plan(tail: *const c_void, tail_len: u64, file_len: u64, max_frames: u64, in_off: *mut u64, in_len: *mut u32,
                               out_off: *mut u64, out_cap: *mut u32, checksum: *mut u32, summary: *mut chip_zstd_seek_summary,
                               stream: *mut c_void) -> c_int;
    ///a seek table of `n` entries into host memory (`checksum` null: 8-byte entries); `table_bytes` is always the exact size
    pub fn chip_zstd_seek_table_write_host(n: u64, c_len: *const u32, d_len: *const u32, checksum: *const u32, dst: *mut c_void, dst_cap: u64,
                                           table_bytes: *mut u64) -> c_int;
    ///the same from device arrays into device memory at any alignment (`table_bytes` a host pointer); only enqueues
    pub fn chip_zstd_seek_table_write(n: u64, c_len: *const u32, d_len: *const u32, checksum: *const u32, dst: *mut c_void, dst_cap: u64,
                                      table_bytes: *mut u64, stream: *mut c_void) -> c_int;
    ///XXH64 (seed 0, all 64 bits) of `n` ranges of device memory, one wave per range; only enqueues
    pub fn chip_xxh64_batch(n: usize, base: *const c_void, off: *const u64, len: *const u32, digest: *mut u64, stream: *mut c_void) -> c_int;

    // ---- LZ4: blocks and frames, decode and encode (no reference counterpart); the batch calls take CHIP_FMT_LZ4_BLOCK / CHIP_FMT_LZ4
    ///the block rules on host memory, and their definition; returns the unit's status
    pub fn chip_lz4_block_decode_host(input: *const u8, len: u64, out: *mut u8, cap: u64, out_len: *mut u64, in_used: *mut u64) -> c_int;
    ///the blocks of the first LZ4 frame of a host buffer, from headers alone; pure host arithmetic
    pub fn chip_lz4_blocks_host(input: *const u8, len: u64, max_blocks: u64, blocks: *mut chip_lz4_block, summary: *mut chip_lz4_blocks_summary) -> c_int;
    ///the same answer for a buffer in device memory (device records, host summary); synchronous on `stream`
    pub fn chip_lz4_blocks(in_base: *const c_void, len: u64, max_blocks: u64, blocks: *mut chip_lz4_block, summary: *mut chip_lz4_blocks_summary,
                           stream: *mut c_void) -> c_int;
    ///XXH32 with `seed` of many device ranges, one wave per range; only enqueues
    pub fn chip_xxh32_batch(n: usize, base: *const c_void, off: *const u64, len: *const u32, seed: u32, digest: *mut u32, stream: *mut c_void) -> c_int;
    ///one large LZ4 frame of independent blocks decoded with a wave per block; anything not clean is the one-unit decode's answer;
    ///synchronous on `stream`
    pub fn chip_lz4_parallel(in_base: *const c_void, len: u64, out_base: *mut c_void, out_cap: u64, flags: u32, summary: *mut chip_lz4_parallel_summary,
                             stream: *mut c_void) -> c_int;
    ///one raw LZ4 block of host memory on the host: the definition of the bytes the batch encoder writes; returns `CHIP_ENC_*`
    pub fn chip_lz4_block_encode_host(input: *const u8, len: u64, level: c_int, out: *mut u8, cap: u64, out_len: *mut u64) -> c_int;
    ///one LZ4 frame of host memory on the host (`strategy`: `CHIP_LZ4_S_*` bits); returns `CHIP_ENC_*`
    pub fn chip_lz4_frame_encode_host(input: *const u8, len: u64, level: c_int, strategy: c_int, out: *mut u8, cap: u64, out_len: *mut u64) -> c_int;
    // ---- Snappy: blocks and framed streams, decode only (no reference counterpart); the batch calls take CHIP_FMT_SNAPPY_BLOCK / CHIP_FMT_SNAPPY
    ///the block rules on host memory, and their definition; returns the unit's status
    pub fn chip_snappy_block_decode_host(input: *const u8, len: u64, out: *mut u8, cap: u64, out_len: *mut u64, in_used: *mut u64) -> c_int;
    ///the data chunks of a framed stream in a host buffer, from the chunk headers alone; pure host arithmetic
    pub fn chip_snappy_chunks_host(input: *const u8, len: u64, max_chunks: u64, chunks: *mut chip_snappy_chunk, summary: *mut chip_snappy_chunks_summary) -> c_int;
    ///the same answer for a buffer in device memory (device records, host summary); synchronous on `stream`
    pub fn chip_snappy_chunks(in_base: *const c_void, len: u64, max_chunks: u64, chunks: *mut chip_snappy_chunk, summary: *mut chip_snappy_chunks_summary,
                              stream: *mut c_void) -> c_int;
    ///CRC-32C (Castagnoli), unmasked, of many device ranges, one wave per range; only enqueues
    pub fn chip_crc32c_batch(n: usize, base: *const c_void, off: *const u64, len32: *const u32, crc: *mut u32, stream: *mut c_void) -> c_int;
    ///one framed Snappy stream decoded with a wave per chunk; anything not clean is the one-unit decode's answer; synchronous on `stream`
    pub fn chip_snappy_parallel(in_base: *const c_void, len: u64, out_base: *mut c_void, out_cap: u64, flags: u32, summary: *mut chip_snappy_parallel_summary,
                                stream: *mut c_void) -> c_int;
    ///`chip_read_ranges(CHIP_FMT_ZSTD, ..)` with the seek table's per-unit checksums verified on the device (`checksum` null: that
    ///call itself); synchronous on `stream`
    pub fn chip_zstd_seek_read(n_units: usize, in_base: *const c_void, in_off: *const u64, in_len: *const u32, out_off: *const u64,
                               out_cap: *const u32, checksum: *const u32, n_ranges: usize, range_lo: *const u64, range_len: *const u32,
                               dst_base: *mut c_void, dst_cap: u64, dst_off: *mut u64, range_status: *mut i32, summary: *mut chip_read_summary,
                               stream: *mut c_void) -> c_int;

    // ---- one large stream: the checkpoint index of a gzip / zlib / raw deflate stream (no reference counterpart)
    ///decode the one unit and record a point every `spacing` decoded bytes (0 = 1 MiB): device buffers and arrays, host summary;
    ///`max_points` 0 with null arrays is the plain decode with a count; synchronous on `stream`
    pub fn chip_inflate_index_build(format: c_int, in_base: *const c_void, len: u64, out_base: *mut c_void, out_cap: u64, spacing: u32, max_points: u64,
                                    pt_bit: *mut u64, pt_out: *mut u64, pt_check: *mut u32, windows: *mut c_void,
                                    summary: *mut chip_inflate_index_summary, stream: *mut c_void) -> c_int;
    ///the chunks of an index on host memory: pure host arithmetic, no device needed; every output array may be null
    pub fn chip_inflate_index_units_host(format: c_int, len: u64, n_points: u64, pt_bit: *const u64, pt_out: *const u64, pt_check: *const u32,
                                         total_out: u64, in_off: *mut u64, in_len: *mut u32, out_cap: *mut u32, win_len: *mut u32, resume: *mut u32,
                                         status: *mut i32, bad_index: *mut u64) -> c_int;
    ///`chip_read_ranges` over the chunks of an index: each touched chunk is decoded once as a resumed unit and verified against
    ///the next point's check value; synchronous on `stream`
    pub fn chip_inflate_index_read(format: c_int, in_base: *const c_void, len: u64, n_points: u64, pt_bit: *const u64, pt_out: *const u64,
                                   pt_check: *const u32, windows: *const c_void, total_out: u64, n_ranges: usize, range_lo: *const u64,
                                   range_len: *const u32, dst_base: *mut c_void, dst_cap: u64, dst_off: *mut u64, range_status: *mut i32,
                                   summary: *mut chip_read_summary, stream: *mut c_void) -> c_int;
    ///the block starts of one deflate stream in host memory: per chunk behind the first, the least bit position where a dynamic
    ///block header the decoder accepts begins; pure host arithmetic; `max` 0 with a null array counts
    pub fn chip_inflate_find_starts_host(input: *const u8, len: u64, first_bit: u64, chunk_bytes: u32, max: u64, starts: *mut u64,
                                         n: *mut u64) -> c_int;
    ///the same for a buffer in device memory (`starts` a device array, `n` a host pointer); synchronous on `stream`
    pub fn chip_inflate_find_starts(in_base: *const c_void, len: u64, first_bit: u64, chunk_bytes: u32, max: u64, starts: *mut u64, n: *mut u64,
                                    stream: *mut c_void) -> c_int;
    ///ONE stream decoded by the whole GPU, a wave per chunk with a block start, with the checkpoint index as a by-product; arguments as
    ///`chip_inflate_index_build`, `chunk_bytes` 0 = the default; synchronous on `stream`
    pub fn chip_inflate_parallel(format: c_int, in_base: *const c_void, len: u64, out_base: *mut c_void, out_cap: u64, chunk_bytes: u32, max_points: u64,
                                 pt_bit: *mut u64, pt_out: *mut u64, pt_check: *mut u32, windows: *mut c_void,
                                 summary: *mut chip_inflate_parallel_summary, stream: *mut c_void) -> c_int;
    pub fn chip_inflate_parallel_next(format: c_int, cur: *mut chip_inflate_cursor, window: *mut c_void, in_base: *const c_void, len: u64,
                                      out_base: *mut c_void, out_cap: u64, chunk_bytes: u32, summary: *mut chip_inflate_next_summary,
                                      stream: *mut c_void) -> c_int;
}
