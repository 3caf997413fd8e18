//! `hip` interface implementation: zlib / gzip / raw deflate, zstd and brotli decoding on an MI355X through `libcompu_hip.so`.
//!
//! Same shape as `zlib_ng.rs`: one static vtable per format family, the state pointer is the backend's opaque
//! decoder object, created by the constructor and freed exactly once by `drop_fn`.

extern crate alloc;

use core::ptr;

use super::zlib_common::ZlibMode;
use super::zstd::ZstdOptions;
use super::{Decode, DecodeError, DecodeStatus, Decoder, Interface};
use crate::hip_sys as sys;

static HIP_ZLIB: Interface = Interface {
    drop_fn,
    reset_fn,
    decode_fn,
    describe_error_fn: describe_zlib_error_fn,
};

static HIP_ZSTD: Interface = Interface {
    drop_fn,
    reset_fn,
    decode_fn,
    describe_error_fn: describe_zstd_error_fn,
};

static HIP_BROTLI: Interface = Interface {
    drop_fn,
    reset_fn,
    decode_fn,
    describe_error_fn: describe_brotli_error_fn,
};

impl Interface {
    ///Creates decoder with `hip` interface for zlib family of formats (same modes as `zlib_ng`).
    ///
    ///Returns `None` if unable to initialize it (no usable GPU, or lack of memory)
    pub fn zlib_hip(mode: ZlibMode) -> Option<Decoder> {
        crate::mem::hip_install_allocator();
        let opts = sys::chip_decoder_opts {
            window_log_max: 0,
            device: -1,
        };
        //`ZlibMode::max_bits()` is zlib's windowBits value (-15 / 15 / 31 / 47), which is the backend's format tag
        let instance = unsafe { sys::chip_decoder_new(mode.max_bits() as _, &opts) };
        ptr::NonNull::new(instance as *mut u8).map(|instance| HIP_ZLIB.inner_decoder(instance))
    }

    ///Creates decoder with `hip` interface for zstd.
    ///
    ///Returns `None` if unable to initialize it (no usable GPU, or lack of memory)
    pub fn zstd_hip(opts: ZstdOptions) -> Option<Decoder> {
        crate::mem::hip_install_allocator();
        let opts = sys::chip_decoder_opts {
            //`window_log` is private to `zstd.rs`; the maintainer adds `pub(super) const fn window_log_max(&self) -> i32`
            //next to `ZstdOptions::apply` (src/decoder/zstd.rs:50-74)
            window_log_max: opts.window_log_max(),
            device: -1,
        };
        let instance = unsafe { sys::chip_decoder_new(sys::CHIP_FMT_ZSTD, &opts) };
        ptr::NonNull::new(instance as *mut u8).map(|instance| HIP_ZSTD.inner_decoder(instance))
    }

    ///Creates decoder with `hip` interface for brotli (the counterpart of `brotli_c`).
    ///
    ///Returns `None` if unable to initialize it (no usable GPU, or lack of memory)
    pub fn brotli_hip() -> Option<Decoder> {
        crate::mem::hip_install_allocator();
        let opts = sys::chip_decoder_opts {
            window_log_max: 0,
            device: -1,
        };
        let instance = unsafe { sys::chip_decoder_new(sys::CHIP_FMT_BROTLI, &opts) };
        ptr::NonNull::new(instance as *mut u8).map(|instance| HIP_BROTLI.inner_decoder(instance))
    }
}

#[inline]
unsafe fn decode_fn(state: ptr::NonNull<u8>, input: *const u8, input_remain: usize, output: *mut u8, output_remain: usize) -> Decode {
    let result = sys::chip_decode(state.as_ptr() as *mut sys::chip_decoder, input, input_remain, output, output_remain);
    Decode {
        input_remain: result.input_remain,
        output_remain: result.output_remain,
        status: match result.err {
            0 => Ok(match result.status {
                0 => DecodeStatus::NeedInput,
                1 => DecodeStatus::NeedOutput,
                _ => DecodeStatus::Finished,
            }),
            //same codes as the CPU backends: zlib's negative return values, -(ZSTD_ErrorCode), BrotliDecoderErrorCode
            code => Err(DecodeError(code)),
        },
    }
}

#[inline]
fn reset_fn(state: ptr::NonNull<u8>) -> Option<ptr::NonNull<u8>> {
    let result = unsafe { sys::chip_decoder_reset(state.as_ptr() as *mut sys::chip_decoder) };
    ptr::NonNull::new(result as *mut u8)
}

#[inline]
fn drop_fn(state: ptr::NonNull<u8>) {
    unsafe {
        sys::chip_decoder_free(state.as_ptr() as *mut sys::chip_decoder);
    }
}

#[inline]
fn describe_zlib_error_fn(code: i32) -> Option<&'static str> {
    let result = unsafe { sys::chip_decoder_strerror(ZlibMode::Auto.max_bits() as _, code) };
    crate::utils::convert_c_str(result)
}

#[inline]
fn describe_zstd_error_fn(code: i32) -> Option<&'static str> {
    let result = unsafe { sys::chip_decoder_strerror(sys::CHIP_FMT_ZSTD, code) };
    crate::utils::convert_c_str(result)
}

#[inline]
fn describe_brotli_error_fn(code: i32) -> Option<&'static str> {
    //BrotliDecoderErrorString's names, src/decoder/brotli_c.rs (describe_error_fn)
    let result = unsafe { sys::chip_decoder_strerror(sys::CHIP_FMT_BROTLI, code) };
    crate::utils::convert_c_str(result)
}

// ---- the batched hot path ------------------------------------------------------------------------------------
//
// compu's `Decoder` decodes one stream per call.  The MI355X backend earns its keep on BATCHES of independent units (one
// wavefront per unit, one launch per batch): these free functions are the safe face of `chip_decode_batch*`.  They sit
// beside the vtable of src/decoder/mod.rs:160-166 and do, per unit, what the loop
// `Interface::zlib_ng(mode)` -> `decode` -> `reset` (src/decoder/zlib_ng.rs:61-108) does on the CPU.

///One unit of a batch: where its compressed bytes lie in the input buffer and where its output goes.
#[derive(Clone, Copy, Debug)]
pub struct BatchUnit {
    ///offset of the unit's first compressed byte in the input buffer
    pub in_off: u64,
    ///compressed length
    pub in_len: u32,
    ///offset of the unit's output range in the output buffer
    pub out_off: u64,
    ///capacity of that range
    pub out_cap: u32,
}

///What the backend reports per unit.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct BatchResult {
    ///bytes written
    pub out_len: u32,
    ///input bytes consumed
    pub in_used: u32,
    ///`Ok(status)` or the codec's error code, as `Decode::status`
    pub status: Result<DecodeStatus, DecodeError>,
}

///Batch format: one of `ZlibMode`'s window-bits values, zstd, or per-unit routing by `Detection::detect`.
///
///(`ZlibMode` derives only `Copy` and `Clone`, src/decoder/zlib_common.rs:1, so `Debug` is written by hand.)
#[derive(Clone, Copy)]
pub enum BatchFormat {
    ///raw deflate / zlib / gzip / zlib-or-gzip, as `Interface::zlib_hip(mode)`
    Zlib(ZlibMode),
    ///zstd frames
    Zstd,
    ///brotli streams (not part of `Detect`: compu cannot detect brotli)
    Brotli,
    ///gzip, zlib and zstd units mixed: each unit goes where `Detection::detect` sends it (src/decoder/mod.rs:28-114)
    Detect,
}

impl core::fmt::Debug for BatchFormat {
    fn fmt(&self, f: &mut core::fmt::Formatter<'_>) -> core::fmt::Result {
        match self {
            BatchFormat::Zlib(mode) => write!(f, "Zlib({})", mode.max_bits()),
            BatchFormat::Zstd => f.write_str("Zstd"),
            BatchFormat::Brotli => f.write_str("Brotli"),
            BatchFormat::Detect => f.write_str("Detect"),
        }
    }
}

impl BatchFormat {
    fn tag(self) -> core::ffi::c_int {
        match self {
            BatchFormat::Zlib(mode) => mode.max_bits() as _,
            BatchFormat::Zstd => sys::CHIP_FMT_ZSTD,
            BatchFormat::Brotli => sys::CHIP_FMT_BROTLI,
            BatchFormat::Detect => sys::CHIP_FMT_DETECT,
        }
    }
}

fn map_status(status: i32) -> Result<DecodeStatus, DecodeError> {
    match status {
        0 => Ok(DecodeStatus::NeedInput),
        1 => Ok(DecodeStatus::NeedOutput),
        2 => Ok(DecodeStatus::Finished),
        code => Err(DecodeError(code)),
    }
}

///Decodes `units` of `input` into `output`, both in HOST memory (pinned memory -- `crate::buffer::PinnedBuffer` -- lets the copies
///overlap the kernels), on `device`.
///
///Returns the backend's error code when the launch itself failed; per-unit outcomes are in the returned vector.
pub fn decode_batch_host(format: BatchFormat, device: i32, input: &[u8], units: &[BatchUnit], output: &mut [u8]) -> Result<alloc::vec::Vec<BatchResult>, i32> {
    let n = units.len();
    for unit in units {
        //the backend trusts offsets and lengths: check them here, once, on the safe side of the boundary
        let in_end = unit.in_off.checked_add(unit.in_len as u64).ok_or(-101)?;
        let out_end = unit.out_off.checked_add(unit.out_cap as u64).ok_or(-101)?;
        if in_end > input.len() as u64 || out_end > output.len() as u64 {
            return Err(-101);
        }
    }
    let in_off: alloc::vec::Vec<u64> = units.iter().map(|u| u.in_off).collect();
    let in_len: alloc::vec::Vec<u32> = units.iter().map(|u| u.in_len).collect();
    let out_off: alloc::vec::Vec<u64> = units.iter().map(|u| u.out_off).collect();
    let out_cap: alloc::vec::Vec<u32> = units.iter().map(|u| u.out_cap).collect();
    let mut out_len = alloc::vec![0u32; n];
    let mut in_used = alloc::vec![0u32; n];
    let mut status = alloc::vec![0i32; n];
    let rc = unsafe {
        sys::chip_decode_batch_host(format.tag(), n, input.as_ptr() as *const _, in_off.as_ptr(), in_len.as_ptr(), output.as_mut_ptr() as *mut _,
                                    out_off.as_ptr(), out_cap.as_ptr(), out_len.as_mut_ptr(), in_used.as_mut_ptr(), status.as_mut_ptr(), device, 0)
    };
    if rc != sys::CHIP_OK {
        return Err(rc);
    }
    Ok((0..n).map(|i| BatchResult { out_len: out_len[i], in_used: in_used[i], status: map_status(status[i]) }).collect())
}

///The same over every visible GPU of the node (or `devices`): the units are partitioned on the host, no collective.
pub fn decode_batch_multi(format: BatchFormat, devices: &[i32], input: &[u8], units: &[BatchUnit], output: &mut [u8]) -> Result<alloc::vec::Vec<BatchResult>, i32> {
    let n = units.len();
    for unit in units {
        let in_end = unit.in_off.checked_add(unit.in_len as u64).ok_or(-101)?;
        let out_end = unit.out_off.checked_add(unit.out_cap as u64).ok_or(-101)?;
        if in_end > input.len() as u64 || out_end > output.len() as u64 {
            return Err(-101);
        }
    }
    let in_off: alloc::vec::Vec<u64> = units.iter().map(|u| u.in_off).collect();
    let in_len: alloc::vec::Vec<u32> = units.iter().map(|u| u.in_len).collect();
    let out_off: alloc::vec::Vec<u64> = units.iter().map(|u| u.out_off).collect();
    let out_cap: alloc::vec::Vec<u32> = units.iter().map(|u| u.out_cap).collect();
    let mut out_len = alloc::vec![0u32; n];
    let mut in_used = alloc::vec![0u32; n];
    let mut status = alloc::vec![0i32; n];
    let rc = unsafe {
        sys::chip_decode_batch_multi(format.tag(), n, input.as_ptr() as *const _, in_off.as_ptr(), in_len.as_ptr(), output.as_mut_ptr() as *mut _,
                                     out_off.as_ptr(), out_cap.as_ptr(), out_len.as_mut_ptr(), in_used.as_mut_ptr(), status.as_mut_ptr(),
                                     if devices.is_empty() { ptr::null() } else { devices.as_ptr() }, devices.len() as _, 0)
    };
    if rc != sys::CHIP_OK {
        return Err(rc);
    }
    Ok((0..n).map(|i| BatchResult { out_len: out_len[i], in_used: in_used[i], status: map_status(status[i]) }).collect())
}

///Device-resident batch: everything -- data, offsets, results -- already lies in `DeviceBuffer`s (src/buffer.rs grows them, see
///`buffer_hip.rs`); the call only enqueues one launch on `stream` (null = default stream).
///
///# Safety
///
///The offset / length arrays are read by the GPU: they must describe ranges inside `input` and `output`, and all buffers must
///stay alive until the stream has been synchronised.
///
///`compu_status`: report every unit's status exactly as this crate's `decode_fn` would have (`CHIP_F_COMPU_STATUS`); `false` names the
///limit that was hit (see `include/compu_hip.h`).
pub unsafe fn decode_batch_device(format: BatchFormat, compu_status: bool, n: usize, input: &crate::buffer::DeviceBuffer, in_off: &crate::buffer::DeviceBuffer,
                                  in_len: &crate::buffer::DeviceBuffer, output: &mut crate::buffer::DeviceBuffer, out_off: &crate::buffer::DeviceBuffer,
                                  out_cap: &crate::buffer::DeviceBuffer, out_len: &mut crate::buffer::DeviceBuffer, in_used: &mut crate::buffer::DeviceBuffer,
                                  status: &mut crate::buffer::DeviceBuffer, stream: *mut core::ffi::c_void) -> Result<(), i32> {
    if in_off.capacity() < 8 * n || out_off.capacity() < 8 * n || in_len.capacity() < 4 * n || out_cap.capacity() < 4 * n || out_len.capacity() < 4 * n
        || in_used.capacity() < 4 * n || status.capacity() < 4 * n
    {
        return Err(-101);
    }
    let flags = if compu_status { sys::CHIP_F_COMPU_STATUS } else { 0 };
    let rc = sys::chip_decode_batch_ex(format.tag(), flags, n, input.as_ptr() as *const _, in_off.as_ptr() as *const u64, in_len.as_ptr() as *const u32,
                                       output.as_mut_ptr() as *mut _, out_off.as_ptr() as *const u64, out_cap.as_ptr() as *const u32,
                                       out_len.as_mut_ptr() as *mut u32, in_used.as_mut_ptr() as *mut u32, status.as_mut_ptr() as *mut i32, stream);
    if rc == sys::CHIP_OK { Ok(()) } else { Err(rc) }
}

///The size pass (`chip_decode_batch_sizes`): the decoded length of every unit of a device-resident batch without decoding it --
///`out_size[i]` (u64), `in_used[i]`, `status[i]` -- so that `decode_batch_device` can be given an `out_cap[i]` that is enough.
///No counterpart in this crate: it replaces the grow-and-retry loop a batch caller would write around `decode_vec`
///(`src/decoder/mod.rs:323-335`).  Every `BatchFormat` but `Brotli` (`Err(-101)`).
///
///# Safety
///
///As `decode_batch_device`.
pub unsafe fn decode_batch_sizes_device(format: BatchFormat, n: usize, input: &crate::buffer::DeviceBuffer, in_off: &crate::buffer::DeviceBuffer,
                                        in_len: &crate::buffer::DeviceBuffer, out_size: &mut crate::buffer::DeviceBuffer,
                                        in_used: &mut crate::buffer::DeviceBuffer, status: &mut crate::buffer::DeviceBuffer,
                                        stream: *mut core::ffi::c_void) -> Result<(), i32> {
    if in_off.capacity() < 8 * n || in_len.capacity() < 4 * n || out_size.capacity() < 8 * n || in_used.capacity() < 4 * n || status.capacity() < 4 * n {
        return Err(-101);
    }
    let rc = sys::chip_decode_batch_sizes(format.tag(), 0, n, input.as_ptr() as *const _, in_off.as_ptr() as *const u64, in_len.as_ptr() as *const u32,
                                          out_size.as_mut_ptr() as *mut u64, in_used.as_mut_ptr() as *mut u32, status.as_mut_ptr() as *mut i32, stream);
    if rc == sys::CHIP_OK { Ok(()) } else { Err(rc) }
}

///`Detection::detect` for every unit of a device-resident batch (`kind[i]` gets the backend's CHIP_DETECT_* value).
///
///# Safety
///
///As `decode_batch_device`.
pub unsafe fn detect_batch_device(n: usize, input: &crate::buffer::DeviceBuffer, in_off: &crate::buffer::DeviceBuffer, in_len: &crate::buffer::DeviceBuffer,
                                  kind: &mut crate::buffer::DeviceBuffer, stream: *mut core::ffi::c_void) -> Result<(), i32> {
    if in_off.capacity() < 8 * n || in_len.capacity() < 4 * n || kind.capacity() < 4 * n {
        return Err(-101);
    }
    let rc = sys::chip_detect_batch(n, input.as_ptr() as *const _, in_off.as_ptr() as *const u64, in_len.as_ptr() as *const u32,
                                    kind.as_mut_ptr() as *mut i32, stream);
    if rc == sys::CHIP_OK { Ok(()) } else { Err(rc) }
}

///The partition `decode_batch_multi` uses: `parts + 1` cut points, worker `w` owns units `cuts[w]..cuts[w + 1]`.
pub fn partition_units(in_len: &[u32], out_cap: &[u32], parts: usize) -> Option<alloc::vec::Vec<usize>> {
    if in_len.len() != out_cap.len() || parts == 0 {
        return None;
    }
    let mut cuts = alloc::vec![0usize; parts + 1];
    let rc = unsafe { sys::chip_partition_units(in_len.len(), in_len.as_ptr(), out_cap.as_ptr(), parts as _, cuts.as_mut_ptr()) };
    if rc == sys::CHIP_OK { Some(cuts) } else { None }
}

///The frame index of a buffer of zstd frames in host memory (`chip_zstd_plan_host`): `(in_off, in_len, out_off, out_cap)` of every
///data frame -- what `decode_batch_host` / `decode_batch_multi` take with `BatchFormat::Zstd` once no `out_cap` is
///`CHIP_ZPLAN_UNSIZED` -- and the summary of the walk.  Pure host arithmetic.  No counterpart in this crate.
#[allow(clippy::type_complexity)]
pub fn zstd_plan_host(input: &[u8]) -> Result<(alloc::vec::Vec<u64>, alloc::vec::Vec<u32>, alloc::vec::Vec<u64>, alloc::vec::Vec<u32>, sys::chip_zstd_plan_summary), i32> {
    let mut summary = sys::chip_zstd_plan_summary::default();
    let rc = unsafe { sys::chip_zstd_plan_host(input.as_ptr(), input.len() as u64, 0, ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), &mut summary) };
    if rc != sys::CHIP_OK {
        return Err(rc);
    }
    let n = summary.n_frames as usize;
    let (mut in_off, mut in_len, mut out_off, mut out_cap) = (alloc::vec![0u64; n], alloc::vec![0u32; n], alloc::vec![0u64; n], alloc::vec![0u32; n]);
    let rc = unsafe {
        sys::chip_zstd_plan_host(input.as_ptr(), input.len() as u64, n as u64, in_off.as_mut_ptr(), in_len.as_mut_ptr(), out_off.as_mut_ptr(),
                                 out_cap.as_mut_ptr(), &mut summary)
    };
    if rc == sys::CHIP_OK { Ok((in_off, in_len, out_off, out_cap, summary)) } else { Err(rc) }
}

///`chip_zstd_plan` over the first `len` bytes of a device-resident buffer: fills the four device arrays for the first
///`max_frames` frames and returns the summary of the whole walk (`max_frames` 0 counts).  Synchronous on `stream`.
///
///# Safety
///
///As `decode_batch_device`; `input` must be 4-byte aligned and padded to a multiple of 4 bytes.
pub unsafe fn zstd_plan_device(input: &crate::buffer::DeviceBuffer, len: usize, max_frames: usize, in_off: &mut crate::buffer::DeviceBuffer,
                               in_len: &mut crate::buffer::DeviceBuffer, out_off: &mut crate::buffer::DeviceBuffer, out_cap: &mut crate::buffer::DeviceBuffer,
                               stream: *mut core::ffi::c_void) -> Result<sys::chip_zstd_plan_summary, i32> {
    if len > input.capacity() || in_off.capacity() < 8 * max_frames || out_off.capacity() < 8 * max_frames || in_len.capacity() < 4 * max_frames
        || out_cap.capacity() < 4 * max_frames
    {
        return Err(-101);
    }
    let mut summary = sys::chip_zstd_plan_summary::default();
    let rc = sys::chip_zstd_plan(input.as_ptr() as *const _, len as u64, max_frames as u64, in_off.as_mut_ptr() as *mut u64, in_len.as_mut_ptr() as *mut u32,
                                 out_off.as_mut_ptr() as *mut u64, out_cap.as_mut_ptr() as *mut u32, &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///The blocks of the first zstd frame of a buffer in host memory (`chip_zstd_blocks_host`): where each block lies, its type, a
///compressed block's section headers and, per table kind, the nearest earlier block that defined the table it may reuse (-1: none);
///and the summary of the walk.  Read from headers alone, nothing is decoded.  Pure host arithmetic.  No counterpart in this crate.
pub fn zstd_blocks_host(input: &[u8]) -> Result<(alloc::vec::Vec<sys::chip_zstd_block>, sys::chip_zstd_blocks_summary), i32> {
    let mut summary = sys::chip_zstd_blocks_summary::default();
    let rc = unsafe { sys::chip_zstd_blocks_host(input.as_ptr(), input.len() as u64, 0, ptr::null_mut(), &mut summary) };
    if rc != sys::CHIP_OK {
        return Err(rc);
    }
    let n = summary.n_blocks as usize;
    let mut blocks = alloc::vec![sys::chip_zstd_block::default(); n];
    let rc = unsafe { sys::chip_zstd_blocks_host(input.as_ptr(), input.len() as u64, n as u64, blocks.as_mut_ptr(), &mut summary) };
    if rc == sys::CHIP_OK { Ok((blocks, summary)) } else { Err(rc) }
}

///`chip_zstd_blocks` over the first `len` bytes of a device-resident buffer that begins with a zstd frame: fills `blocks` (device
///memory, 48 bytes per `chip_zstd_block`) for the first `max_blocks` blocks and returns the summary of the whole walk (`max_blocks`
///0 counts).  Synchronous on `stream`.
///
///# Safety
///
///As `decode_batch_device`; `input` must be 4-byte aligned and padded to a multiple of 4 bytes.
pub unsafe fn zstd_blocks_device(input: &crate::buffer::DeviceBuffer, len: usize, max_blocks: usize, blocks: &mut crate::buffer::DeviceBuffer,
                                 stream: *mut core::ffi::c_void) -> Result<sys::chip_zstd_blocks_summary, i32> {
    if len > input.capacity() || blocks.capacity() < core::mem::size_of::<sys::chip_zstd_block>() * max_blocks {
        return Err(-101);
    }
    let mut summary = sys::chip_zstd_blocks_summary::default();
    let rc = sys::chip_zstd_blocks(input.as_ptr() as *const _, len as u64, max_blocks as u64, blocks.as_mut_ptr() as *mut sys::chip_zstd_block, &mut summary,
                                   stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///`chip_zstd_parallel`: the first zstd frame of the first `len` bytes of `input` decoded into `output` with a wave per block; the
///summary carries the batch decode's `out_len`, `in_used` and `status`, the exact size on `NeedOutput` and the path taken.
///`flags`: `CHIP_ZPAR_NO_CHECKSUM`.  Synchronous on `stream`.
///
///# Safety
///
///As `decode_batch_device`; `input` must be 4-byte aligned and padded to a multiple of 4 bytes.
pub unsafe fn zstd_parallel_device(input: &crate::buffer::DeviceBuffer, len: usize, output: &mut crate::buffer::DeviceBuffer, window_log_max: i32, flags: u32,
                                   stream: *mut core::ffi::c_void) -> Result<sys::chip_zstd_parallel_summary, i32> {
    if len > input.capacity() {
        return Err(-101);
    }
    let mut summary = sys::chip_zstd_parallel_summary::default();
    let rc = sys::chip_zstd_parallel(input.as_ptr() as *const _, len as u64, output.as_mut_ptr() as *mut _, output.capacity() as u64, window_log_max, flags,
                                     &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///`chip_zstd_parallel_next`: decodes the next part of one zstd frame of any length.  `slab` holds `len` bytes of the frame from byte
///`cursor.in_total` on, `state` the carried table definers and the window ring (`summary.need_state` says how large it must be once
///the frame header is read); the call delivers whole blocks into `output` while they fit, moves the cursor to a later block boundary
///(or through the checksum) and says in the summary how many bytes of the slab lie in front of the new cursor, how many bytes it
///delivered and why it stopped.  `flags`: `CHIP_ZPAR_NO_CHECKSUM`, the same in every call of a frame.  Synchronous on `stream`.
///No counterpart in this crate.
///
///# Safety
///
///As `decode_batch_device`; `state` must be the one the cursor was left with.
pub unsafe fn zstd_parallel_next_device(cursor: &mut sys::chip_zstd_cursor, state: &mut crate::buffer::DeviceBuffer, slab: &crate::buffer::DeviceBuffer,
                                        len: usize, output: &mut crate::buffer::DeviceBuffer, window_log_max: i32, flags: u32,
                                        stream: *mut core::ffi::c_void) -> Result<sys::chip_zstd_next_summary, i32> {
    if len > slab.capacity() || state.capacity() < sys::CHIP_ZCUR_CARRY_BYTES {
        return Err(-101);
    }
    let mut summary = sys::chip_zstd_next_summary::default();
    let cap = core::cmp::min(output.capacity() as u64, (1u64 << 31) - 1);
    let rc = sys::chip_zstd_parallel_next(cursor, state.as_mut_ptr() as *mut _, state.capacity() as u64, slab.as_ptr() as *const _, len as u64,
                                          output.as_mut_ptr() as *mut _, cap, window_log_max, flags, &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///`chip_gzip_plan` over the first `len` bytes of a device-resident buffer of gzip members (WARC records, `cat a.gz b.gz`, what
///`encode_file_device` writes for gzip): fills the four device arrays for the first `max_members` members -- what
///`decode_batch_device` takes with `BatchFormat::Zlib` in gzip mode -- and returns the summary of the whole walk (`max_members` 0 counts).
///Synchronous on `stream`.  There is no host form: finding a member's end is an inflate.
///
///# Safety
///
///As `decode_batch_device`; `input` must be 4-byte aligned and padded to a multiple of 4 bytes.
pub unsafe fn gzip_plan_device(input: &crate::buffer::DeviceBuffer, len: usize, max_members: usize, in_off: &mut crate::buffer::DeviceBuffer,
                               in_len: &mut crate::buffer::DeviceBuffer, out_off: &mut crate::buffer::DeviceBuffer, out_cap: &mut crate::buffer::DeviceBuffer,
                               stream: *mut core::ffi::c_void) -> Result<sys::chip_gzip_plan_summary, i32> {
    if len > input.capacity() || in_off.capacity() < 8 * max_members || out_off.capacity() < 8 * max_members || in_len.capacity() < 4 * max_members
        || out_cap.capacity() < 4 * max_members
    {
        return Err(-101);
    }
    let mut summary = sys::chip_gzip_plan_summary::default();
    let rc = sys::chip_gzip_plan(input.as_ptr() as *const _, len as u64, max_members as u64, in_off.as_mut_ptr() as *mut u64, in_len.as_mut_ptr() as *mut u32,
                                 out_off.as_mut_ptr() as *mut u64, out_cap.as_mut_ptr() as *mut u32, &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///`chip_layout_units`: from the `out_size` of `decode_batch_sizes_device` to the `out_off` / `out_cap` of `decode_batch_device`
///without a host round trip per unit.  Returns `(total, n_over)`: the bytes to allocate and the units above 4 GiB - 1.
///Synchronous on `stream`.
///
///# Safety
///
///As `decode_batch_device`.
pub unsafe fn layout_units_device(n: usize, out_size: &crate::buffer::DeviceBuffer, out_off: &mut crate::buffer::DeviceBuffer,
                                  out_cap: &mut crate::buffer::DeviceBuffer, stream: *mut core::ffi::c_void) -> Result<(u64, u64), i32> {
    if out_size.capacity() < 8 * n || out_off.capacity() < 8 * n || out_cap.capacity() < 4 * n {
        return Err(-101);
    }
    let (mut total, mut n_over) = (0u64, 0u64);
    let rc = sys::chip_layout_units(n, out_size.as_ptr() as *const u64, out_off.as_mut_ptr() as *mut u64, out_cap.as_mut_ptr() as *mut u32, &mut total,
                                    &mut n_over, stream);
    if rc == sys::CHIP_OK { Ok((total, n_over)) } else { Err(rc) }
}

///What `select_units_host` answers: the sub-batch of the selected units (`sel_unit` their indices in the plan), `src_off` /
///`dst_off` / `range_status` per range, and the summary.
#[derive(Clone, Debug, Default)]
pub struct Selection {
    pub sel_unit: alloc::vec::Vec<u32>,
    pub sel_in_off: alloc::vec::Vec<u64>,
    pub sel_in_len: alloc::vec::Vec<u32>,
    pub sel_out_off: alloc::vec::Vec<u64>,
    pub sel_out_cap: alloc::vec::Vec<u32>,
    pub src_off: alloc::vec::Vec<u64>,
    pub dst_off: alloc::vec::Vec<u64>,
    pub range_status: alloc::vec::Vec<i32>,
    pub summary: sys::chip_select_summary,
}

///The units that the byte ranges `(range_lo[r], range_len[r])` of a plan's decoded content touch (`chip_select_units_host`): one
///call to count, one to fill.  On `CHIP_READ_BAD_LAYOUT` the arrays are empty.  Pure host arithmetic.  No counterpart in this
///crate.
pub fn select_units_host(in_off: &[u64], in_len: &[u32], out_off: &[u64], out_cap: &[u32], range_lo: &[u64], range_len: &[u32]) -> Result<Selection, i32> {
    let (n, m) = (out_cap.len(), range_len.len());
    if in_off.len() != n || in_len.len() != n || out_off.len() != n || range_lo.len() != m {
        return Err(-101);
    }
    let mut s = Selection::default();
    let rc = unsafe {
        sys::chip_select_units_host(n, in_off.as_ptr(), in_len.as_ptr(), out_off.as_ptr(), out_cap.as_ptr(), m, range_lo.as_ptr(), range_len.as_ptr(), 0,
                                    ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut(),
                                    ptr::null_mut(), ptr::null_mut(), &mut s.summary)
    };
    if rc != sys::CHIP_OK {
        return Err(rc);
    }
    if s.summary.status != sys::CHIP_READ_OK {
        return Ok(s);
    }
    let k = s.summary.n_sel as usize;
    s.sel_unit = alloc::vec![0u32; k];
    s.sel_in_off = alloc::vec![0u64; k];
    s.sel_in_len = alloc::vec![0u32; k];
    s.sel_out_off = alloc::vec![0u64; k];
    s.sel_out_cap = alloc::vec![0u32; k];
    s.src_off = alloc::vec![0u64; m];
    s.dst_off = alloc::vec![0u64; m];
    s.range_status = alloc::vec![0i32; m];
    let rc = unsafe {
        sys::chip_select_units_host(n, in_off.as_ptr(), in_len.as_ptr(), out_off.as_ptr(), out_cap.as_ptr(), m, range_lo.as_ptr(), range_len.as_ptr(),
                                    k as u64, s.sel_unit.as_mut_ptr(), s.sel_in_off.as_mut_ptr(), s.sel_in_len.as_mut_ptr(), s.sel_out_off.as_mut_ptr(),
                                    s.sel_out_cap.as_mut_ptr(), s.src_off.as_mut_ptr(), s.dst_off.as_mut_ptr(), s.range_status.as_mut_ptr(), &mut s.summary)
    };
    if rc == sys::CHIP_OK { Ok(s) } else { Err(rc) }
}

///The device arrays of a plan: `n` units, `in_off` / `out_off` u64 and `in_len` / `out_cap` u32 entries.
pub struct PlanArrays<'a> {
    pub n: usize,
    pub in_off: &'a crate::buffer::DeviceBuffer,
    pub in_len: &'a crate::buffer::DeviceBuffer,
    pub out_off: &'a crate::buffer::DeviceBuffer,
    pub out_cap: &'a crate::buffer::DeviceBuffer,
}

impl PlanArrays<'_> {
    fn fits(&self) -> bool {
        self.in_off.capacity() >= 8 * self.n && self.out_off.capacity() >= 8 * self.n && self.in_len.capacity() >= 4 * self.n
            && self.out_cap.capacity() >= 4 * self.n
    }
}

///`chip_select_units`: the index step alone, for a caller that decodes into a buffer of its own.  `sel` holds room for `max_sel`
///rows of the sub-batch (`sel_unit`, then the four arrays of `decode_batch_device`); `src_off`, `dst_off` and `range_status`, if
///given, get one entry per range.  `max_sel` 0 counts.  Synchronous on `stream`.
///
///# Safety
///
///As `decode_batch_device`.
#[allow(clippy::too_many_arguments)]
pub unsafe fn select_units_device(plan: &PlanArrays, n_ranges: usize, range_lo: &crate::buffer::DeviceBuffer, range_len: &crate::buffer::DeviceBuffer,
                                  max_sel: usize, sel_unit: &mut crate::buffer::DeviceBuffer, sel: &mut [&mut crate::buffer::DeviceBuffer; 4],
                                  src_off: Option<&mut crate::buffer::DeviceBuffer>, dst_off: Option<&mut crate::buffer::DeviceBuffer>,
                                  range_status: Option<&mut crate::buffer::DeviceBuffer>, stream: *mut core::ffi::c_void)
                                  -> Result<sys::chip_select_summary, i32> {
    let small = |b: &Option<&mut crate::buffer::DeviceBuffer>, each: usize| b.as_ref().map_or(false, |b| b.capacity() < each * n_ranges);
    if !plan.fits() || range_lo.capacity() < 8 * n_ranges || range_len.capacity() < 4 * n_ranges || sel_unit.capacity() < 4 * max_sel
        || sel[0].capacity() < 8 * max_sel || sel[1].capacity() < 4 * max_sel || sel[2].capacity() < 8 * max_sel || sel[3].capacity() < 4 * max_sel
        || small(&src_off, 8) || small(&dst_off, 8) || small(&range_status, 4)
    {
        return Err(-101);
    }
    let opt = |b: Option<&mut crate::buffer::DeviceBuffer>| b.map_or(ptr::null_mut(), |b| b.as_mut_ptr());
    let mut summary = sys::chip_select_summary::default();
    let rc = sys::chip_select_units(plan.n, plan.in_off.as_ptr() as *const u64, plan.in_len.as_ptr() as *const u32, plan.out_off.as_ptr() as *const u64,
                                    plan.out_cap.as_ptr() as *const u32, n_ranges, range_lo.as_ptr() as *const u64, range_len.as_ptr() as *const u32,
                                    max_sel as u64, sel_unit.as_mut_ptr() as *mut u32, sel[0].as_mut_ptr() as *mut u64, sel[1].as_mut_ptr() as *mut u32,
                                    sel[2].as_mut_ptr() as *mut u64, sel[3].as_mut_ptr() as *mut u32, opt(src_off) as *mut u64, opt(dst_off) as *mut u64,
                                    opt(range_status) as *mut i32, &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///`chip_read_ranges`: the bytes of `n_ranges` ranges of the plan's decoded content, end to end in `dst`; only the units the ranges
///touch are decoded, each once.  `format` is what `decode_batch_device` takes for the plan's units (`BatchFormat::Zlib(ZlibMode::Gzip)` for a
///BGZF plan).  On `CHIP_READ_NEED_OUTPUT` nothing is written and `summary.out_len` says how much room is needed.  Synchronous on
///`stream`.
///
///# Safety
///
///As `decode_batch_device`; `dst` must not overlap `input`.
#[allow(clippy::too_many_arguments)]
pub unsafe fn read_ranges_device(format: BatchFormat, input: &crate::buffer::DeviceBuffer, plan: &PlanArrays, n_ranges: usize,
                                 range_lo: &crate::buffer::DeviceBuffer, range_len: &crate::buffer::DeviceBuffer, dst: &mut crate::buffer::DeviceBuffer,
                                 dst_off: Option<&mut crate::buffer::DeviceBuffer>, range_status: Option<&mut crate::buffer::DeviceBuffer>,
                                 stream: *mut core::ffi::c_void) -> Result<sys::chip_read_summary, i32> {
    let small = |b: &Option<&mut crate::buffer::DeviceBuffer>, each: usize| b.as_ref().map_or(false, |b| b.capacity() < each * n_ranges);
    if !plan.fits() || range_lo.capacity() < 8 * n_ranges || range_len.capacity() < 4 * n_ranges || small(&dst_off, 8) || small(&range_status, 4) {
        return Err(-101);
    }
    let opt = |b: Option<&mut crate::buffer::DeviceBuffer>| b.map_or(ptr::null_mut(), |b| b.as_mut_ptr());
    let mut summary = sys::chip_read_summary::default();
    let rc = sys::chip_read_ranges(format.tag(), plan.n, input.as_ptr() as *const _, plan.in_off.as_ptr() as *const u64, plan.in_len.as_ptr() as *const u32,
                                   plan.out_off.as_ptr() as *const u64, plan.out_cap.as_ptr() as *const u32, n_ranges, range_lo.as_ptr() as *const u64,
                                   range_len.as_ptr() as *const u32, dst.as_mut_ptr() as *mut _, dst.capacity() as u64, opt(dst_off) as *mut u64,
                                   opt(range_status) as *mut i32, &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///The device arrays of a checkpoint index: `n` points, `pt_bit` / `pt_out` u64 and `pt_check` u32 entries, `windows` 32 768 bytes
///per point.
pub struct IndexArrays<'a> {
    pub n: usize,
    pub pt_bit: &'a crate::buffer::DeviceBuffer,
    pub pt_out: &'a crate::buffer::DeviceBuffer,
    pub pt_check: &'a crate::buffer::DeviceBuffer,
    pub windows: &'a crate::buffer::DeviceBuffer,
}

impl IndexArrays<'_> {
    fn fits(&self) -> bool {
        self.pt_bit.capacity() >= 8 * self.n && self.pt_out.capacity() >= 8 * self.n && self.pt_check.capacity() >= 4 * self.n
            && self.windows.capacity() >= sys::CHIP_INDEX_WINDOW * self.n
    }
}

///`chip_inflate_index_build`: decodes the ONE gzip / zlib / raw deflate stream in the first `len` bytes of `input` into `output` --
///the answers are `decode_batch_device`'s for that unit -- and records a point every `spacing` decoded bytes (0 = 1 MiB) into the
///first `max_points` entries of the four arrays (`max_points` 0 counts).  Synchronous on `stream`.  No counterpart in this crate.
///
///# Safety
///
///As `decode_batch_device`; `input` must be 4-byte aligned and padded to a multiple of 4 bytes.
#[allow(clippy::too_many_arguments)]
pub unsafe fn inflate_index_build_device(mode: ZlibMode, input: &crate::buffer::DeviceBuffer, len: usize,
                                         output: &mut crate::buffer::DeviceBuffer, spacing: u32, max_points: usize,
                                         pt_bit: &mut crate::buffer::DeviceBuffer, pt_out: &mut crate::buffer::DeviceBuffer,
                                         pt_check: &mut crate::buffer::DeviceBuffer, windows: &mut crate::buffer::DeviceBuffer,
                                         stream: *mut core::ffi::c_void) -> Result<sys::chip_inflate_index_summary, i32> {
    if len > input.capacity() || pt_bit.capacity() < 8 * max_points || pt_out.capacity() < 8 * max_points || pt_check.capacity() < 4 * max_points
        || windows.capacity() < sys::CHIP_INDEX_WINDOW * max_points
    {
        return Err(-101);
    }
    let mut summary = sys::chip_inflate_index_summary::default();
    let rc = sys::chip_inflate_index_build(BatchFormat::Zlib(mode).tag(), input.as_ptr() as *const _, len as u64, output.as_mut_ptr() as *mut _,
                                           output.capacity() as u64, spacing, max_points as u64, pt_bit.as_mut_ptr() as *mut u64,
                                           pt_out.as_mut_ptr() as *mut u64, pt_check.as_mut_ptr() as *mut u32, windows.as_mut_ptr() as *mut _,
                                           &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///`chip_inflate_index_read`: the bytes of `n_ranges` ranges of an indexed stream's content, end to end in `dst`; only the chunks
///the ranges touch are decoded, each once and on a wave of its own, and each is verified against the next point's check value.
///`mode` is the build's `wrap` (Deflate, Zlib or Gzip; not Auto), `total_out` its `out_len`.  Synchronous on `stream`.
///
///# Safety
///
///As `read_ranges_device`.
#[allow(clippy::too_many_arguments)]
pub unsafe fn inflate_index_read_device(mode: ZlibMode, input: &crate::buffer::DeviceBuffer, len: usize, index: &IndexArrays,
                                        total_out: u64, n_ranges: usize, range_lo: &crate::buffer::DeviceBuffer,
                                        range_len: &crate::buffer::DeviceBuffer, dst: &mut crate::buffer::DeviceBuffer,
                                        dst_off: Option<&mut crate::buffer::DeviceBuffer>, range_status: Option<&mut crate::buffer::DeviceBuffer>,
                                        stream: *mut core::ffi::c_void) -> Result<sys::chip_read_summary, i32> {
    let small = |b: &Option<&mut crate::buffer::DeviceBuffer>, each: usize| b.as_ref().map_or(false, |b| b.capacity() < each * n_ranges);
    if len > input.capacity() || !index.fits() || range_lo.capacity() < 8 * n_ranges || range_len.capacity() < 4 * n_ranges || small(&dst_off, 8)
        || small(&range_status, 4)
    {
        return Err(-101);
    }
    let opt = |b: Option<&mut crate::buffer::DeviceBuffer>| b.map_or(ptr::null_mut(), |b| b.as_mut_ptr());
    let mut summary = sys::chip_read_summary::default();
    let rc = sys::chip_inflate_index_read(BatchFormat::Zlib(mode).tag(), input.as_ptr() as *const _, len as u64, index.n as u64,
                                          index.pt_bit.as_ptr() as *const u64, index.pt_out.as_ptr() as *const u64, index.pt_check.as_ptr() as *const u32,
                                          index.windows.as_ptr() as *const _, total_out, n_ranges, range_lo.as_ptr() as *const u64,
                                          range_len.as_ptr() as *const u32, dst.as_mut_ptr() as *mut _, dst.capacity() as u64, opt(dst_off) as *mut u64,
                                          opt(range_status) as *mut i32, &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///`chip_inflate_find_starts_host`: the block starts of the deflate stream in `input` (host memory), whose first block header is at
///bit `first_bit`: per chunk of `chunk_bytes` behind the first, the least bit position at which a dynamic block header the decoder
///accepts begins.  Pure host arithmetic; a start is a candidate, not a confirmed boundary.  No counterpart in this crate.
pub fn inflate_find_starts_host(input: &[u8], first_bit: u64, chunk_bytes: u32) -> Result<Vec<u64>, i32> {
    let mut n = 0u64;
    let rc = unsafe { sys::chip_inflate_find_starts_host(input.as_ptr(), input.len() as u64, first_bit, chunk_bytes, 0, ptr::null_mut(), &mut n) };
    if rc != sys::CHIP_OK {
        return Err(rc);
    }
    let mut starts = vec![0u64; n as usize];
    let rc = unsafe { sys::chip_inflate_find_starts_host(input.as_ptr(), input.len() as u64, first_bit, chunk_bytes, n, starts.as_mut_ptr(), &mut n) };
    if rc == sys::CHIP_OK { Ok(starts) } else { Err(rc) }
}

///`chip_inflate_find_starts`: the same answer for the first `len` bytes of a device-resident buffer, one wave per chunk.  The first
///`max` starts go to `starts` (u64 entries, ascending; `max` 0 counts); returns the number of starts of the whole buffer.
///Synchronous on `stream`.
///
///# Safety
///
///As `decode_batch_device`.
pub unsafe fn inflate_find_starts_device(input: &crate::buffer::DeviceBuffer, len: usize, first_bit: u64, chunk_bytes: u32, max: usize,
                                         starts: &mut crate::buffer::DeviceBuffer, stream: *mut core::ffi::c_void) -> Result<u64, i32> {
    if len > input.capacity() || starts.capacity() < 8 * max {
        return Err(-101);
    }
    let mut n = 0u64;
    let rc = sys::chip_inflate_find_starts(input.as_ptr() as *const _, len as u64, first_bit, chunk_bytes, max as u64, starts.as_mut_ptr() as *mut u64,
                                           &mut n, stream);
    if rc == sys::CHIP_OK { Ok(n) } else { Err(rc) }
}

///`chip_inflate_parallel`: decodes the ONE gzip / zlib / raw deflate stream in the first `len` bytes of `input` into `output` with a
///wave per chunk of `chunk_bytes` (0 = the default) in which a block start is found, and leaves the checkpoint index of the chain's
///chunks in the first `max_points` entries of the four arrays (`max_points` 0 counts).  A clean stream's answers are
///`decode_batch_device`'s for the unit; with too little room the summary says `CHIP_NEED_OUTPUT`, `out_len` 0 and the `total_out`
///to come back with; whatever is not clean is decoded serially (`path` 0).  Synchronous on `stream`.  No counterpart in this crate.
///
///# Safety
///
///As `inflate_index_build_device`.
#[allow(clippy::too_many_arguments)]
pub unsafe fn inflate_parallel_device(mode: ZlibMode, input: &crate::buffer::DeviceBuffer, len: usize, output: &mut crate::buffer::DeviceBuffer,
                                      chunk_bytes: u32, max_points: usize, pt_bit: &mut crate::buffer::DeviceBuffer,
                                      pt_out: &mut crate::buffer::DeviceBuffer, pt_check: &mut crate::buffer::DeviceBuffer,
                                      windows: &mut crate::buffer::DeviceBuffer, stream: *mut core::ffi::c_void)
                                      -> Result<sys::chip_inflate_parallel_summary, i32> {
    if len > input.capacity() || pt_bit.capacity() < 8 * max_points || pt_out.capacity() < 8 * max_points || pt_check.capacity() < 4 * max_points
        || windows.capacity() < sys::CHIP_INDEX_WINDOW * max_points
    {
        return Err(-101);
    }
    let mut summary = sys::chip_inflate_parallel_summary::default();
    let rc = sys::chip_inflate_parallel(BatchFormat::Zlib(mode).tag(), input.as_ptr() as *const _, len as u64, output.as_mut_ptr() as *mut _,
                                        output.capacity() as u64, chunk_bytes, max_points as u64, pt_bit.as_mut_ptr() as *mut u64,
                                        pt_out.as_mut_ptr() as *mut u64, pt_check.as_mut_ptr() as *mut u32, windows.as_mut_ptr() as *mut _,
                                        &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}

///`chip_inflate_parallel_next`: decodes the next part of one gzip / zlib / raw deflate stream of any length.  `slab` holds `len`
///bytes of the stream from byte `cursor.in_total` on, `window` (at least 32 768 bytes) the last `cursor.hist` bytes of the content
///delivered so far; the call delivers whole chain chunks or blocks into `output` while they fit, moves the cursor to a later block
///boundary (or through the trailer) and says in the summary how many bytes of the slab lie in front of the new cursor, how many
///bytes it delivered and why it stopped.  Synchronous on `stream`.  No counterpart in this crate.
///
///# Safety
///
///As `inflate_parallel_device`; `window` must be the one the cursor was left with.
pub unsafe fn inflate_parallel_next_device(mode: ZlibMode, cursor: &mut sys::chip_inflate_cursor, window: &mut crate::buffer::DeviceBuffer,
                                           slab: &crate::buffer::DeviceBuffer, len: usize, output: &mut crate::buffer::DeviceBuffer,
                                           chunk_bytes: u32, stream: *mut core::ffi::c_void)
                                           -> Result<sys::chip_inflate_next_summary, i32> {
    if len > slab.capacity() || window.capacity() < sys::CHIP_INDEX_WINDOW {
        return Err(-101);
    }
    let mut summary = sys::chip_inflate_next_summary::default();
    let rc = sys::chip_inflate_parallel_next(BatchFormat::Zlib(mode).tag(), cursor, window.as_mut_ptr() as *mut _, slab.as_ptr() as *const _,
                                             len as u64, output.as_mut_ptr() as *mut _, output.capacity() as u64, chunk_bytes, &mut summary, stream);
    if rc == sys::CHIP_OK { Ok(summary) } else { Err(rc) }
}
