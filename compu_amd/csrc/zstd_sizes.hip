// The size pass of the batched zstd decode (chip_decode_batch_sizes): zstd_sizes_kernel and its launch.
//
// The kernel is zstd.hip's kernel body compiled with SIZES set (see there): headers, table builds, the FSE state chain, offsets and
// placement checks are that file's source, not a copy.  It has a translation unit of its own because a second kernel beside
// zstd_kernel changes the compiler's inlining of the functions both call; the decoder must come out of the build as it was.
#define CHIP_ZSTD_SIZES_TU 1
#include "zstd.hip"
