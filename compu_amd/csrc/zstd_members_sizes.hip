// CHIP_F_MEMBERS for zstd, the size pass: zstd_members_sizes_kernel and its launch.
//
// zstd.hip's kernel body compiled with SIZES and the frame loop (CHIP_ZSTD_MEMBERS, see there); a translation unit of its own as
// zstd_sizes.hip and zstd_members.hip are.
#define CHIP_ZSTD_SIZES_TU 1
#define CHIP_ZSTD_MEMBERS 1
#include "zstd.hip"
