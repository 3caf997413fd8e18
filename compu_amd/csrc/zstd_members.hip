// CHIP_F_MEMBERS for zstd: zstd_members_kernel and its launch.
//
// The kernel is zstd.hip's kernel body compiled with the frame loop (CHIP_ZSTD_MEMBERS, see there): a unit is a series of zstd frames and
// skippable frames, decoded one behind the other by the wave that owns the unit.  It has a translation unit of its own for the reason
// zstd_sizes.hip has one: zstd_kernel must come out of the build as it was.
#define CHIP_ZSTD_MEMBERS 1
#include "zstd.hip"
