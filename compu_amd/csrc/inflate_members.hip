// CHIP_F_MEMBERS for gzip: inflate_members_kernel and inflate_members_sizes_kernel and their launch.
//
// The kernels are inflate.hip's unit loop compiled with the member loop (CHIP_INFLATE_MEMBERS, see inflate_unit there): a unit is a
// series of gzip members, decoded one behind the other by the wave that owns the unit.  They have a translation unit of their own for
// the reason inflate_sizes.hip has one: inflate_kernel and inflate_sizes_kernel must come out of the build as they were.  The host
// side (scratch slot, lock, launch order) stays in inflate.hip, which calls enqueue_inflate_members() here.
#define CHIP_INFLATE_MEMBERS 1
#include "inflate.hip"
