// The size pass of the batched inflate (chip_decode_batch_sizes): inflate_sizes_kernel and its launch.
//
// The kernel is inflate.hip's unit loop instantiated without the LZ77 executor (inflate_unit<true>: wrapper, block headers, table
// builds, walk and path resolve as they are, count_tokens() in place of flush_tokens()), so the device code is that file's, compiled
// here a second time.  It has a translation unit of its own because a second kernel beside inflate_kernel changes the compiler's
// inlining of the functions both call and with it inflate_kernel's register allocation; the decoder must come out of the build as
// it was.  The host side (scratch slot, lock, launch order) stays in inflate.hip: launch_inflate_sizes() there calls
// enqueue_inflate_sizes() here.
#define CHIP_INFLATE_SIZES_TU 1
#include "inflate.hip"
