// lz_place.hip -- the kernel that moves a call's messages from the caller's device addresses into
// their streams' history rings (tonk_compress_batch.h, cbatch.cpp).  The byte logic is lz_place.h's.
//
//   tamd_lz_place_ring : the work item is a message.  Messages run from 1 to 24,000 bytes and a
//       tick's are mostly a few hundred, so a workgroup each (the drop-in's tamd_lz_scatter_ring)
//       or a wave each would idle most of its lanes: sixteen lanes share a message, as in
//       tamd_dgram_frames, and stride the aligned 16-byte granules of the ring under it, 256
//       contiguous bytes per step and two steps in flight.  A 1300-byte message takes three such
//       rounds, a 64-byte one a single store per lane at the most; a 24,000-byte message takes 47,
//       which is rare and still coalesced.  A granule is stored whole only when every byte of it
//       is this message's, and the bytes at a message's two ends go out singly, so the messages
//       of one stream in a pass, which abut in the ring and share granules, need no order among
//       them: a block of 256 threads takes any 16 items of the call.  The host never puts two
//       messages of a pass on the same ring bytes (lz_pass.h).  No LDS.
#include "kernel_abi.h"
#include "lz_place.h"

#define TAMD_LZ_PLACE_BLOCK 256u
#define TAMD_LZ_PLACE_SHARE 16u  // lanes that share a message

extern "C" __global__ void __launch_bounds__(TAMD_LZ_PLACE_BLOCK)
tamd_lz_place_ring(const LzPlaceDesc* __restrict__ d, uint32_t n) {
    const uint32_t item = blockIdx.x * (TAMD_LZ_PLACE_BLOCK / TAMD_LZ_PLACE_SHARE) + threadIdx.x / TAMD_LZ_PLACE_SHARE;
    if (item >= n) return;
    const LzPlaceDesc g = d[item];
    tamd_lz_place((uint8_t*)g.ring, g.slot, (const uint8_t*)g.src, g.len, threadIdx.x % TAMD_LZ_PLACE_SHARE, TAMD_LZ_PLACE_SHARE);
}
