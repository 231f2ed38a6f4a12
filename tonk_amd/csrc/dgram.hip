// dgram.hip -- the kernels that lay messages and footers out as datagrams in a caller's device
// buffers and walk the message sections of received ones (tonk_datagram.h, dgram.cpp).  The byte
// logic is dgram.h's.
//
//   tamd_dgram_frames : the work item is a message (then a footer).  Messages run from 3-byte
//       AckAcks to 2047 bytes, so a wave each would idle most of its lanes: sixteen lanes share a
//       message and stride the aligned 16-byte granules under its header and body, 256 contiguous
//       bytes per step and two steps in flight; a 2047-byte body takes four such rounds and one
//       more for its last granule, an AckAck one.  A granule is stored whole only when every byte
//       of it is this message's, so the messages of a datagram, which abut inside granules, and
//       its footer need no order among them: a block of 256 threads takes any 16 items of the
//       call.  The footer (24 bytes at the most) is written with byte stores.  No LDS.
//
//   tamd_dgram_sections : one serial chain per section, parallel over sections; the shape of
//       tamd_seal_packets' tag phase.  A workgroup of 512 threads owns 64 consecutive sections
//       and stages a tile of 128 bytes of each into LDS, eight lanes per section with coalesced
//       16-byte loads; then lane p of the first wave chases section p's headers through its tile
//       in LDS, where a header costs an LDS read and not a trip to memory.  The loads of the next
//       tile are in flight under the walk.  Every tile is staged, also those a long body passes
//       over; the loop bound is the group's longest section.  Nothing on the device but the
//       results is written.
//
// LDS: a section's tile is 9 granules (144 bytes) apart from the next one's, as in seal.hip.  The
// walking lanes read single bytes, which the LDS serves 32 lanes at a time over 32 dword banks: at
// 36 dwords from lane to lane, lanes at the same depth of their tiles meet four to a bank, where
// a pitch of 128 bytes would put all 32 on one.  (An odd pitch in dwords would spread them over
// all banks but break the 16-byte alignment of the staging stores.)  9,992 bytes per workgroup.
#include "kernel_abi.h"
#include "dgram.h"

#define TAMD_DGRAM_BUILD_BLOCK 256u
#define TAMD_DGRAM_BUILD_SHARE 16u  // lanes that share a message
#define TAMD_DGRAM_GROUP 64u        // sections of a workgroup: one per lane of the wave that walks
#define TAMD_DGRAM_SHARE 8u         // lanes that stage a section's tile
#define TAMD_DGRAM_BLOCK (TAMD_DGRAM_GROUP * TAMD_DGRAM_SHARE)
#define TAMD_DGRAM_PITCH (TAMD_DGRAM_TILE_V16 + 1u)

static_assert(TAMD_DGRAM_SHARE == TAMD_DGRAM_TILE_V16, "one lane per granule of a tile");

extern "C" __global__ void __launch_bounds__(TAMD_DGRAM_BUILD_BLOCK)
tamd_dgram_frames(const DgramMsg* __restrict__ msg, uint32_t n_msg, const DgramFoot* __restrict__ foot, uint32_t n_foot) {
    const uint32_t item = blockIdx.x * (TAMD_DGRAM_BUILD_BLOCK / TAMD_DGRAM_BUILD_SHARE) + threadIdx.x / TAMD_DGRAM_BUILD_SHARE;
    const uint32_t lane = threadIdx.x % TAMD_DGRAM_BUILD_SHARE;
    if (item < n_msg) {
        const DgramMsg g = msg[item];
        tamd_dgram_put((uint8_t*)g.dst, (const uint8_t*)g.src, g.len, g.head >> 16, g.head & 0xffffu, lane, TAMD_DGRAM_BUILD_SHARE);
    } else if (item - n_msg < n_foot) {
        const DgramFoot* f = foot + (item - n_msg);
        tamd_dgram_put_footer((uint8_t*)f->dst, f->b, f->len, lane, TAMD_DGRAM_BUILD_SHARE);
    }
}

extern "C" __global__ void __launch_bounds__(TAMD_DGRAM_BLOCK)
tamd_dgram_sections(const DgramSect* __restrict__ d, uint32_t n, uint32_t mode, uint32_t cap, DgramOut* __restrict__ out,
                    uint32_t* __restrict__ table) {
    __shared__ tamd_v16 s_tile[TAMD_DGRAM_GROUP * TAMD_DGRAM_PITCH];
    __shared__ uint64_t s_data[TAMD_DGRAM_GROUP];
    __shared__ uint32_t s_bytes[TAMD_DGRAM_GROUP], s_longest;

    // (threads past the first wave own no section: they only help to stage)
    const uint32_t lane = threadIdx.x, first = blockIdx.x * TAMD_DGRAM_GROUP, i = first + lane;
    const bool owner = lane < TAMD_DGRAM_GROUP;
    DgramSect g = {0, 0, 1};
    if (owner && i < n) g = d[i];
    const bool live = !g.skip;
    const uint32_t bytes = live ? g.bytes : 0u;

    if (owner) {
        s_data[lane] = g.data;
        s_bytes[lane] = bytes;
        uint32_t longest = bytes;
        for (uint32_t o = 32; o; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)longest, (int)o);
            longest = other > longest ? other : longest;
        }
        if (lane == 0) s_longest = longest;
    }
    __syncthreads();

    tamd_dgram_walk w;
    tamd_dgram_walk_init(&w, bytes);
    uint32_t* row = table + (size_t)(owner && i < n ? i : 0u) * cap;
    const uint32_t tiles = (s_longest + TAMD_DGRAM_TILE - 1u) / TAMD_DGRAM_TILE;
    const uint32_t j = lane / TAMD_DGRAM_SHARE, gr = lane % TAMD_DGRAM_SHARE;
    const uint8_t* from = (const uint8_t*)s_data[j];
    const uint32_t from_len = s_bytes[j];
    tamd_v16 v;
    bool have = tamd_dgram_stage(from, from_len, 0, gr, &v);
    for (uint32_t t = 0; t < tiles; ++t) {
        if (have) s_tile[j * TAMD_DGRAM_PITCH + gr] = v;
        __syncthreads();
        have = tamd_dgram_stage(from, from_len, t + 1u, gr, &v);
        if (live) tamd_dgram_walk_tile(&w, (const uint8_t*)&s_tile[lane * TAMD_DGRAM_PITCH], t, mode, row, cap);
        __syncthreads();  // the tile is consumed
    }
    if (owner && i < n) {
        tamd_dgram_walk_end(&w);
        DgramOut o;
        o.status = w.status;
        o.count = w.count;
        o.rel_off = w.rel_lo;
        o.rel_bytes = w.rel_hi - w.rel_lo;
        out[i] = o;
    }
}
