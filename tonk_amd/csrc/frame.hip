// frame.hip -- the kernels that move packets between a caller's device buffers and arena rows
// (tonk_batch.h, batch.cpp).  The byte logic is frame.h's; here it runs across the lanes of one
// wave per packet, or `wpp` (1, 2 or 4) waves of one workgroup for long packets.  No LDS, no
// scratch: a lane keeps two 16-byte granules and the shifted result in registers.
#include "kernel_abi.h"
#include "frame.h"

// (packet index, lane within the packet's lanes) of this thread: frame.h's arithmetic
__device__ __forceinline__ uint32_t frame_packet(uint32_t wpp, uint32_t* lane) {
    return tamd_frame_packet(blockIdx.x, threadIdx.x, wpp, lane);
}

// Packet -> arena row: varint(len) || payload || zeros to the row's capacity (raw: no header).
extern "C" __global__ void __launch_bounds__(TAMD_FRAME_BLOCK)
tamd_frame_rows(const FrameDesc* __restrict__ d, uint32_t n, uint8_t* __restrict__ arena, uint32_t wpp) {
    uint32_t lane;
    const uint32_t i = frame_packet(wpp, &lane);
    if (i >= n) return;
    const FrameDesc g = d[i];
    tamd_frame_row(arena + (size_t)g.row * TAMD_ROW_UNIT, g.cap, (const uint8_t*)g.src, g.len, g.raw, lane, 64u * wpp);
}

// Arena row -> the caller's slot.  The header is decoded and checked against the row's upper bound
// and the slot pitch before anything is written; out[i] gets the payload length and the status.
// Nothing is written past the payload, and no payload at all without `write`.
extern "C" __global__ void __launch_bounds__(TAMD_FRAME_BLOCK)
tamd_unframe_rows(const UnframeDesc* __restrict__ d, uint32_t n, const uint8_t* __restrict__ arena, uint64_t pitch,
                  UnframeOut* __restrict__ out, uint32_t write, uint32_t wpp) {
    uint32_t lane;
    const uint32_t i = frame_packet(wpp, &lane);
    if (i >= n) return;
    tamd_unframe_packet(d, i, arena, pitch, out, write, lane, 64u * wpp);
}

// The last min(total, 8) bytes of each packet (a recovery packet's footer), 8 bytes per packet.
extern "C" __global__ void __launch_bounds__(TAMD_FRAME_BLOCK)
tamd_gather_tails(const TailDesc* __restrict__ d, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * TAMD_FRAME_BLOCK + threadIdx.x;
    if (i >= n) return;
    const TailDesc g = d[i];
    uint8_t t[8];
    tamd_tail8((const uint8_t*)g.src, g.total, t);
    uint2 v;
    v.x = t[0] | t[1] << 8 | t[2] << 16 | (uint32_t)t[3] << 24;
    v.y = t[4] | t[5] << 8 | t[6] << 16 | (uint32_t)t[7] << 24;
    ((uint2*)out)[i] = v;
}
