// unlz.hip -- tonk::MessageDecompressor on gfx950: restores zstd compressed blocks (and takes
// uncompressed messages into the history) for many streams at once.
//
// One wave per job; a job is a run of consecutive messages of one stream, decoded strictly in
// order (each is history for the next).  The waves of a workgroup run unrelated jobs and
// synchronise only with themselves.  The block reader is unlz.h, run with 64 lanes: its serial
// parts (headers, the table descriptions' bit fields, the FSE state walk) on lane 0, the Huffman
// streams on one lane each (four for the 4-stream form); the sequence tables' build (a lane per
// symbol, then per state), the Huffman table fill and every copy (literals, matches -- an
// overlapping match of offset o reads src + (i mod o)) over all lanes.  Sequences
// are decoded TAMD_UNLZ_CHUNK at a time into LDS and executed chunk by chunk.
//
// A wave's LDS: the stream's state (repeat offsets, ring bookkeeping, the Huffman table and the
// three sequence tables -- loaded from and written back to the stream's device memory, so they
// persist across launches), the block's working memory, the literals of a message of up to
// TAMD_LZ_MAX_MESSAGE bytes and a copy of a block of up to that size (the serial lanes then read
// LDS, not global memory).  Larger literal sections go to the job's global scratch; larger
// blocks are read in place.  The ring itself stays in global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

// A wave's writes (LDS and global) are complete and visible to its own lanes.
#define TAMD_UNLZ_SYNC()                                         \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   \
    } while (0)
#include "unlz.h"

struct UnlzWave {
    tamd_unlz_state S;
    tamd_unlz_work W;
    __attribute__((aligned(16))) uint8_t lit[TAMD_LZ_MAX_MESSAGE];
    __attribute__((aligned(16))) uint8_t blk[TAMD_LZ_MAX_MESSAGE + 16];
};
// (the compressor's kernel uses 17.5 KB per wave, lz.hip)
static_assert(sizeof(UnlzWave) <= 17920, "LDS per wave");
static_assert(sizeof(tamd_unlz_state) % 4 == 0 && sizeof(tamd_unlz_job) == 32 && sizeof(tamd_unlz_msg) == 32, "layouts");

typedef uint32_t unlz_u32u __attribute__((aligned(1)));

extern "C" __global__ void __launch_bounds__(64 * TAMD_UNLZ_WAVES)
tamd_lz_decompress(const tamd_unlz_job* __restrict__ jobs, uint32_t n_jobs, const tamd_unlz_msg* __restrict__ msgs,
                   const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint8_t* __restrict__ scratch,
                   uint32_t* __restrict__ restored, int32_t* __restrict__ status) {
    __shared__ UnlzWave Wv[TAMD_UNLZ_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ji = blockIdx.x * TAMD_UNLZ_WAVES + wave;
    if (ji >= n_jobs) return;  // (no workgroup barrier anywhere: the waves are independent)
    UnlzWave& L = Wv[wave];
    const tamd_unlz_job job = jobs[ji];
    uint32_t* const gstate = (uint32_t*)job.stream;
    uint8_t* const ring = job.stream + TAMD_UNLZ_RING_AT;
    uint8_t* const big = job.scratch == TAMD_UNLZ_NO_SCRATCH ? nullptr : scratch + job.scratch;
    if (job.flags & TAMD_UNLZ_FRESH) {
        if (lane == 0) tamd_unlz_reset(&L.S);
    } else {
        for (uint32_t i = lane; i < sizeof(tamd_unlz_state) / 4u; i += 64u) ((uint32_t*)&L.S)[i] = gstate[i];
    }
    TAMD_UNLZ_SYNC();

    for (uint32_t mi = job.first; mi < job.first + job.count; ++mi) {
        const tamd_unlz_msg m = msgs[mi];
        const uint32_t n = m.bytes;
        int32_t rc = L.S.failed ? TAMD_UNLZ_E_FAILED : (n == 0 || n > job.cap) ? TAMD_UNLZ_E_SIZE : TAMD_UNLZ_OK;
        uint32_t r = 0;
        if (!rc) {
            uint8_t* const o = (m.flags & TAMD_UNLZ_MSG_QUIET) ? nullptr : out + m.out;
            const uint8_t* src = in + m.in;
            if (lane == 0) tamd_unlz_place(&L.S, job.cap);
            if (m.flags & TAMD_UNLZ_MSG_BLOCK) {
                if (n <= TAMD_LZ_MAX_MESSAGE) {
                    // (4 bytes per lane, unaligned; up to 3 bytes past the block are read: the
                    // input carries 32 readable bytes after its last slot)
                    for (uint32_t i = 4u * lane; i < n; i += 256u) *(uint32_t*)(L.blk + i) = *(const unlz_u32u*)(src + i);
                    src = L.blk;
                }
                TAMD_UNLZ_SYNC();
                // (a block always has an output slot: the reader writes ring and slot together)
                rc = o ? tamd_unlz_block(&L.S, &L.W, ring, src, n, job.cap, o, L.lit, TAMD_LZ_MAX_MESSAGE, big, job.cap,
                                         lane, 64u, &r)
                       : TAMD_UNLZ_E_SIZE;
            } else {
                TAMD_UNLZ_SYNC();
                tamd_unlz_insert(&L.S, ring, src, n, o, lane, 64u);
                r = n;
            }
        }
        if (lane == 0) {
            status[mi] = rc;
            restored[mi] = rc ? 0u : r;
            if (rc && !L.S.failed) L.S.failed = rc;
        }
        TAMD_UNLZ_SYNC();
    }
    if (job.flags & TAMD_UNLZ_KEEP)
        for (uint32_t i = lane; i < sizeof(tamd_unlz_state) / 4u; i += 64u) gstate[i] = ((const uint32_t*)&L.S)[i];
}
