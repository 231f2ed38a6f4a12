// seal.hip -- the kernels that cipher and tag datagrams in a caller's device buffers (tonk_seal.h,
// seal.cpp).  The byte logic is seal.h's.
//
// A workgroup of 512 threads owns 64 consecutive datagrams of a call.  The two halves of the work
// have opposite shapes and run as two phases of the same workgroup:
//
//   cipher : parallel per byte.  Eight lanes share a datagram and stride its aligned 16-byte
//            granules (128 contiguous bytes per step); the eight waves cover the 64 datagrams.
//   tag    : one serial chain per datagram.  The workgroup stages a tile of 128 bytes of each of
//            its datagrams into LDS, again eight lanes per datagram; then lane p of the first wave
//            advances datagram p's hash state, kept in registers, over its tile.  The loop bound is
//            the group's longest datagram; a lane past its datagram's end does nothing.
//
// Eight waves rather than one: every step of either phase is a memory round trip (load, then a
// dependent store to memory or LDS), and a call of a tick's 16,384 datagrams has only 256 groups,
// one per CU.  With one wave per group nothing hides that latency (92.8 us for that call against
// 30 us with eight waves).  What remains is mostly the hash chain itself:
// four blocks per tile on one wave, while the other seven wait at the barrier.
//
// seal ciphers, then tags the ciphertext it wrote (a workgroup barrier in between orders the
// stores before the loads; the second read comes from the cache).  open tags the bytes as
// received, compares, and deciphers only the datagrams whose tag matched: nothing is written
// before the tag is known.
//
// LDS: a datagram's tile is 9 granules (144 bytes) apart from the next one.  A lane reads its
// 32-byte block as two 16-byte reads; the 16 lanes served together start 36 dwords apart, which
// spreads them over all 64 banks (a pitch of 128 bytes would put every other lane on the same
// four).  10,248 bytes per workgroup.
#include "kernel_abi.h"
#include "seal.h"

#define TAMD_SEAL_GROUP 64u  // datagrams of a workgroup: one per lane of the wave that hashes
#define TAMD_SEAL_SHARE 8u   // lanes that share a datagram in the cooperative steps
#define TAMD_SEAL_BLOCK (TAMD_SEAL_GROUP * TAMD_SEAL_SHARE)
#define TAMD_SEAL_PITCH (TAMD_SEAL_TILE_V16 + 1u)

static_assert(TAMD_SEAL_SHARE == TAMD_SEAL_TILE_V16, "one lane per granule of a tile");

__device__ __forceinline__ tamd_seal_key seal_load_key(const uint32_t* __restrict__ keys, uint32_t stream) {
    const uint4 v = ((const uint4*)keys)[stream];
    tamd_seal_key k;
    k.k[0] = v.x; k.k[1] = v.y; k.k[2] = v.z; k.k[3] = v.w;
    return k;
}

// The cipher over the bytes s_cipher names: datagram j of the group by threads 8 j .. 8 j + 7.
__device__ __forceinline__ void seal_cipher_phase(const SealDesc* __restrict__ d, uint32_t first,
                                                  const uint32_t* __restrict__ keys, const uint32_t* s_cipher) {
    const uint32_t j = threadIdx.x / TAMD_SEAL_SHARE;
    const uint32_t len = s_cipher[j];
    if (!len) return;
    const SealDesc g = d[first + j];
    tamd_seal_cipher((uint8_t*)g.data, len, seal_load_key(keys, g.stream), tamd_seal_adder(g.nonce), threadIdx.x % TAMD_SEAL_SHARE,
                     TAMD_SEAL_SHARE);
}

extern "C" __global__ void __launch_bounds__(TAMD_SEAL_BLOCK)
tamd_seal_packets(const SealDesc* __restrict__ d, uint32_t n, const uint32_t* __restrict__ keys, uint32_t mode,
                  uint32_t* __restrict__ out) {
    __shared__ tamd_v16 s_tile[TAMD_SEAL_GROUP * TAMD_SEAL_PITCH];
    __shared__ uint64_t s_data[TAMD_SEAL_GROUP];
    __shared__ uint32_t s_tagged[TAMD_SEAL_GROUP], s_cipher[TAMD_SEAL_GROUP], s_longest;

    // (threads past the first wave own no datagram: they only help to move bytes)
    const uint32_t lane = threadIdx.x, first = blockIdx.x * TAMD_SEAL_GROUP, i = first + lane;
    const bool owner = lane < TAMD_SEAL_GROUP;
    const bool datagram = mode & TAMD_SEAL_M_DATAGRAM, check = mode & TAMD_SEAL_M_CHECK;
    SealDesc g = {0, 0, 0, 0, 0, 1};
    if (owner && i < n) g = d[i];
    const bool live = !g.skip;
    tamd_seal_key K = {{0, 0, 0, 0}};
    if (live) K = seal_load_key(keys, g.stream);
    uint8_t* data = (uint8_t*)g.data;
    const uint32_t tagged = !live || !(mode & TAMD_SEAL_M_TAG) ? 0u : datagram ? g.bytes - TAMD_SEAL_UNTAGGED : g.bytes;
    const uint32_t clen = !live || !(mode & TAMD_SEAL_M_CIPHER) || tamd_seal_key_is_zero(K) ? 0u : datagram ? g.msg : g.bytes;
    uint32_t result = live ? TAMD_SEAL_OK : TAMD_SEAL_INVALID;

    if (owner) {
        s_data[lane] = g.data;
        s_tagged[lane] = tagged;
        s_cipher[lane] = check ? 0u : clen;
        uint32_t longest = tagged;
        for (uint32_t o = 32; o; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)longest, (int)o);
            longest = other > longest ? other : longest;
        }
        if (lane == 0) s_longest = longest;
    }
    __syncthreads();

    if (!check && (mode & TAMD_SEAL_M_CIPHER)) seal_cipher_phase(d, first, keys, s_cipher);

    if (mode & TAMD_SEAL_M_TAG) {
        tamd_t1ha st;
        tamd_t1ha_init(&st, tagged, g.nonce ^ tamd_seal_key64(K));
        uint64_t hash = 0;
        bool done = false;
        const uint32_t tiles = (s_longest + TAMD_SEAL_TILE - 1u) / TAMD_SEAL_TILE;
        const uint32_t j = lane / TAMD_SEAL_SHARE, gr = lane % TAMD_SEAL_SHARE;
        const uint8_t* from = (const uint8_t*)s_data[j];
        const uint32_t from_len = s_tagged[j];
        __syncthreads();  // the cipher's stores are visible
        // (the loads of tile t + 1 are in flight while tile t is hashed)
        tamd_v16 v;
        bool have = tamd_seal_stage(from, from_len, 0, gr, &v);
        for (uint32_t t = 0; t < tiles; ++t) {
            if (have) s_tile[j * TAMD_SEAL_PITCH + gr] = v;
            __syncthreads();
            have = tamd_seal_stage(from, from_len, t + 1u, gr, &v);
            if (live && !done) done = tamd_seal_hash_tile(&st, &s_tile[lane * TAMD_SEAL_PITCH], t, &hash);
            __syncthreads();  // the tile is consumed
        }
        if (live && !done) hash = tamd_seal_hash_end(&st);
        if (live && datagram) {
            const uint16_t tag = tamd_seal_datagram_tag(K, hash, data, tagged);
            if (check) {
                const uint16_t stored = (uint16_t)(data[tagged + 4u] | data[tagged + 5u] << 8);
                if (stored != tag) result = TAMD_SEAL_BAD_TAG;
                s_cipher[lane] = stored == tag ? clen : 0u;
            } else {
                data[tagged + 4u] = (uint8_t)tag;
                data[tagged + 5u] = (uint8_t)(tag >> 8);
            }
        } else if (live) {
            result = tamd_seal_tag16(hash);
        }
    }

    if (check) {
        __syncthreads();
        seal_cipher_phase(d, first, keys, s_cipher);
    }
    if (owner && i < n) out[i] = result;
}

// The last min(total, 24) bytes of each datagram, right-aligned in 24 bytes, zeros in front.
extern "C" __global__ void __launch_bounds__(256)
tamd_gather_footers(const TailDesc* __restrict__ d, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const TailDesc g = d[i];
    uint8_t t[TAMD_SEAL_FOOTER];
    tamd_seal_footer24((const uint8_t*)g.src, g.total, t);
#pragma unroll
    for (uint32_t k = 0; k < TAMD_SEAL_FOOTER / 4u; ++k)
        ((uint32_t*)out)[i * (TAMD_SEAL_FOOTER / 4u) + k] =
            t[4 * k] | t[4 * k + 1] << 8 | t[4 * k + 2] << 16 | (uint32_t)t[4 * k + 3] << 24;
}
