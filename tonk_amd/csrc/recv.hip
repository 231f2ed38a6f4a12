// recv.hip -- the kernels that take a call's datagrams through the front of Tonk's receive path in
// the caller's device buffers (tonk_receive.h, recv.cpp).  The byte and state logic is recv.h's,
// the cipher and the hash seal.h's.
//
// A datagram's tag is a serial hash chain seeded with its nonce, and its nonce depends on which
// earlier datagrams of its connection passed their tag.  Five launches on the handle's stream, in
// this order, break that circle without hashing in a per-connection loop and without one launch
// per depth of the tick; order between workgroups comes from the launch order alone:
//
//   parse    : a thread per datagram reads its footer fields (RecvFields).
//   predict  : a thread per listed stream guesses its datagrams' nonces in list order, as if every
//              earlier one of the call were accepted (only a failed tag makes a guess wrong).  It
//              reads the state and writes guesses only.
//   tag      : tamd_seal_packets' tag phase over every datagram under its guessed nonce: 512
//              threads own 64 datagrams, stage 128-byte tiles in LDS (eight lanes per datagram, 144
//              bytes apart), and the first wave advances one hash chain per lane.  Verdicts only.
//   resolve  : a thread per listed stream walks its datagrams against the real state: expansion,
//              duplicate check, the verdict of `tag` where the real nonce is the guess (else the
//              lane hashes that one datagram again), accept, the re-ordered rule.
//   decipher : seal.h's cipher, eight lanes per accepted datagram; its first workgroup also
//              copies the handle's guard blocks behind the results.
//
// Nothing in the caller's memory is written before `decipher`, so `tag` and a repair in `resolve`
// hash every datagram as it was received, a datagram that lies twice in the call included.
#include "kernel_abi.h"
#include "recv.h"

#define TAMD_RECV_GROUP 64u  // datagrams of a workgroup of tag and decipher
#define TAMD_RECV_SHARE 8u   // lanes that share a datagram there
#define TAMD_RECV_BLOCK (TAMD_RECV_GROUP * TAMD_RECV_SHARE)
#define TAMD_RECV_PITCH (TAMD_SEAL_TILE_V16 + 1u)
#define TAMD_RECV_GUARD 64u  // bytes of a guard block (recv.cpp kGuard)

static_assert(TAMD_RECV_SHARE == TAMD_SEAL_TILE_V16, "one lane per granule of a tile");

__device__ __forceinline__ tamd_seal_key recv_load_key(const uint32_t* __restrict__ keys, uint32_t stream) {
    const uint4 v = ((const uint4*)keys)[stream];
    tamd_seal_key k;
    k.k[0] = v.x; k.k[1] = v.y; k.k[2] = v.z; k.k[3] = v.w;
    return k;
}

extern "C" __global__ void __launch_bounds__(256) tamd_rx_parse(const RecvCall c) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= c.n) return;
    const RecvDesc g = c.d[i];
    c.f[i] = tamd_recv_read_footer((const uint8_t*)g.data, g.bytes, c.max_bytes);
}

extern "C" __global__ void __launch_bounds__(64) tamd_rx_predict(const RecvCall c) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= c.n_listed) return;
    const uint32_t a = c.start[j];
    tamd_recv_predict_stream(c.state + (uint64_t)c.listed[j] * TAMD_RECV_STATE_WORDS, c.idx + a, c.start[j + 1u] - a, c.f, c.pred);
}

extern "C" __global__ void __launch_bounds__(TAMD_RECV_BLOCK) tamd_rx_tag(const RecvCall c) {
    __shared__ tamd_v16 s_tile[TAMD_RECV_GROUP * TAMD_RECV_PITCH];
    __shared__ uint64_t s_data[TAMD_RECV_GROUP];
    __shared__ uint32_t s_tagged[TAMD_RECV_GROUP], s_longest;

    // (threads past the first wave own no datagram: they only help to move bytes)
    const uint32_t lane = threadIdx.x, i = blockIdx.x * TAMD_RECV_GROUP + lane;
    const bool owner = lane < TAMD_RECV_GROUP;
    RecvDesc g = {0, 0, 0};
    RecvFields f = {0, 0, 0, 0, 0, 0, 0};
    if (owner && i < c.n) {
        g = c.d[i];
        f = c.f[i];
    }
    const bool live = f.flags != 0;
    tamd_seal_key K = {{0, 0, 0, 0}};
    uint64_t nonce = 0;
    if (live) {
        K = recv_load_key(c.keys, g.stream);
        nonce = c.pred[i];
    }
    const uint32_t tagged = live ? g.bytes - TAMD_SEAL_UNTAGGED : 0u;
    if (owner) {
        s_data[lane] = g.data;
        s_tagged[lane] = tagged;
        uint32_t longest = tagged;
        for (uint32_t o = 32; o; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)longest, (int)o);
            longest = other > longest ? other : longest;
        }
        if (lane == 0) s_longest = longest;
    }
    __syncthreads();

    tamd_t1ha st;
    tamd_t1ha_init(&st, tagged, nonce ^ tamd_seal_key64(K));
    uint64_t hash = 0;
    bool done = false;
    const uint32_t tiles = (s_longest + TAMD_SEAL_TILE - 1u) / TAMD_SEAL_TILE;
    const uint32_t j = lane / TAMD_RECV_SHARE, gr = lane % TAMD_RECV_SHARE;
    const uint8_t* from = (const uint8_t*)s_data[j];
    const uint32_t from_len = s_tagged[j];
    // (the loads of tile t + 1 are in flight while tile t is hashed)
    tamd_v16 v;
    bool have = tamd_seal_stage(from, from_len, 0, gr, &v);
    for (uint32_t t = 0; t < tiles; ++t) {
        if (have) s_tile[j * TAMD_RECV_PITCH + gr] = v;
        __syncthreads();
        have = tamd_seal_stage(from, from_len, t + 1u, gr, &v);
        if (live && !done) done = tamd_seal_hash_tile(&st, &s_tile[lane * TAMD_RECV_PITCH], t, &hash);
        __syncthreads();  // the tile is consumed
    }
    if (live && !done) hash = tamd_seal_hash_end(&st);
    if (owner && i < c.n) c.tag_ok[i] = live ? tamd_recv_tag_ok(K, hash, (const uint8_t*)g.data, g.bytes) : 0u;
}

extern "C" __global__ void __launch_bounds__(64) tamd_rx_resolve(const RecvCall c) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= c.n_listed) return;
    const uint32_t a = c.start[j], stream = c.listed[j];
    tamd_recv_resolve_stream(c.state + (uint64_t)stream * TAMD_RECV_STATE_WORDS, recv_load_key(c.keys, stream), c.idx + a,
                             c.start[j + 1u] - a, c.d, c.f, c.pred, c.tag_ok, c.rc, c.res, c.clen);
}

extern "C" __global__ void __launch_bounds__(TAMD_RECV_BLOCK) tamd_rx_decipher(const RecvCall c) {
    if (blockIdx.x == 0 && threadIdx.x < 3u * TAMD_RECV_GUARD / 4u) {  // the guard blocks, a dword per thread
        const uint32_t b = threadIdx.x / (TAMD_RECV_GUARD / 4u), w = threadIdx.x % (TAMD_RECV_GUARD / 4u);
        const uint8_t* from = b == 0 ? c.guard[0] : b == 1 ? c.guard[1] : c.guard[2];  // (selects: no indexed read of the arguments)
        ((uint32_t*)c.guards_out)[threadIdx.x] = ((const uint32_t*)from)[w];
    }
    const uint32_t i = blockIdx.x * TAMD_RECV_GROUP + threadIdx.x / TAMD_RECV_SHARE;
    if (i >= c.n) return;
    const uint32_t len = c.clen[i];
    if (!len) return;
    const RecvDesc g = c.d[i];
    tamd_seal_cipher((uint8_t*)g.data, len, recv_load_key(c.keys, g.stream), tamd_seal_adder(c.res[i].nonce),
                     threadIdx.x % TAMD_RECV_SHARE, TAMD_RECV_SHARE);
}
