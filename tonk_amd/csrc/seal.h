// seal.h -- Tonk's datagram cipher and tag (tonk_seal.h): the byte logic shared by the kernels
// (seal.hip), their host side (seal.cpp) and the serial host walk of the tests
// (tests/native/seal_check.cpp).  A restatement of security::SimpleCipher (SimpleCipher.cpp:208-364)
// and of the 64-bit little-endian t1ha it tags with (thirdparty/t1ha.c:292-424).
//
//   cipher : byte q of the data is XORed with byte q & 3 of W(q >> 2),
//            W(w) = K[w & 3] + ((w >> 2) + 1) * A[w & 3]  (32-bit wrapping) -- the closed form of
//            the reference's running k[i] += a[i], its 4-byte tail loop and partial last word
//            included.  K is the expanded key, A the adder of the datagram's sequence.  Skipped
//            when K0 == K1 == 0.
//   tag    : (u16)(t1ha(data, bytes, seq ^ key) >> 19), computed with any key.
//
// The cipher functions are written for `nl` cooperating lanes (lane = 0..nl-1), as frame.h's are:
// the aligned 16-byte granules of memory under the data are strided over the lanes.  A granule is
// read when at least one of its bytes is ciphered; it is written with one aligned 16-byte store
// when all of its bytes are, and with single byte stores otherwise, so no byte outside the
// ciphered range is ever written.  The hash is one serial chain per datagram: a lane walks it over
// tiles of TAMD_SEAL_TILE bytes that tamd_seal_stage has laid out from datagram byte 0 (LDS on
// the device, a local array on the host; on the host nl = 1).  No libc.
#pragma once
#include "frame.h"

#define TAMD_SEAL_FN TAMD_FRAME_FN
#if defined(__HIPCC__)
#define TAMD_SEAL_UNROLL _Pragma("unroll")
#else
#define TAMD_SEAL_UNROLL
#endif

#define TAMD_SEAL_UNTAGGED 6u  // timestamp (3), flags (1), tag (2): TonkineseProtocol.h:169-193
#define TAMD_SEAL_FOOTER 24u   // kMaxOverheadBytes
#define TAMD_SEAL_TILE 128u    // bytes of one datagram staged at a time: four hash blocks
#define TAMD_SEAL_TILE_V16 (TAMD_SEAL_TILE / 16u)

// result of a datagram
#define TAMD_SEAL_OK 0
#define TAMD_SEAL_INVALID 1  // bytes < 6, bytes > max_datagram_bytes or message_bytes > bytes - 6
#define TAMD_SEAL_BAD_TAG 2  // open: the tag does not match; nothing was written

// kernel modes (bit set)
#define TAMD_SEAL_M_CIPHER 1u    // cipher [0, msg)
#define TAMD_SEAL_M_TAG 2u       // hash [0, tagged)
#define TAMD_SEAL_M_DATAGRAM 4u  // the connected-datagram layout: tagged = bytes - 6, tag at bytes - 2
#define TAMD_SEAL_M_CHECK 8u     // with DATAGRAM: compare the stored tag, cipher only on a match (open)

typedef struct tamd_seal_key { uint32_t k[4]; } tamd_seal_key;

// (a * b) folded: the low word of the product xor the product shifted down by 19
// (SimpleCipher.cpp:208-212)
TAMD_SEAL_FN uint32_t tamd_seal_maf19(uint32_t a, uint32_t b) {
    const uint64_t p = (uint64_t)a * b;
    return (uint32_t)p ^ (uint32_t)(p >> 19);
}

// Initialize (SimpleCipher.cpp:214-225)
TAMD_SEAL_FN tamd_seal_key tamd_seal_expand(uint64_t key) {
    tamd_seal_key e;
    e.k[0] = (uint32_t)key;
    e.k[1] = (uint32_t)(key >> 32);
    e.k[2] = tamd_seal_maf19(0xe7988061u, e.k[0]);
    e.k[3] = tamd_seal_maf19(0xbd9fa5c7u, e.k[1]);
    return e;
}

TAMD_SEAL_FN uint32_t tamd_seal_key_is_zero(const tamd_seal_key& e) { return (e.k[0] | e.k[1]) == 0u; }
TAMD_SEAL_FN uint64_t tamd_seal_key64(const tamd_seal_key& e) { return (uint64_t)e.k[1] << 32 | e.k[0]; }

// The adder of sequence `seq` (SimpleCipher.cpp:252-269)
TAMD_SEAL_FN tamd_seal_key tamd_seal_adder(uint64_t seq) {
    const uint32_t n0 = (uint32_t)seq + 0x80771ab1u;
    const uint32_t n1 = tamd_seal_maf19((uint32_t)(seq >> 32) + 0x55f2cc88u, 0xf3f77d13u);
    tamd_seal_key a;
    a.k[0] = tamd_seal_maf19(0x905c4577u, n0) + n1;
    a.k[1] = tamd_seal_maf19(0xb84c88cbu, n0) + n1;
    a.k[2] = tamd_seal_maf19(0xde0efbf1u, n0) + n1;
    a.k[3] = tamd_seal_maf19(0x9f614c3du, n0) + n1;
    return a;
}

// Word i & 3 of a key, picked with masks: a select chain over the words would become an indexed
// load and move the key from registers to scratch memory.
TAMD_SEAL_FN uint32_t tamd_seal_pick(const tamd_seal_key& e, uint32_t i) {
    const uint32_t odd = 0u - (i & 1u), high = 0u - ((i >> 1) & 1u);
    const uint32_t even_w = e.k[0] ^ ((e.k[0] ^ e.k[2]) & high), odd_w = e.k[1] ^ ((e.k[1] ^ e.k[3]) & high);
    return even_w ^ ((even_w ^ odd_w) & odd);
}

// The key rotated by c words: word k of the result is word (c + k) & 3 of e.
TAMD_SEAL_FN tamd_seal_key tamd_seal_rotate(const tamd_seal_key& e, uint32_t c) {
    tamd_seal_key r;
    r.k[0] = tamd_seal_pick(e, c);
    r.k[1] = tamd_seal_pick(e, c + 1u);
    r.k[2] = tamd_seal_pick(e, c + 2u);
    r.k[3] = tamd_seal_pick(e, c + 3u);
    return r;
}

// Keystream word w of a datagram
TAMD_SEAL_FN uint32_t tamd_seal_word(const tamd_seal_key& K, const tamd_seal_key& A, uint32_t w) {
    return tamd_seal_pick(K, w) + ((w >> 2) + 1u) * tamd_seal_pick(A, w);
}

// The byte mask of the memory dword whose first byte is datagram byte q (q may be negative, or
// the dword may reach past the end): 0xff for every byte with 0 <= q + b < len.
TAMD_SEAL_FN uint32_t tamd_seal_mask(int64_t q, uint32_t len) {
    uint32_t m = 0;
    TAMD_SEAL_UNROLL
    for (uint32_t b = 0; b < 4u; ++b) {
        const int64_t at = q + (int64_t)b;
        if (at >= 0 && at < (int64_t)len) m |= 0xffu << (8u * b);
    }
    return m;
}

// The keystream of the memory dword whose first byte is datagram byte q: a byte funnel of the two
// keystream words under it, zero for the bytes outside [0, len).
TAMD_SEAL_FN uint32_t tamd_seal_keystream(const tamd_seal_key& K, const tamd_seal_key& A, int64_t q, uint32_t len) {
    const uint32_t m = tamd_seal_mask(q, len);
    if (!m) return 0u;
    const uint32_t w = (uint32_t)(q >> 2), r = ((uint32_t)q & 3u) * 8u;  // (q >> 2 rounds down)
    const uint32_t lo = q >= 0 ? tamd_seal_word(K, A, w) : 0u;
    const uint32_t hi = tamd_seal_word(K, A, w + 1u);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> r) & m;
}

// One aligned granule of the data: `v` holds the 16 bytes at g0 + 16 m, where g0 is the granule
// under data byte 0 and s the data's offset in it; Kr and Ar are K and A rotated for s (below).
// The ciphered bytes go back with one 16-byte store when the whole granule is data, else byte by byte.
TAMD_SEAL_FN void tamd_seal_cipher_granule(uint8_t* g0, uint32_t s, uint32_t len, const tamd_seal_key& K, const tamd_seal_key& A,
                                           const tamd_seal_key& Kr, const tamd_seal_key& Ar, uint32_t m, tamd_v16 v) {
    uint8_t* g = g0 + 16u * (uint64_t)m;
    const int64_t q0 = 16 * (int64_t)m - (int64_t)s;  // the datagram byte at the granule's first byte
    if (q0 >= 0 && q0 + 16 <= (int64_t)len) {
        // the five keystream words under the granule, funnelled by the datagram's misalignment
        const uint32_t w0 = (uint32_t)(q0 >> 2), r = ((uint32_t)q0 & 3u) * 8u;
        uint32_t ks[5];
        TAMD_SEAL_UNROLL
        for (uint32_t k = 0; k < 5u; ++k) ks[k] = Kr.k[k & 3u] + (((w0 + k) >> 2) + 1u) * Ar.k[k & 3u];
        TAMD_SEAL_UNROLL
        for (uint32_t k = 0; k < 4u; ++k) v.w[k] ^= (uint32_t)((((uint64_t)ks[k + 1] << 32) | ks[k]) >> r);
        tamd_st16(g, v);
    } else {  // an end of the data: single bytes
        TAMD_SEAL_UNROLL
        for (uint32_t k = 0; k < 4u; ++k) {
            const int64_t q = q0 + 4 * (int64_t)k;
            const uint32_t x = v.w[k] ^ tamd_seal_keystream(K, A, q, len);
            TAMD_SEAL_UNROLL
            for (uint32_t b = 0; b < 4u; ++b) {
                const int64_t at = q + (int64_t)b;
                if (at >= 0 && at < (int64_t)len) g[4u * k + b] = (uint8_t)(x >> (8u * b));
            }
        }
    }
}

// Lane `lane` of `nl`: its part of Cipher(data, len, seq) under the expanded key K.  No byte
// outside data[0, len) is written.  Four granules are loaded before the first is stored, so that
// a lane has four loads in flight: the loop is a chain of memory round trips otherwise.
TAMD_SEAL_FN void tamd_seal_cipher(uint8_t* data, uint32_t len, const tamd_seal_key& K, const tamd_seal_key& A,
                                   uint32_t lane, uint32_t nl) {
    if (len == 0 || tamd_seal_key_is_zero(K)) return;
    const uint32_t s = (uint32_t)((uintptr_t)data & 15u);
    uint8_t* g0 = data - s;
    const uint32_t ng = (uint32_t)(((uint64_t)s + len + 15u) / 16u);
    // The first keystream word under a granule is word (16 m - s) >> 2: its index & 3 is the same
    // for every granule, so the keys are rotated once and then indexed statically.
    const uint32_t c = ((0u - s) >> 2) & 3u;
    const tamd_seal_key Kr = tamd_seal_rotate(K, c), Ar = tamd_seal_rotate(A, c);
    for (uint32_t m = lane; m < ng; m += 4u * nl) {
        tamd_v16 v[4];
        TAMD_SEAL_UNROLL
        for (uint32_t u = 0; u < 4u; ++u)
            if (m + u * nl < ng) v[u] = tamd_ld16((uintptr_t)(g0 + 16u * (uint64_t)(m + u * nl)));
        TAMD_SEAL_UNROLL
        for (uint32_t u = 0; u < 4u; ++u)
            if (m + u * nl < ng) tamd_seal_cipher_granule(g0, s, len, K, A, Kr, Ar, m + u * nl, v[u]);
    }
}

// TagInt (SimpleCipher.cpp:353-364)
TAMD_SEAL_FN uint64_t tamd_seal_rot64(uint64_t v, uint32_t s) { return (v >> s) | (v << (64u - s)); }
TAMD_SEAL_FN uint16_t tamd_seal_tag_int(const tamd_seal_key& K, uint32_t data) {
    const uint64_t prod = (uint64_t)K.k[0] * (data ^ K.k[1]);
    return (uint16_t)((prod ^ tamd_seal_rot64(prod, 41)) >> 19);
}

// ---- t1ha (thirdparty/t1ha.c:292-424), 64-bit little-endian ----

#define TAMD_T1HA_P0 17048867929148541611ull
#define TAMD_T1HA_P1 9386433910765580089ull
#define TAMD_T1HA_P2 15343884574428479051ull
#define TAMD_T1HA_P3 13662985319504319857ull
#define TAMD_T1HA_P4 11242949449147999147ull
#define TAMD_T1HA_P5 13862205317416547141ull
#define TAMD_T1HA_P6 14653293970879851569ull

// High and low halves of the 128-bit product, xored (t1ha.c:319-350), from 32-bit pieces: only
// tamd_t1ha_finish needs it, at most five times per datagram.
TAMD_SEAL_FN uint64_t tamd_t1ha_mux64(uint64_t v, uint64_t p) {
    const uint64_t v0 = (uint32_t)v, v1 = v >> 32, q0 = (uint32_t)p, q1 = p >> 32;
    const uint64_t ll = v0 * q0, lh = v0 * q1, hl = v1 * q0, hh = v1 * q1;
    const uint64_t mid = (ll >> 32) + (uint32_t)lh + (uint32_t)hl;
    const uint64_t hi = hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
    return hi ^ (v * p);
}

// The hash state of one datagram.  `blocks` 32-byte blocks come first (none when len <= 32), then
// `rem` tail bytes (0..32) from byte 32 * blocks.
typedef struct tamd_t1ha {
    uint64_t a, b, c, d;
    uint32_t blocks, rem;
} tamd_t1ha;

TAMD_SEAL_FN void tamd_t1ha_init(tamd_t1ha* s, uint32_t len, uint64_t seed) {
    s->a = seed;
    s->b = len;
    s->c = tamd_seal_rot64(len, 17) + seed;
    s->d = len ^ tamd_seal_rot64(seed, 17);
    s->blocks = len > 32u ? len / 32u : 0u;
    s->rem = len > 32u ? len & 31u : len;
}

// One 32-byte block (t1ha.c:368-378): low 64 bits of every product.
TAMD_SEAL_FN void tamd_t1ha_block(tamd_t1ha* s, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    const uint64_t d02 = w0 ^ tamd_seal_rot64(w2 + s->d, 17);
    const uint64_t c13 = w1 ^ tamd_seal_rot64(w3 + s->c, 17);
    s->c += s->a ^ tamd_seal_rot64(w0, 41);
    s->d -= s->b ^ tamd_seal_rot64(w1, 31);
    s->a ^= TAMD_T1HA_P1 * (d02 + w3);
    s->b ^= TAMD_T1HA_P0 * (c13 + w2);
}

// The low `n` bytes (1..8) of w
TAMD_SEAL_FN uint64_t tamd_t1ha_low(uint64_t w, uint32_t n) { return n >= 8u ? w : w & ((1ull << (8u * n)) - 1ull); }

// The fold after the blocks and the tail (t1ha.c:382-422).  w[0..3] hold the tail bytes in
// order; bytes past `rem` may be anything.
TAMD_SEAL_FN uint64_t tamd_t1ha_finish(const tamd_t1ha* s, const uint64_t* w) {
    uint64_t a = s->a, b = s->b;
    if (s->blocks) {
        a ^= TAMD_T1HA_P6 * (tamd_seal_rot64(s->c, 17) + s->d);
        b ^= TAMD_T1HA_P5 * (s->c + tamd_seal_rot64(s->d, 17));
    }
    const uint32_t rem = s->rem;
    if (rem > 24u) {
        b += tamd_t1ha_mux64(w[0], TAMD_T1HA_P4);
        a += tamd_t1ha_mux64(w[1], TAMD_T1HA_P3);
        b += tamd_t1ha_mux64(w[2], TAMD_T1HA_P2);
        a += tamd_t1ha_mux64(tamd_t1ha_low(w[3], rem - 24u), TAMD_T1HA_P1);
    } else if (rem > 16u) {
        a += tamd_t1ha_mux64(w[0], TAMD_T1HA_P3);
        b += tamd_t1ha_mux64(w[1], TAMD_T1HA_P2);
        a += tamd_t1ha_mux64(tamd_t1ha_low(w[2], rem - 16u), TAMD_T1HA_P1);
    } else if (rem > 8u) {
        b += tamd_t1ha_mux64(w[0], TAMD_T1HA_P2);
        a += tamd_t1ha_mux64(tamd_t1ha_low(w[1], rem - 8u), TAMD_T1HA_P1);
    } else if (rem > 0u) {
        a += tamd_t1ha_mux64(tamd_t1ha_low(w[0], rem), TAMD_T1HA_P1);
    }
    const uint64_t x = (a ^ b) * TAMD_T1HA_P0;
    return tamd_t1ha_mux64(tamd_seal_rot64(a + b, 17), TAMD_T1HA_P4) + (x ^ tamd_seal_rot64(x, 41));
}

// Tag (SimpleCipher.cpp:337-347) from the finished hash
TAMD_SEAL_FN uint16_t tamd_seal_tag16(uint64_t hash) { return (uint16_t)(hash >> 19); }

// ---- the tiles the hash walks ----

// Granule g (0..7) of tile t of the `len` bytes at `data`: datagram bytes [128 t + 16 g, + 16),
// zero past `len`.  False when the granule holds no byte (nothing to store).
TAMD_SEAL_FN bool tamd_seal_stage(const uint8_t* data, uint32_t len, uint32_t t, uint32_t g, tamd_v16* out) {
    const uint32_t off = t * TAMD_SEAL_TILE + 16u * g;
    if (off >= len) return false;
    *out = tamd_load16((uintptr_t)data + off, (uintptr_t)data, (uintptr_t)data + len);
    return true;
}

TAMD_SEAL_FN uint64_t tamd_seal_u64(const tamd_v16& v, uint32_t half) {
    return (uint64_t)v.w[2u * half + 1u] << 32 | v.w[2u * half];
}

// Advance the state over tile t (`tile`: its eight granules as staged): the whole blocks that lie
// in it, and the fold when the tail starts in it.  Returns true with *hash once the datagram is
// done.  A datagram whose tail is empty is done after its last block; tamd_seal_hash_end
// finishes one that no tile reached (len 0, or the tile after the last block was never staged).
TAMD_SEAL_FN bool tamd_seal_hash_tile(tamd_t1ha* s, const tamd_v16* tile, uint32_t t, uint64_t* hash) {
    TAMD_SEAL_UNROLL
    for (uint32_t k = 0; k < TAMD_SEAL_TILE / 32u; ++k) {
        const uint32_t blk = t * (TAMD_SEAL_TILE / 32u) + k;
        if (blk > s->blocks) break;
        const tamd_v16 x = tile[2u * k], y = tile[2u * k + 1u];
        const uint64_t w[4] = {tamd_seal_u64(x, 0), tamd_seal_u64(x, 1), tamd_seal_u64(y, 0), tamd_seal_u64(y, 1)};
        if (blk < s->blocks) {
            tamd_t1ha_block(s, w[0], w[1], w[2], w[3]);
        } else if (s->rem) {
            *hash = tamd_t1ha_finish(s, w);
            return true;
        }
    }
    return false;
}
TAMD_SEAL_FN uint64_t tamd_seal_hash_end(const tamd_t1ha* s) {
    const uint64_t w[4] = {0, 0, 0, 0};
    return tamd_t1ha_finish(s, w);  // (rem is 0: no tail byte is read)
}

// Whether a connected datagram of `bytes` with `msg` ciphered bytes may be sealed or opened.
TAMD_SEAL_FN bool tamd_seal_valid(uint32_t bytes, uint32_t msg, uint32_t max_bytes) {
    return bytes >= TAMD_SEAL_UNTAGGED && bytes <= max_bytes && msg <= bytes - TAMD_SEAL_UNTAGGED;
}

// The tag a connected datagram carries: Tag over its first `tagged` = bytes - 6 bytes (whose hash
// is `hash`) xor TagInt(ts24 << 8 | flags), read from the datagram (TonkineseOutgoing.cpp:643-678).
TAMD_SEAL_FN uint16_t tamd_seal_datagram_tag(const tamd_seal_key& K, uint64_t hash, const uint8_t* data, uint32_t tagged) {
    const uint32_t ts24 = data[tagged] | (uint32_t)data[tagged + 1u] << 8 | (uint32_t)data[tagged + 2u] << 16;
    return (uint16_t)(tamd_seal_tag16(hash) ^ tamd_seal_tag_int(K, ts24 << 8 | data[tagged + 3u]));
}

// The last min(total, 24) bytes of a datagram, right-aligned in out[0, 24), zeros in front.
TAMD_SEAL_FN void tamd_seal_footer24(const uint8_t* src, uint32_t total, uint8_t* out) {
    const uint32_t tl = total < TAMD_SEAL_FOOTER ? total : TAMD_SEAL_FOOTER;
    for (uint32_t k = 0; k < TAMD_SEAL_FOOTER; ++k)
        out[k] = k + tl >= TAMD_SEAL_FOOTER ? src[total - TAMD_SEAL_FOOTER + k] : (uint8_t)0;
}
