// lz_place.h -- moving a message from a caller's device address into its stream's history ring
// (tonk_compress_batch.h, cbatch.cpp): the byte logic of tamd_lz_place_ring (lz_place.hip), also
// run as a serial host walk by tests/native/cbatch_check.cpp.
//
// The ring is TAMD_LZ_RING bytes, 16-byte aligned, with its first TAMD_LZ_MIRROR bytes repeated
// after it (lz.h: the compression kernel's wide loads at the ring's end).  A message of `len`
// bytes lands at ring offsets slot, slot + 1, ... wrapping at the ring's end; whatever of it falls
// into the ring's first TAMD_LZ_MIRROR bytes is written to the mirror as well.  So a message is
// up to four pieces (before the wrap, after it, and each one's share of the mirror), each a
// contiguous run of source bytes to a contiguous destination.
//
// Written for `nl` cooperating lanes (lane = 0..nl-1) that call with the same arguments and
// share nothing; on the host nl = 1.  No libc.  The source is read through frame.h's granule
// funnel: only aligned 16-byte granules that hold at least one byte of the message, at any source
// alignment, so nothing has to be readable behind a message.  The ring is written with aligned
// 16-byte stores where a whole granule belongs to the piece and with single bytes at the piece's
// two ends.
#pragma once
#include "frame.h"
#include "lz.h"

// Byte k (0..15) of v, picked with selects (an indexed read would move v to scratch memory).
TAMD_FRAME_FN uint32_t tamd_lz_place_byte(const tamd_v16& v, uint32_t k) {
    const uint32_t q = k >> 2;
    const uint32_t w = q == 0 ? v.w[0] : q == 1 ? v.w[1] : q == 2 ? v.w[2] : v.w[3];
    return (w >> (8u * (k & 3u))) & 0xffu;
}

// Whether granule m under a piece of `len` bytes that starts `s` bytes into granule 0 holds bytes
// of this piece only.
TAMD_FRAME_FN bool tamd_lz_place_whole(uint32_t s, uint32_t len, uint32_t m) {
    const int32_t p0 = 16 * (int32_t)m - (int32_t)s;
    return p0 >= 0 && p0 + 16 <= (int32_t)len;
}

// Lane `lane` of `nl`: its part of dst[0, len) = the bytes at src, a piece of the message that
// occupies [lo, hi) (source reads stay inside the granules under [lo, hi)).  No byte outside
// dst[0, len) is written.  Whole granules are strided over the lanes, two loaded before the first
// is stored; the first and the last granule, where the piece does not fill them, go out as
// single bytes, byte k of the granule by lane k % nl.
TAMD_FRAME_FN void tamd_lz_place_piece(uint8_t* dst, uintptr_t src, uint32_t len, uintptr_t lo, uintptr_t hi, uint32_t lane,
                                       uint32_t nl) {
    if (!len) return;
    const uint32_t s = (uint32_t)((uintptr_t)dst & 15u);
    uint8_t* g0 = dst - s;
    const uint32_t ng = (s + len + 15u) / 16u;
    for (uint32_t m = lane; m < ng; m += 2u * nl) {
        tamd_v16 v[2];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t u = 0; u < 2u; ++u)
            if (m + u * nl < ng && tamd_lz_place_whole(s, len, m + u * nl))
                v[u] = tamd_load16((uintptr_t)((int64_t)src + 16 * (int64_t)(m + u * nl) - (int64_t)s), lo, hi);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t u = 0; u < 2u; ++u)
            if (m + u * nl < ng && tamd_lz_place_whole(s, len, m + u * nl)) tamd_st16(g0 + 16u * (uint64_t)(m + u * nl), v[u]);
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t e = 0; e < 2u; ++e) {  // the two ends
        const uint32_t m = e ? ng - 1u : 0u;
        if ((e && m == 0u) || tamd_lz_place_whole(s, len, m)) continue;
        const int32_t p0 = 16 * (int32_t)m - (int32_t)s;
        const tamd_v16 v = tamd_load16((uintptr_t)((int64_t)src + p0), lo, hi);
        for (uint32_t k = lane; k < 16u; k += nl) {
            const int32_t at = p0 + (int32_t)k;
            if (at >= 0 && at < (int32_t)len) g0[16u * (uint64_t)m + k] = (uint8_t)tamd_lz_place_byte(v, k);
        }
    }
}

// Lane `lane` of `nl`: its part of the message of `len` bytes (1 .. TAMD_LZ_RING) at `src` into
// `ring` (16-byte aligned, TAMD_LZ_RING + TAMD_LZ_MIRROR bytes) from offset `slot`.
TAMD_FRAME_FN void tamd_lz_place(uint8_t* ring, uint32_t slot, const uint8_t* src, uint32_t len, uint32_t lane, uint32_t nl) {
    if (len == 0 || len > TAMD_LZ_RING) return;
    slot &= TAMD_LZ_RING - 1u;
    const uintptr_t lo = (uintptr_t)src, hi = lo + len;
    const uint32_t first = TAMD_LZ_RING - slot < len ? TAMD_LZ_RING - slot : len;  // bytes before the wrap
    tamd_lz_place_piece(ring + slot, lo, first, lo, hi, lane, nl);
    if (slot < TAMD_LZ_MIRROR) {
        const uint32_t part = TAMD_LZ_MIRROR - slot < first ? TAMD_LZ_MIRROR - slot : first;
        tamd_lz_place_piece(ring + TAMD_LZ_RING + slot, lo, part, lo, hi, lane, nl);
    }
    if (first < len) {  // the rest from the ring's start, and its share of the mirror
        const uint32_t rest = len - first;
        tamd_lz_place_piece(ring, lo + first, rest, lo, hi, lane, nl);
        tamd_lz_place_piece(ring + TAMD_LZ_RING, lo + first, rest < TAMD_LZ_MIRROR ? rest : TAMD_LZ_MIRROR, lo, hi, lane, nl);
    }
}
