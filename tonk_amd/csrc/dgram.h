// dgram.h -- Tonk's message frames and datagram footers (tonk_datagram.h): the byte logic shared by
// the kernels (dgram.hip), their host side (dgram.cpp) and the serial host walk of the tests
// (tests/native/dgram_check.cpp).  A restatement of
//
//   the frame header   : u16 little-endian, type << 11 | bytes (protocol::WriteMessageFrameHeader,
//                        TonkineseProtocol.h:494-505; kMessageLengthBits 11, kMessageTypeMask 31)
//   the footer         : sequence bytes, nonce bytes, 12 handshake bytes, 24-bit timestamp, the
//                        flags byte, two tag bytes (sendQueuedDatagram, TonkineseOutgoing.cpp:602-640;
//                        the masks of TonkineseProtocol.h:518-523)
//   the walk           : headers chased through a message section with the errors "Truncated
//                        message", "Invalid frame" and "Invalid ackack", and the span of the reliable
//                        frames (ProcessDatagram, TonkineseIncoming.cpp:269-411 and :347-353;
//                        resumeProcessing :634-682 and onCompressed :488-515 without the AckAck rule)
//
// The copy of a message into its datagram is written for `nl` cooperating lanes (lane = 0..nl-1),
// as frame.h's and seal.h's functions are: the aligned 16-byte granules of memory under the
// message's header and body are strided over the lanes.  A granule is written with one aligned
// 16-byte store when all of its bytes belong to this message and with single byte stores
// otherwise (only the first and the last granule can be shared), so messages that abut inside a
// granule, and the footer behind them, never write each other's bytes and need no order among
// them.  A source granule is read only when one of its bytes belongs to the message.  The walk is
// one serial chain per section: a lane walks tiles of TAMD_DGRAM_TILE bytes that tamd_dgram_stage
// has laid out from section byte 0 (LDS on the device, a local array on the host).  No libc.
#pragma once
#include "frame.h"

#define TAMD_DGRAM_FN TAMD_FRAME_FN
#if defined(__HIPCC__)
#define TAMD_DGRAM_UNROLL _Pragma("unroll")
#else
#define TAMD_DGRAM_UNROLL
#endif

#define TAMD_DGRAM_FRAME 2u          // kMessageFrameBytes
#define TAMD_DGRAM_LEN_BITS 11u      // kMessageLengthBits
#define TAMD_DGRAM_LEN_MASK 2047u    // kMessageLengthMask
#define TAMD_DGRAM_TYPE_MASK 31u     // kMessageTypeMask
#define TAMD_DGRAM_T_ACKACK 2u       // MessageType_AckAck
#define TAMD_DGRAM_T_PADDING 4u      // MessageType_Padding
#define TAMD_DGRAM_T_RELIABLE 5u     // MessageType_StartOfReliables
#define TAMD_DGRAM_T_RAW 255u        // build only: no frame header (the body of an OnlyFEC datagram)
#define TAMD_DGRAM_ACKACK_BYTES 3u   // kAckAckBytes
#define TAMD_DGRAM_HANDSHAKE 12u     // kHandshakeBytes
#define TAMD_DGRAM_FOOTER 24u        // the longest footer: 3 + 3 + 12 + 3 + 1 + 2 (kMaxOverheadBytes)
#define TAMD_DGRAM_F_CONNECTION 0x80u
#define TAMD_DGRAM_F_HANDSHAKE 0x40u
#define TAMD_DGRAM_F_SEQCOMP 0x20u
#define TAMD_DGRAM_F_ONLYFEC 0x10u
#define TAMD_DGRAM_TILE 128u         // bytes of one section staged at a time
#define TAMD_DGRAM_TILE_V16 (TAMD_DGRAM_TILE / 16u)

// status of a parsed section
#define TAMD_DGRAM_OK 0u
#define TAMD_DGRAM_E_TRUNCATED 2u  // "Truncated message": a header announces more than remains
#define TAMD_DGRAM_E_FRAME 3u      // "Invalid frame": one byte is left over
#define TAMD_DGRAM_E_ACKACK 4u     // "Invalid ackack": ProcessDatagram's rules only

// ---- headers, flags, footer ----

TAMD_DGRAM_FN uint32_t tamd_dgram_header(uint32_t type, uint32_t bytes) { return (type << TAMD_DGRAM_LEN_BITS | bytes) & 0xffffu; }
TAMD_DGRAM_FN uint32_t tamd_dgram_header_type(uint32_t h) { return (h >> TAMD_DGRAM_LEN_BITS) & TAMD_DGRAM_TYPE_MASK; }
TAMD_DGRAM_FN uint32_t tamd_dgram_header_bytes(uint32_t h) { return h & TAMD_DGRAM_LEN_MASK; }
// A table entry of the parse: type (5 bits), bytes (11), the payload's offset in the section (16).
TAMD_DGRAM_FN uint32_t tamd_dgram_entry(uint32_t type, uint32_t bytes, uint32_t payload_offset) {
    return type << 27 | bytes << 16 | payload_offset;
}

// Of the caller's flag bits only SeqComp and OnlyFEC are taken.
TAMD_DGRAM_FN uint32_t tamd_dgram_flags(uint32_t seq_bytes, uint32_t nonce_bytes, uint32_t handshake, uint32_t flag_bits) {
    return TAMD_DGRAM_F_CONNECTION | (handshake ? TAMD_DGRAM_F_HANDSHAKE : 0u) |
           (flag_bits & (TAMD_DGRAM_F_SEQCOMP | TAMD_DGRAM_F_ONLYFEC)) | nonce_bytes << 2 | seq_bytes;
}

TAMD_DGRAM_FN uint32_t tamd_dgram_footer_bytes(uint32_t seq_bytes, uint32_t nonce_bytes, uint32_t handshake) {
    return seq_bytes + nonce_bytes + (handshake ? TAMD_DGRAM_HANDSHAKE : 0u) + 3u + 1u + 2u;
}

// The footer into out[0, 24): the low seq_bytes bytes of seq, the low nonce_bytes bytes of nonce,
// the handshake, the timestamp, the flags, two zero bytes where the tag will go.  Returns its length.
TAMD_DGRAM_FN uint32_t tamd_dgram_footer(uint8_t* out, uint32_t seq, uint32_t seq_bytes, uint32_t nonce, uint32_t nonce_bytes,
                                         const uint8_t* handshake, uint32_t ts24, uint32_t flag_bits) {
    uint32_t at = 0;
    for (uint32_t k = 0; k < seq_bytes; ++k) out[at++] = (uint8_t)(seq >> (8u * k));
    for (uint32_t k = 0; k < nonce_bytes; ++k) out[at++] = (uint8_t)(nonce >> (8u * k));
    for (uint32_t k = 0; handshake && k < TAMD_DGRAM_HANDSHAKE; ++k) out[at++] = handshake[k];
    for (uint32_t k = 0; k < 3u; ++k) out[at++] = (uint8_t)(ts24 >> (8u * k));
    out[at++] = (uint8_t)tamd_dgram_flags(seq_bytes, nonce_bytes, handshake != nullptr, flag_bits);
    out[at++] = 0;
    out[at++] = 0;
    return at;
}

// ---- the layout of one datagram (build) ----

typedef struct tamd_dgram_plan {
    uint32_t message_bytes, out_bytes, reliable_offset, reliable_bytes, rc;
} tamd_dgram_plan;

// The layout of a datagram of `count` messages (type[k], bytes[k]); offset[k] gets where message
// k's header (its body, for a raw one) starts.  rc 1 and nothing else meaningful when the input
// is invalid: a type above 31 or a body above 2047 bytes; a footer field wider than 3 bytes; an
// OnlyFEC datagram that is not exactly one raw message without a sequence number, or a raw message
// anywhere else; reliable messages without sequence bytes; a message other than Padding behind a
// reliable one that is not reliable itself (only Padding follows reliable data,
// TonkineseIncoming.cpp:398-400), or anything but Padding behind that Padding; a total above
// max_bytes or pitch.  The reliable span runs from the first reliable header to the end of the
// last reliable body, what the receiver's walk finds (below).
TAMD_DGRAM_FN tamd_dgram_plan tamd_dgram_layout(const uint32_t* type, const uint32_t* bytes, uint32_t count, uint32_t* offset,
                                                uint32_t seq_bytes, uint32_t nonce_bytes, uint32_t handshake, uint32_t flag_bits,
                                                uint32_t max_bytes, uint64_t pitch) {
    tamd_dgram_plan p = {0, 0, 0, 0, 1};
    if (seq_bytes > 3u || nonce_bytes > 3u) return p;
    const bool only_fec = (flag_bits & TAMD_DGRAM_F_ONLYFEC) != 0;
    if (only_fec && (count != 1u || type[0] != TAMD_DGRAM_T_RAW || seq_bytes != 0u)) return p;
    uint64_t at = 0;
    uint32_t lo = 0, hi = 0;
    bool padded = false;
    for (uint32_t k = 0; k < count; ++k) {
        offset[k] = (uint32_t)at;
        if (only_fec) { at += bytes[k]; break; }
        if (type[k] > TAMD_DGRAM_TYPE_MASK || bytes[k] > TAMD_DGRAM_LEN_MASK) return p;
        const uint64_t end = at + TAMD_DGRAM_FRAME + bytes[k];
        if (type[k] >= TAMD_DGRAM_T_RELIABLE) {
            if (padded) return p;
            if (hi == 0) lo = (uint32_t)at;
            hi = (uint32_t)end;
        } else if (hi != 0) {
            if (type[k] != TAMD_DGRAM_T_PADDING) return p;
            padded = true;
        }
        at = end;
        if (at > 65535u) return p;
    }
    if (hi != 0 && seq_bytes == 0u) return p;
    const uint64_t total = at + tamd_dgram_footer_bytes(seq_bytes, nonce_bytes, handshake);
    if (total > max_bytes || total > pitch) return p;
    p.message_bytes = (uint32_t)at;
    p.out_bytes = (uint32_t)total;
    p.reliable_offset = lo;
    p.reliable_bytes = hi - lo;
    p.rc = 0;
    return p;
}

// ---- a message into its datagram ----

// The 16 bytes that lie at message bytes [p0, p0 + 16) (p0 may be negative; byte 0 is the first
// header byte, byte hb the first of the `len` body bytes at `src`; src 0: a body of zeros).  Only
// the bytes inside [0, hb + len) mean anything.
TAMD_DGRAM_FN tamd_v16 tamd_dgram_chunk(uintptr_t src, uint32_t len, uint32_t hb, uint32_t hword, int32_t p0) {
    tamd_v16 v = {{0, 0, 0, 0}};
    if (src && len) v = tamd_load16((uintptr_t)((int64_t)src + p0 - (int32_t)hb), src, src + len);
    if (p0 < (int32_t)hb) {  // header bytes lie in this chunk
        TAMD_DGRAM_UNROLL
        for (uint32_t k = 0; k < TAMD_DGRAM_FRAME; ++k) {
            const int32_t b = (int32_t)k - p0;
            if (k >= hb || b < 0 || b >= 16) continue;
            const uint32_t sh = ((uint32_t)b & 3u) * 8u, val = ((hword >> (8u * k)) & 0xffu) << sh;
            TAMD_DGRAM_UNROLL
            for (uint32_t w = 0; w < 4u; ++w)
                if (((uint32_t)b >> 2) == w) v.w[w] = (v.w[w] & ~(0xffu << sh)) | val;
        }
    }
    return v;
}

// Byte k (0..15) of v, picked with selects (an indexed read would move v to scratch memory).
TAMD_DGRAM_FN uint32_t tamd_dgram_byte(const tamd_v16& v, uint32_t k) {
    const uint32_t q = k >> 2;
    const uint32_t w = q == 0 ? v.w[0] : q == 1 ? v.w[1] : q == 2 ? v.w[2] : v.w[3];
    return (w >> (8u * (k & 3u))) & 0xffu;
}

// Whether granule m of the message's destination (s: the offset of the message's first byte in
// granule 0) holds bytes of this message only.
TAMD_DGRAM_FN bool tamd_dgram_whole(uint32_t s, uint32_t total, uint32_t m) {
    const int32_t p0 = 16 * (int32_t)m - (int32_t)s;
    return p0 >= 0 && p0 + 16 <= (int32_t)total;
}

// Lane `lane` of `nl`: its part of dst[0, hb + len) = header || body, where the header is the low
// hb (0 or 2) bytes of hword.  No byte outside is written.  The granules that are wholly this
// message's are strided over the lanes, one aligned 16-byte store each, two loaded before the
// first is stored so that a lane has up to four loads in flight.  The first and the last granule,
// where they are shared, go out as single bytes, byte k of the granule by lane k % nl: the lanes
// of a group each write one byte at the most.
TAMD_DGRAM_FN void tamd_dgram_put(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t hb, uint32_t hword, uint32_t lane,
                                  uint32_t nl) {
    const uint32_t total = hb + len;
    if (!total) return;
    const uint32_t s = (uint32_t)((uintptr_t)dst & 15u);
    uint8_t* g0 = dst - s;
    const uint32_t ng = (s + total + 15u) / 16u;
    for (uint32_t m = lane; m < ng; m += 2u * nl) {
        tamd_v16 v[2];
        TAMD_DGRAM_UNROLL
        for (uint32_t u = 0; u < 2u; ++u)
            if (m + u * nl < ng && tamd_dgram_whole(s, total, m + u * nl))
                v[u] = tamd_dgram_chunk((uintptr_t)src, len, hb, hword, 16 * (int32_t)(m + u * nl) - (int32_t)s);
        TAMD_DGRAM_UNROLL
        for (uint32_t u = 0; u < 2u; ++u)
            if (m + u * nl < ng && tamd_dgram_whole(s, total, m + u * nl)) tamd_st16(g0 + 16u * (uint64_t)(m + u * nl), v[u]);
    }
    TAMD_DGRAM_UNROLL
    for (uint32_t e = 0; e < 2u; ++e) {  // the two ends
        const uint32_t m = e ? ng - 1u : 0u;
        if ((e && m == 0u) || tamd_dgram_whole(s, total, m)) continue;
        const int32_t p0 = 16 * (int32_t)m - (int32_t)s;
        const tamd_v16 v = tamd_dgram_chunk((uintptr_t)src, len, hb, hword, p0);
        for (uint32_t k = lane; k < 16u; k += nl) {
            const int32_t at = p0 + (int32_t)k;
            if (at >= 0 && at < (int32_t)total) g0[16u * (uint64_t)m + k] = (uint8_t)tamd_dgram_byte(v, k);
        }
    }
}

// Lane `lane` of `nl`: its bytes of the footer, byte stores only.
TAMD_DGRAM_FN void tamd_dgram_put_footer(uint8_t* dst, const uint8_t* footer, uint32_t len, uint32_t lane, uint32_t nl) {
    for (uint32_t k = lane; k < len && k < TAMD_DGRAM_FOOTER; k += nl) dst[k] = footer[k];
}

// ---- the walk of a message section ----

// Granule g (0..7) of tile t of the `len` bytes at `data`: section bytes [128 t + 16 g, + 16).
// False when the granule holds no byte of the section (nothing to store).
TAMD_DGRAM_FN bool tamd_dgram_stage(const uint8_t* data, uint32_t len, uint32_t t, uint32_t g, tamd_v16* out) {
    const uint32_t off = t * TAMD_DGRAM_TILE + 16u * g;
    if (off >= len) return false;
    *out = tamd_load16((uintptr_t)data + off, (uintptr_t)data, (uintptr_t)data + len);
    return true;
}

// The state of one section's walk.  `pos` is where the next header starts; `half` is set when its
// first byte (`low`) was the last byte of the tile before.
typedef struct tamd_dgram_walk {
    uint32_t bytes, pos, count, rel_lo, rel_hi, status, low;
    bool half, done;
} tamd_dgram_walk;

TAMD_DGRAM_FN void tamd_dgram_walk_init(tamd_dgram_walk* w, uint32_t bytes) {
    w->bytes = bytes;
    w->pos = w->count = w->rel_lo = w->rel_hi = w->low = 0;
    w->status = TAMD_DGRAM_OK;
    w->half = false;
    w->done = false;
}

// The end of a walk that ran out of headers: one byte left over is "Invalid frame"
// (TonkineseIncoming.cpp:407-411); true when the walk is over.
TAMD_DGRAM_FN bool tamd_dgram_walk_end(tamd_dgram_walk* w) {
    if (w->done) return true;
    const uint32_t left = w->bytes - w->pos;
    if (left >= TAMD_DGRAM_FRAME) return false;
    if (left) w->status = TAMD_DGRAM_E_FRAME;
    w->done = true;
    return true;
}

// Advance the walk over tile t (`tile`: its 128 bytes as staged; tiles come in order, none left
// out): every header that starts in it.  A header whose second byte lies in the next tile is
// finished there; a body may pass over whole tiles.  Entries go to table[0, cap), the frames
// beyond are counted only.  mode 0: ProcessDatagram's rules; 1: resumeProcessing's and
// onCompressed's, which have no AckAck rule.  The walk stops at the first error, whose frame is
// neither counted nor part of the reliable span.
TAMD_DGRAM_FN void tamd_dgram_walk_tile(tamd_dgram_walk* w, const uint8_t* tile, uint32_t t, uint32_t mode, uint32_t* table,
                                        uint32_t cap) {
    const uint32_t base = t * TAMD_DGRAM_TILE, end = base + TAMD_DGRAM_TILE;
    while (!tamd_dgram_walk_end(w)) {
        uint32_t b0, b1;
        if (w->half) {  // (pos + 1 == base)
            b0 = w->low;
            b1 = tile[0];
            w->half = false;
        } else {
            if (w->pos >= end) return;
            b0 = tile[w->pos - base];
            if (w->pos + 1u >= end) {
                w->low = b0;
                w->half = true;
                return;
            }
            b1 = tile[w->pos + 1u - base];
        }
        const uint32_t h = b0 | b1 << 8, len = tamd_dgram_header_bytes(h), type = tamd_dgram_header_type(h);
        const uint32_t body = w->pos + TAMD_DGRAM_FRAME;
        if (w->bytes - body < len) {
            w->status = TAMD_DGRAM_E_TRUNCATED;
            w->done = true;
            return;
        }
        if (mode == 0u && type == TAMD_DGRAM_T_ACKACK && len != TAMD_DGRAM_ACKACK_BYTES) {
            w->status = TAMD_DGRAM_E_ACKACK;
            w->done = true;
            return;
        }
        if (w->count < cap) table[w->count] = tamd_dgram_entry(type, len, body);
        ++w->count;
        if (type >= TAMD_DGRAM_T_RELIABLE) {
            if (w->rel_hi == 0u) w->rel_lo = w->pos;
            w->rel_hi = body + len;
        }
        w->pos = body + len;
    }
}
