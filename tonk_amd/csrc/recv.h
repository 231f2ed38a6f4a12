// recv.h -- the front of Tonk's receive path (tonk_receive.h): the byte and state logic shared by
// the kernels (recv.hip), their host side (recv.cpp) and the serial host walk of the tests
// (tests/native/recv_check.cpp).  A restatement of
//
//   the footer read   : flags, 24-bit timestamp, handshake, truncated nonce, truncated sequence
//                       number from the datagram's end (SessionIncoming::ProcessDatagram,
//                       TonkineseIncoming.cpp:110-140 and :203-207; FlagsReader,
//                       TonkineseProtocol.h:518-575)
//   the expansion     : CounterExpand (Counter.h:297-350 and :390-409) against LargestSequence;
//                       no nonce bytes: LargestSequence + 1
//   the register      : security::StrikeRegister's IsDuplicate and Accept (StrikeRegister.cpp:62-142)
//                       over 4096 bits that rotate in place, Counter64's wrapping comparisons
//   the verdict       : duplicate, then tag, then accept, then "Ignored re-ordered"
//                       (TonkineseIncoming.cpp:142-173 and :216)
//
// A stream's state is TAMD_RECV_STATE_WORDS 64-bit words: LargestSequence, WindowBase,
// WindowBitRotation and the 64 window words.
//
// The work of a call is split in steps (recv.hip).  The per-datagram steps take lane `lane` of
// `nl` as seal.h's functions do; the per-stream steps are one serial walk over a stream's
// datagrams in list order, one lane per stream (on the host nl = 1 and the lanes run one after
// the other).  tamd_recv_predict_stream guesses every nonce as if all earlier datagrams of the
// call were accepted; the tags are checked in parallel under the guesses; tamd_recv_resolve_stream
// then walks the real state and takes a guess's verdict only where the real nonce equals the
// guess -- otherwise it hashes that datagram again itself.  So no result depends on the guesses:
// with any array of guesses (and the verdicts under them) the results are the sequential model's.
// No libc.
#pragma once
#include "kernel_abi.h"
#include "seal.h"

#define TAMD_RECV_FN TAMD_FRAME_FN

#define TAMD_RECV_BITS 4096u         // kStrikeRegisterBits
#define TAMD_RECV_WORDS 64u          // kWordCount
#define TAMD_RECV_STATE_WORDS 67u    // largest, base, rotation, the window
#define TAMD_RECV_S_LARGEST 0u
#define TAMD_RECV_S_BASE 1u
#define TAMD_RECV_S_ROTATION 2u
#define TAMD_RECV_S_WINDOW 3u

// result of a datagram, in the reference's order of checks
#define TAMD_RECV_OK 0u
#define TAMD_RECV_INVALID 1u    // too short for its own flags, too long, or not a connection datagram
#define TAMD_RECV_BAD_TAG 2u    // "Bad checksum"
#define TAMD_RECV_DUPLICATE 3u  // "Ignored dupe"
#define TAMD_RECV_REORDERED 4u  // accepted and deciphered, but "Ignored re-ordered"
#define TAMD_RECV_REPAIRED 0x100u  // or-ed into the kernel's word: the tag was hashed again in the resolve step

// a < b as Counter64 compares (Counter.h:185-204): the wrapped difference has its top bit set
TAMD_RECV_FN bool tamd_recv_less(uint64_t a, uint64_t b) { return (int64_t)(a - b) < 0; }

// ---- the footer ----

TAMD_RECV_FN uint32_t tamd_recv_handshake_bytes(uint32_t flags) { return flags & 0x40u ? 12u : 0u; }
TAMD_RECV_FN uint32_t tamd_recv_nonce_bytes(uint32_t flags) { return (flags >> 2) & 3u; }
TAMD_RECV_FN uint32_t tamd_recv_seq_bytes(uint32_t flags) { return flags & 3u; }
// ConnectedFooterBytes
TAMD_RECV_FN uint32_t tamd_recv_footer_bytes(uint32_t flags) {
    return TAMD_SEAL_UNTAGGED + tamd_recv_handshake_bytes(flags) + tamd_recv_nonce_bytes(flags) + tamd_recv_seq_bytes(flags);
}

// The low `nb` (0..3) bytes that end in front of data[end], little-endian (ReadFooterField).
TAMD_RECV_FN uint32_t tamd_recv_field(const uint8_t* data, uint32_t end, uint32_t nb) {
    uint32_t v = 0;
    TAMD_SEAL_UNROLL
    for (uint32_t k = 0; k < 3u; ++k)
        if (k < nb) v |= (uint32_t)data[end - nb + k] << (8u * k);
    return v;
}

// The footer fields of the datagram of `bytes` at `data`.  flags 0 and nothing read further when it
// is invalid: shorter than six bytes or than the footer its own flags byte announces, longer than
// max_bytes, or without the connection bit.
TAMD_RECV_FN RecvFields tamd_recv_read_footer(const uint8_t* data, uint32_t bytes, uint32_t max_bytes) {
    RecvFields f = {0, 0, 0, 0, 0, 0, 0};
    if (bytes < TAMD_SEAL_UNTAGGED || bytes > max_bytes) return f;
    const uint32_t flags = data[bytes - 3u];
    if (!(flags & 0x80u) || bytes < tamd_recv_footer_bytes(flags)) return f;
    const uint32_t hs = tamd_recv_handshake_bytes(flags), nb = tamd_recv_nonce_bytes(flags), sb = tamd_recv_seq_bytes(flags);
    const uint32_t T = bytes - TAMD_SEAL_UNTAGGED;
    f.ts24 = data[T] | (uint32_t)data[T + 1u] << 8 | (uint32_t)data[T + 2u] << 16;
    f.partial_nonce = tamd_recv_field(data, T - hs, nb);
    f.partial_seq = tamd_recv_field(data, T - hs - nb, sb);
    f.flags = (uint8_t)flags;
    f.seq_bytes = (uint8_t)sb;
    f.nonce_bytes = (uint8_t)nb;
    f.handshake_bytes = (uint8_t)hs;
    return f;
}

// ---- the nonce ----

// The nonce a datagram with `nb` nonce bytes `partial` means when `largest` is the largest accepted
// so far: largest + 1 without nonce bytes, else largest plus the sign-extended 8 nb-bit difference
// (the generic ExpandFromTruncated and its 8- and 16-bit specialisations are this one rule).
TAMD_RECV_FN uint64_t tamd_recv_expand(uint64_t largest, uint32_t partial, uint32_t nb) {
    if (nb == 0u) return largest + 1u;
    const uint32_t bits = 8u * nb, mask = 0xffffffffu >> (32u - bits), msb = 1u << (bits - 1u);
    const uint32_t gap = (partial - (uint32_t)largest) & mask;
    return largest + (uint64_t)((int64_t)gap - (int64_t)(((uint64_t)gap & msb) << 1));
}

// ---- the register ----

// A stream's scalars in registers and its window in memory.
typedef struct tamd_recv_reg {
    uint64_t largest, base;
    uint32_t rotation;
    uint64_t* window;
} tamd_recv_reg;

TAMD_RECV_FN tamd_recv_reg tamd_recv_load(uint64_t* st) {
    tamd_recv_reg r;
    r.largest = st[TAMD_RECV_S_LARGEST];
    r.base = st[TAMD_RECV_S_BASE];
    r.rotation = (uint32_t)st[TAMD_RECV_S_ROTATION];
    r.window = st + TAMD_RECV_S_WINDOW;
    return r;
}
TAMD_RECV_FN void tamd_recv_store(uint64_t* st, const tamd_recv_reg& r) {
    st[TAMD_RECV_S_LARGEST] = r.largest;
    st[TAMD_RECV_S_BASE] = r.base;
    st[TAMD_RECV_S_ROTATION] = r.rotation;
}

// Reset(base) into the 67 words at st
TAMD_RECV_FN void tamd_recv_reset_state(uint64_t* st, uint64_t base) {
    st[TAMD_RECV_S_LARGEST] = base;
    st[TAMD_RECV_S_BASE] = base;
    st[TAMD_RECV_S_ROTATION] = 0;
    for (uint32_t k = 0; k < TAMD_RECV_WORDS; ++k) st[TAMD_RECV_S_WINDOW + k] = 0;
}

// IsDuplicate (StrikeRegister.cpp:62-80)
TAMD_RECV_FN bool tamd_recv_is_duplicate(const tamd_recv_reg& r, uint64_t seq) {
    if (tamd_recv_less(seq, r.base)) return true;  // too old to check
    const uint64_t distance = seq - r.base;
    if (distance >= TAMD_RECV_BITS) return false;
    const uint32_t bit = ((uint32_t)distance + r.rotation) % TAMD_RECV_BITS;
    return (r.window[bit / 64u] >> (bit % 64u)) & 1u;
}

// Accept (StrikeRegister.cpp:82-142)
TAMD_RECV_FN void tamd_recv_accept(tamd_recv_reg* r, uint64_t seq) {
    if (tamd_recv_less(r->largest, seq)) r->largest = seq;
    if (tamd_recv_less(seq, r->base)) return;
    uint64_t distance = seq - r->base;
    if (distance >= TAMD_RECV_BITS) {
        const uint64_t slide = (distance - TAMD_RECV_BITS) / 64u + 1u;
        if (slide >= TAMD_RECV_WORDS) {  // the whole window goes: Reset(seq), then its bit
            r->largest = seq;
            r->base = seq;
            r->rotation = 0;
            for (uint32_t k = 1; k < TAMD_RECV_WORDS; ++k) r->window[k] = 0;
            r->window[0] = 1;
            return;
        }
        uint32_t word = r->rotation / 64u;
        for (uint32_t k = 0; k < (uint32_t)slide; ++k) {
            r->window[word] = 0;
            word = word + 1u >= TAMD_RECV_WORDS ? 0u : word + 1u;
        }
        const uint32_t slide_bits = (uint32_t)slide * 64u;
        r->base += slide_bits;
        r->rotation += slide_bits;
        if (r->rotation >= TAMD_RECV_BITS) r->rotation -= TAMD_RECV_BITS;
        distance -= slide_bits;
    }
    const uint32_t bit = ((uint32_t)distance + r->rotation) % TAMD_RECV_BITS;
    r->window[bit / 64u] |= (uint64_t)1 << (bit % 64u);
}

// ---- the tag ----

// t1ha of the `len` bytes at `data` by one lane straight from memory, in aligned granules that
// hold at least one of the bytes: what the resolve step runs for a datagram whose guess was wrong.
TAMD_RECV_FN uint64_t tamd_recv_hash(const uint8_t* data, uint32_t len, uint64_t seed) {
    tamd_t1ha s;
    tamd_t1ha_init(&s, len, seed);
    const uintptr_t lo = (uintptr_t)data, hi = lo + len;
    for (uint32_t b = 0; b < s.blocks; ++b) {
        const tamd_v16 x = tamd_load16(lo + 32u * (uintptr_t)b, lo, hi), y = tamd_load16(lo + 32u * (uintptr_t)b + 16u, lo, hi);
        tamd_t1ha_block(&s, tamd_seal_u64(x, 0), tamd_seal_u64(x, 1), tamd_seal_u64(y, 0), tamd_seal_u64(y, 1));
    }
    if (!s.rem) return tamd_seal_hash_end(&s);
    const uintptr_t at = lo + 32u * (uintptr_t)s.blocks;
    tamd_v16 x = tamd_load16(at, lo, hi), y = {{0, 0, 0, 0}};
    if (s.rem > 16u) y = tamd_load16(at + 16u, lo, hi);
    const uint64_t w[4] = {tamd_seal_u64(x, 0), tamd_seal_u64(x, 1), tamd_seal_u64(y, 0), tamd_seal_u64(y, 1)};
    return tamd_t1ha_finish(&s, w);
}

// Whether the tag the valid datagram of `bytes` carries is the one `hash` (of its first bytes - 6
// bytes, seeded with nonce ^ key) makes.
TAMD_RECV_FN uint32_t tamd_recv_tag_ok(const tamd_seal_key& K, uint64_t hash, const uint8_t* data, uint32_t bytes) {
    const uint32_t T = bytes - TAMD_SEAL_UNTAGGED;
    const uint16_t stored = (uint16_t)(data[T + 4u] | data[T + 5u] << 8);
    return stored == tamd_seal_datagram_tag(K, hash, data, T) ? 1u : 0u;
}

// ---- the per-stream steps ----

// Predict: the nonce of each of the stream's `count` datagrams (items idx[0 .. count) of the call,
// in list order) if every datagram before it is accepted.  Reads the state, writes pred[] only.
TAMD_RECV_FN void tamd_recv_predict_stream(const uint64_t* st, const uint32_t* idx, uint32_t count, const RecvFields* f,
                                           uint64_t* pred) {
    uint64_t run = st[TAMD_RECV_S_LARGEST];
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t i = idx[k];
        const RecvFields fi = f[i];
        if (!fi.flags) {
            pred[i] = 0;
            continue;
        }
        const uint64_t nonce = tamd_recv_expand(run, fi.partial_nonce, fi.nonce_bytes);
        pred[i] = nonce;
        if (tamd_recv_less(run, nonce)) run = nonce;
    }
}

// Resolve: the stream's datagrams in list order against its state.  tag_ok[i] is the verdict under
// pred[i]; it counts only where the real nonce is pred[i].  Writes rc[i] (TAMD_RECV_*, with
// TAMD_RECV_REPAIRED when the tag was hashed here), res[i] unless the datagram is invalid, and
// clen[i], the bytes to decipher (0: none).
TAMD_RECV_FN void tamd_recv_resolve_stream(uint64_t* st, const tamd_seal_key& K, const uint32_t* idx, uint32_t count,
                                           const RecvDesc* d, const RecvFields* f, const uint64_t* pred, const uint32_t* tag_ok,
                                           uint32_t* rc, RecvResult* res, uint32_t* clen) {
    tamd_recv_reg r = tamd_recv_load(st);
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t i = idx[k];
        const RecvFields fi = f[i];
        clen[i] = 0;
        if (!fi.flags) {
            rc[i] = TAMD_RECV_INVALID;
            continue;
        }
        const RecvDesc di = d[i];
        const uint64_t nonce = tamd_recv_expand(r.largest, fi.partial_nonce, fi.nonce_bytes);
        RecvResult o;
        o.nonce = nonce;
        o.message_bytes = di.bytes - tamd_recv_footer_bytes(fi.flags);
        o.timestamp24 = fi.ts24;
        o.partial_seq = fi.partial_seq;
        o.flags = fi.flags;
        o.seq_bytes = fi.seq_bytes;
        o.nonce_bytes = fi.nonce_bytes;
        o.handshake_bytes = fi.handshake_bytes;
        res[i] = o;
        if (tamd_recv_is_duplicate(r, nonce)) {
            rc[i] = TAMD_RECV_DUPLICATE;
            continue;
        }
        uint32_t ok = tag_ok[i], repaired = 0;
        if (nonce != pred[i]) {
            const uint8_t* data = (const uint8_t*)di.data;
            ok = tamd_recv_tag_ok(K, tamd_recv_hash(data, di.bytes - TAMD_SEAL_UNTAGGED, nonce ^ tamd_seal_key64(K)), data, di.bytes);
            repaired = TAMD_RECV_REPAIRED;
        }
        if (!ok) {
            rc[i] = TAMD_RECV_BAD_TAG | repaired;
            continue;
        }
        tamd_recv_accept(&r, nonce);
        // seqBytes < nonceBytes && GetNextExpected() > nonce + 1, after the accept
        const bool reordered = fi.seq_bytes > 0 && fi.seq_bytes < fi.nonce_bytes && tamd_recv_less(nonce + 1u, r.largest + 1u);
        rc[i] = (reordered ? TAMD_RECV_REORDERED : TAMD_RECV_OK) | repaired;
        clen[i] = o.message_bytes;
    }
    tamd_recv_store(st, r);
}
