// unlz.h -- the reader of zstd compressed blocks (RFC 8878 s3.1.1.3) shared by the decompression
// kernel (unlz.hip), its host side (decompress.cpp) and the serial host walk of the tests
// (tests/native/unlz_check.cpp): literals section, Huffman tree description, sequences section,
// the state a stream carries from block to block (as the reference's DCtx does across
// ZSTD_decompressBlock calls) and the history ring of tonk::MessageDecompressor.
//
// The functions are written for `nl` cooperating lanes (lane = 0..nl-1) that all call them with
// the same arguments: the serial parts run on lane 0 (or one lane per Huffman stream), the copies
// and table fills are strided over the lanes, and TAMD_UNLZ_SYNC() separates a phase that writes
// shared memory from one that reads it.  The kernel runs them with a wave (nl = 64); on the host
// nl = 1 and TAMD_UNLZ_SYNC() is empty (the tests also run 64 lanes as fibres, the sync a
// barrier: unlz_check lanes).  No libc.
//
// Every read of the block, the literal buffer and the ring and every write of the ring and the
// output is bounded; a block that would step outside is rejected with a negative status.
#pragma once
#include "lz.h"

#ifndef TAMD_UNLZ_SYNC
#define TAMD_UNLZ_SYNC() do { } while (0)
#endif
// (the host walk of the tests counts which paths ran)
#ifndef TAMD_UNLZ_COUNT
#define TAMD_UNLZ_COUNT(what) do { } while (0)
#endif
enum {
    TAMD_CNT_LIT_RAW, TAMD_CNT_LIT_RLE, TAMD_CNT_LIT_HUF, TAMD_CNT_LIT_TREELESS, TAMD_CNT_HUF_1, TAMD_CNT_HUF_4,
    TAMD_CNT_W_DIRECT, TAMD_CNT_W_FSE, TAMD_CNT_NOSEQ,
    TAMD_CNT_LL_PREDEF, TAMD_CNT_LL_RLE, TAMD_CNT_LL_FSE, TAMD_CNT_LL_REPEAT,
    TAMD_CNT_ML_PREDEF, TAMD_CNT_ML_RLE, TAMD_CNT_ML_FSE, TAMD_CNT_ML_REPEAT,
    TAMD_CNT_OF_PREDEF, TAMD_CNT_OF_RLE, TAMD_CNT_OF_FSE, TAMD_CNT_OF_REPEAT,
    TAMD_CNT_OFF_NEW, TAMD_CNT_REP0, TAMD_CNT_REP1, TAMD_CNT_REP2, TAMD_CNT_REP_LL0_1, TAMD_CNT_REP_LL0_2,
    TAMD_CNT_REP_LL0_DEC, TAMD_CNT_EXT_MATCH, TAMD_CNT_EXT_CROSS, TAMD_CNT_OVERLAP, TAMD_CNT_RESTART,
    TAMD_CNT_N,
    // (behind the paths: the outcomes of tamd_unlz_block's decisions to wait for bytes just written)
    TAMD_CNT_WAIT_EXT = TAMD_CNT_N, TAMD_CNT_NOWAIT_EXT, TAMD_CNT_CROSS_REST, TAMD_CNT_CROSS_NONE,
    TAMD_CNT_WAIT_MATCH, TAMD_CNT_NOWAIT_MATCH,
    TAMD_CNT_ALL
};

#define TAMD_UNLZ_RING TAMD_LZ_DICT  // kCompressionDictBytes (lz.h)
#define TAMD_UNLZ_HUF_LOG 11u   // largest Huffman table log (RFC 8878 s4.2.1)
#define TAMD_UNLZ_LL_LOG 9u
#define TAMD_UNLZ_ML_LOG 9u
#define TAMD_UNLZ_OF_LOG 8u
#define TAMD_UNLZ_CHUNK 64u     // sequences decoded (one lane) before they are executed (all lanes)
#define TAMD_UNLZ_GUARD 8u      // (see tamd_unlz_resolve)

// status of a message: 0 or the reason the block was rejected
#define TAMD_UNLZ_OK 0
#define TAMD_UNLZ_E_SHORT (-1)       // the block ends inside a header or a section
#define TAMD_UNLZ_E_LITERALS (-2)    // literals section header: sizes inconsistent or over the limit
#define TAMD_UNLZ_E_HUFTREE (-3)     // Huffman tree description
#define TAMD_UNLZ_E_HUFSTREAM (-4)   // a Huffman stream is not consumed exactly
#define TAMD_UNLZ_E_NOTABLE (-5)     // Treeless / Repeat with no table from an earlier block
#define TAMD_UNLZ_E_SEQHEADER (-6)   // sequences section header, RLE symbol out of range
#define TAMD_UNLZ_E_NCOUNT (-7)      // FSE table description
#define TAMD_UNLZ_E_BITSTREAM (-8)   // sequence bit stream: no end mark, read past its start, bits left
#define TAMD_UNLZ_E_LITOVER (-9)     // the sequences use more literals than the block has
#define TAMD_UNLZ_E_OFFSET (-10)     // an offset reaches beyond the history
#define TAMD_UNLZ_E_DSTCAP (-11)     // the block restores more than the stream's maximum
#define TAMD_UNLZ_E_EMPTY (-12)      // the block restores nothing (Tonk treats 0 bytes as failure)
#define TAMD_UNLZ_E_FAILED (-13)     // an earlier block of the stream failed: not decoded
#define TAMD_UNLZ_E_SIZE (-14)       // message size 0 or above the stream's maximum

// What a stream keeps between blocks.  FSE entries: symbol | nbBits << 8 | next-state base << 16;
// Huffman entries: symbol | nbBits << 8.
typedef struct tamd_unlz_state {
    uint32_t rep[3];        // repeat offsets (start 1, 4, 8)
    uint32_t next;          // ring write offset = bytes of the current segment (it starts at offset 0)
    uint32_t dict_len;      // the previous segment: ring bytes [0, dict_len), zstd's external dictionary
    uint32_t have_huf, huf_log;
    uint32_t have_seq;      // a block with sequences has set the three tables (Repeat is allowed)
    uint32_t log[3];        // table logs: LL, ML, OF
    uint32_t predef[3];     // the table in use is the predefined one (`pre`), not fse[k]
    int32_t failed;
    uint32_t have_pre;      // `pre` is built (by the stream's first block that asks for one)
    uint32_t pre[160];      // the predefined tables: LL (64 states), ML (64), OF (32)
    uint16_t huf[1u << TAMD_UNLZ_HUF_LOG];
    uint32_t fse[3][1u << TAMD_UNLZ_LL_LOG];
} tamd_unlz_state;

// Working memory of one block (shared by the lanes; nothing in it outlives the block).
typedef struct tamd_unlz_work {
    int32_t status;
    uint32_t lit_type, lit_n, lit_rle, lit_at;  // type, count, the RLE byte, raw literals' offset in the block
    uint32_t lit_sel;             // decoded literals are in the second (large) buffer
    uint32_t n_streams, st_off[4], st_len[4], st_out[4], st_cnt[4];  // Huffman streams
    int32_t st_status[4];
    uint32_t tree_at, tree_len;   // Huffman tree description
    uint32_t seq_at;              // offset of the sequences section
    uint32_t modes, tab_at, tab_nsym, tab_log;  // its modes byte; the table description being read
    uint32_t nseq, seq_done, chunk_n;
    uint32_t br_at, br_n;         // the sequences' bit stream; bits not read yet
    int32_t br_left;
    uint32_t st[3];               // FSE states LL, ML, OF
    uint32_t rep[3];
    uint32_t lit_used, produced;
    uint32_t nsym, nbig;
    uint32_t rank[16];            // Huffman weights: symbols per weight, then table positions
    uint16_t hpos[256], hbig[32];
    uint8_t weights[256];
    int16_t norm[256];
    uint8_t spread[512];
    uint16_t nxt[256];
    uint32_t wtab[64];
    uint32_t seq_ll[TAMD_UNLZ_CHUNK], seq_ml[TAMD_UNLZ_CHUNK], seq_off[TAMD_UNLZ_CHUNK];
} tamd_unlz_work;

// ---- the kernel's interface (unlz.hip tamd_lz_decompress, decompress.cpp) ---------------------
// A stream's device memory: its tamd_unlz_state, then its ring.
#define TAMD_UNLZ_RING_AT ((uint32_t)((sizeof(tamd_unlz_state) + 63u) & ~63u))
#define TAMD_UNLZ_STREAM_BYTES (TAMD_UNLZ_RING_AT + ((TAMD_UNLZ_RING + 63u) & ~63u))
#define TAMD_UNLZ_FRESH 1u       // job flag: the stream starts here (its stored state is not read)
#define TAMD_UNLZ_KEEP 2u        // job flag: the state is written back after the job's last message
#define TAMD_UNLZ_NO_SCRATCH (~0ull)
#define TAMD_UNLZ_MSG_BLOCK 1u   // message flag: a compressed block (else: InsertUncompressed)
#define TAMD_UNLZ_MSG_QUIET 2u   // message flag: no output slot (history only)
#define TAMD_UNLZ_WAVES 8u       // jobs (waves) per workgroup

// A run of consecutive messages of one stream, decoded in order by one wave.
typedef struct tamd_unlz_job {
    uint8_t* stream;        // TAMD_UNLZ_STREAM_BYTES
    uint32_t first, count;  // its messages
    uint32_t cap, flags;    // the stream's maximum message size; TAMD_UNLZ_FRESH / KEEP
    uint64_t scratch;       // byte offset of `cap` bytes for the literals of large messages
} tamd_unlz_job;

// One message: byte offsets of its input and its output slot (`cap` bytes), its size.
typedef struct tamd_unlz_msg {
    uint64_t in, out;
    uint32_t bytes, flags, pad[2];
} tamd_unlz_msg;

TAMD_HD static inline void tamd_unlz_reset(tamd_unlz_state* S) {
    S->rep[0] = 1;
    S->rep[1] = 4;
    S->rep[2] = 8;
    S->next = S->dict_len = 0;
    S->have_huf = S->huf_log = S->have_seq = 0;
    for (uint32_t k = 0; k < 3; ++k) S->log[k] = S->predef[k] = 0;
    S->failed = 0;
    S->have_pre = 0;
}

// RingBuffer::Allocate(max) followed by zstd's continuity check (ZSTD_checkContinuity): a message
// placed where the previous one did not end starts a new segment at offset 0; the segment that
// just ended becomes the external dictionary and the one before it is dropped.
TAMD_HD static inline void tamd_unlz_place(tamd_unlz_state* S, uint32_t max) {
    if (S->next + max > TAMD_UNLZ_RING) {
        if (S->next) {
            S->dict_len = S->next;
            TAMD_UNLZ_COUNT(TAMD_CNT_RESTART);
        }
        S->next = 0;
    }
}

// ---- bit readers ----------------------------------------------------------------------------
// Bits [lo, lo + 64) of the n bytes at p taken as one little-endian number; bits outside it are 0.
TAMD_HD static inline uint64_t tamd_bits_window(const uint8_t* p, uint32_t n, int32_t lo8) {
    uint64_t w = 0;
    for (int32_t j = 0; j < 8; ++j) {
        const int32_t i = lo8 + j;
        if (i >= 0 && (uint32_t)i < n) w |= (uint64_t)p[i] << (8 * j);
    }
    return w;
}

// A stream read from its end (s4.1): `left` bits are unread; win caches bits [wlo, wlo + 64).
typedef struct tamd_bitr {
    const uint8_t* p;
    uint32_t n;
    int32_t left, wlo;
    uint64_t win;
    bool over;  // a read went past the stream's start
} tamd_bitr;

// The bits below the end mark of the stream's last byte; false without one.
TAMD_HD static inline bool tamd_bitr_open(tamd_bitr* r, const uint8_t* p, uint32_t n) {
    r->p = p;
    r->n = n;
    r->over = false;
    r->left = 0;
    r->wlo = 0;
    r->win = 0;
    if (n == 0 || n > 0x00ffffffu || p[n - 1] == 0) return false;
    r->left = (int32_t)(8u * (n - 1u) + (31u - (uint32_t)__builtin_clz((uint32_t)p[n - 1])));
    r->wlo = 0x40000000;  // (no window yet)
    return true;
}
TAMD_HD static inline void tamd_bitr_resume(tamd_bitr* r, const uint8_t* p, uint32_t n, int32_t left) {
    r->p = p;
    r->n = n;
    r->over = false;
    r->left = left;
    r->wlo = 0x40000000;
    r->win = 0;
}
// The next k <= 32 bits without consuming them; past the stream's start they read as 0.
TAMD_HD static inline uint32_t tamd_bitr_peek(tamd_bitr* r, uint32_t k) {
    if (!k) return 0;
    const int32_t lo = r->left - (int32_t)k;
    if (lo < r->wlo || r->left > r->wlo + 64) {
        r->wlo = ((r->left + 7) & ~7) - 64;
        r->win = tamd_bits_window(r->p, r->n, r->wlo / 8);  // (wlo is a multiple of 8, maybe negative)
    }
    const uint64_t v = r->win >> (uint32_t)(lo - r->wlo);
    return (uint32_t)(k >= 32 ? v : v & ((1ull << k) - 1ull));
}
TAMD_HD static inline void tamd_bitr_skip(tamd_bitr* r, uint32_t k) {
    if ((int32_t)k > r->left) {
        r->over = true;
        r->left = 0;
    } else {
        r->left -= (int32_t)k;
    }
}
TAMD_HD static inline uint32_t tamd_bitr_read(tamd_bitr* r, uint32_t k) {
    const uint32_t v = tamd_bitr_peek(r, k);
    tamd_bitr_skip(r, k);
    return v;
}

// k <= 16 bits at bit position `at` of a stream read from its start (the table descriptions).
TAMD_HD static inline uint32_t tamd_fwd_bits(const uint8_t* p, uint32_t n, uint32_t at, uint32_t k) {
    uint32_t v = 0;
    const uint32_t b = at >> 3;
    for (uint32_t j = 0; j < 4; ++j)
        if (b + j < n) v |= (uint32_t)p[b + j] << (8 * j);
    return (v >> (at & 7u)) & ((1u << k) - 1u);
}

// ---- FSE table description and decoding table (s4.1.1) --------------------------------------
// Normalized counts of symbols 0..max_sym from the `avail` bytes at p (at least 4, as the
// reference requires): norm[s] (-1: a "less than one" symbol), *nsym, *log, *used = its bytes.
TAMD_HD static inline int32_t tamd_unlz_ncount(const uint8_t* p, uint32_t avail, uint32_t max_sym, uint32_t max_log,
                                               int16_t* norm, uint32_t* nsym, uint32_t* log, uint32_t* used) {
    if (avail < 4) return TAMD_UNLZ_E_SHORT;
    if (avail > 0x01000000u) avail = 0x01000000u;
    uint32_t at = 4;
    const uint32_t lg = tamd_fwd_bits(p, avail, 0, 4) + 5u;
    if (lg > max_log) return TAMD_UNLZ_E_NCOUNT;
    int32_t remaining = (int32_t)(1u << lg) + 1, threshold = (int32_t)(1u << lg);
    uint32_t nb = lg + 1u, sym = 0;
    bool prev0 = false;
    while (remaining > 1 && sym <= max_sym) {
        if (prev0) {
            uint32_t n0 = sym;
            while (tamd_fwd_bits(p, avail, at, 16) == 0xffffu) {
                // (a run of 24 zero counts so close to the end that the reference stops refilling
                // its window: rejected here)
                if ((at >> 3) + 6u > avail) return TAMD_UNLZ_E_NCOUNT;
                n0 += 24;
                at += 16;
                if (n0 > max_sym) return TAMD_UNLZ_E_NCOUNT;
            }
            while (tamd_fwd_bits(p, avail, at, 2) == 3u) {
                n0 += 3;
                at += 2;
                if (n0 > max_sym) return TAMD_UNLZ_E_NCOUNT;
            }
            n0 += tamd_fwd_bits(p, avail, at, 2);
            at += 2;
            if (n0 > max_sym) return TAMD_UNLZ_E_NCOUNT;
            while (sym < n0) norm[sym++] = 0;
        }
        const int32_t mx = 2 * threshold - 1 - remaining;
        const uint32_t v = tamd_fwd_bits(p, avail, at, nb);
        int32_t count;
        if ((int32_t)(v & (uint32_t)(threshold - 1)) < mx) {
            count = (int32_t)(v & (uint32_t)(threshold - 1));
            at += nb - 1u;
        } else {
            count = (int32_t)(v & (uint32_t)(2 * threshold - 1));
            if (count >= threshold) count -= mx;
            at += nb;
        }
        --count;  // (the field is the count + 1; -1 = "less than one")
        remaining -= count < 0 ? -count : count;
        norm[sym++] = (int16_t)count;
        prev0 = count == 0;
        while (remaining < threshold && threshold > 1) {
            --nb;
            threshold >>= 1;
        }
        if (at > 8u * avail) return TAMD_UNLZ_E_SHORT;
    }
    if (remaining != 1) return TAMD_UNLZ_E_NCOUNT;
    if (at > 8u * avail) return TAMD_UNLZ_E_SHORT;
    *nsym = sym;
    *log = lg;
    *used = (at + 7u) >> 3;
    return TAMD_UNLZ_OK;
}

// The decoding table of normalized counts (FSE_buildDTable's layout: "less than one" symbols
// from the top, the others spread with step 5/8 size + 3, then per state its bit count and
// next-state base in the order of the states), built by `nl` lanes in three phases; the caller
// (tamd_unlz_fse_table) separates them with TAMD_UNLZ_SYNC().  spread: 1 << log bytes; nxt, cum:
// nsym entries.  The counts sum to the table size (tamd_unlz_ncount, the predefined tables).
//
// Phase 0, a lane per symbol: its first state number (nxt), the table entries that precede its
// own (cum, a prefix sum over the counts), and the place of a "less than one" symbol.
TAMD_HD static inline void tamd_unlz_fse_symbols(const int16_t* norm, uint32_t nsym, uint32_t log, uint8_t* spread,
                                                 uint16_t* nxt, uint16_t* cum, uint32_t lane, uint32_t nl) {
    const uint32_t size = 1u << log;
    for (uint32_t s = lane; s < nsym; s += nl) {
        uint32_t c = 0, low = 0;
        for (uint32_t t = 0; t < s; ++t) {
            const int32_t v = norm[t];
            c += v > 0 ? (uint32_t)v : 0u;
            low += v == -1;
        }
        cum[s] = (uint16_t)c;
        if (norm[s] == -1) {
            if (low < size) spread[size - 1u - low] = (uint8_t)s;
            nxt[s] = 1;
        } else {
            nxt[s] = (uint16_t)norm[s];
        }
    }
}

// Phase 1, a lane per step t of the spread: the walk visits (t * step) mod size and skips the
// places of the `nlow` "less than one" symbols at the top, so step t fills entry
// j = t - (skipped steps before t); a skipped place p is step p / step (mod size).  Entry j
// belongs to the last symbol whose cum is <= j.
TAMD_HD static inline void tamd_unlz_fse_spread(const int16_t* norm, uint32_t nsym, uint32_t log, uint8_t* spread,
                                                const uint16_t* cum, uint32_t lane, uint32_t nl) {
    const uint32_t size = 1u << log, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
    uint32_t nlow = 0;
    for (uint32_t t = 0; t < nsym; ++t) nlow += norm[t] == -1;
    if (nlow > size) nlow = size;
    uint32_t inv = step;  // 1 / step mod 2^32 (step is odd: Newton's iteration doubles the correct bits)
    for (uint32_t i = 0; i < 5; ++i) inv *= 2u - step * inv;
    for (uint32_t t = lane; t < size; t += nl) {
        const uint32_t pos = (t * step) & mask;
        if (pos + nlow >= size) continue;
        uint32_t j = t;
        for (uint32_t p = size - nlow; p < size; ++p) j -= ((p * inv) & mask) < t;
        uint32_t lo = 0, hi = nsym;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cum[mid] <= j) lo = mid;
            else hi = mid;
        }
        spread[pos] = (uint8_t)lo;
    }
}

// Phase 2, a lane per state, nl states [b, b + nl) at a time: state u of symbol s gets the number
// nxt[s] + (states of s in [b, u)).  Returns s | number << 8 | (the last state of s in this
// group) << 31, ~0 for no state; tamd_unlz_fse_put writes the entry and moves nxt[s] on.
TAMD_HD static inline uint32_t tamd_unlz_fse_number(const uint8_t* spread, const uint16_t* nxt, uint32_t log, uint32_t b,
                                                    uint32_t lane, uint32_t nl) {
    const uint32_t size = 1u << log, u = b + lane;
    if (u >= size) return ~0u;
    const uint32_t s = spread[u], lim = size - b < nl ? size - b : nl;
    uint32_t before = 0, after = 0;
    for (uint32_t i = 0; i < lim; ++i) {
        const uint32_t same = spread[b + i] == s;
        before += same & (i < lane);
        after += same & (i > lane);
    }
    uint32_t ns = (uint32_t)nxt[s] + before;
    if (ns == 0) ns = 1;  // (no symbol of the table has state number 0)
    return s | (ns << 8) | (after == 0 ? 0x80000000u : 0u);
}
TAMD_HD static inline void tamd_unlz_fse_put(uint32_t v, uint32_t* tab, uint16_t* nxt, uint32_t log, uint32_t b,
                                             uint32_t lane) {
    if (v == ~0u) return;
    const uint32_t size = 1u << log, s = v & 0xffu, ns = (v >> 8) & 0x7fffffu;
    const uint32_t nb = log - (31u - (uint32_t)__builtin_clz(ns));
    tab[b + lane] = s | (nb << 8) | (((ns << nb) - size) << 16);
    if (v >> 31) nxt[s] = (uint16_t)(ns + 1u);
}

// All `nl` lanes (nl = 1: one lane, serially).
TAMD_HD static inline void tamd_unlz_fse_table(const int16_t* norm, uint32_t nsym, uint32_t log, uint32_t* tab,
                                               uint8_t* spread, uint16_t* nxt, uint16_t* cum, uint32_t lane, uint32_t nl) {
    tamd_unlz_fse_symbols(norm, nsym, log, spread, nxt, cum, lane, nl);
    TAMD_UNLZ_SYNC();
    tamd_unlz_fse_spread(norm, nsym, log, spread, cum, lane, nl);
    TAMD_UNLZ_SYNC();
    for (uint32_t b = 0; b < (1u << log); b += nl) {
        const uint32_t v = tamd_unlz_fse_number(spread, nxt, log, b, lane, nl);
        TAMD_UNLZ_SYNC();  // (every lane has read nxt)
        tamd_unlz_fse_put(v, tab, nxt, log, b, lane);
        TAMD_UNLZ_SYNC();
    }
}

// The predefined distributions (s3.1.1.3.2.2.1-3), table k: 0 LL, 1 ML, 2 OF.  All lanes.
TAMD_HD static inline void tamd_unlz_predefined(uint32_t k, uint32_t* tab, int16_t* norm, uint8_t* spread, uint16_t* nxt,
                                                uint16_t* cum, uint32_t lane, uint32_t nl) {
    const int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                           2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    const int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                           1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    const int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    const uint32_t n = k == 0 ? 36u : k == 1 ? 53u : 29u;
    for (uint32_t s = lane; s < n; s += nl) norm[s] = k == 0 ? ll[s] : k == 1 ? ml[s] : of[s];
    TAMD_UNLZ_SYNC();
    tamd_unlz_fse_table(norm, n, k == 2 ? 5u : 6u, tab, spread, nxt, cum, lane, nl);
}

// ---- literals section (s3.1.1.3.1) ----------------------------------------------------------
// Header (lane 0's part): type, sizes, the streams' places.  Sets W->seq_at.
TAMD_HD static inline int32_t tamd_unlz_lit_header(const uint8_t* blk, uint32_t n, uint32_t cap, tamd_unlz_work* W) {
    if (n < 3) return TAMD_UNLZ_E_SHORT;  // (the reference's smallest block)
    const uint32_t type = blk[0] & 3u, fmt = (blk[0] >> 2) & 3u;
    W->lit_type = type;
    W->n_streams = 0;
    if (type < 2) {  // Raw, RLE
        uint32_t hs, ln;
        if (fmt == 1) {
            hs = 2;
            ln = ((uint32_t)blk[0] | ((uint32_t)blk[1] << 8)) >> 4;
        } else if (fmt == 3) {
            hs = 3;
            ln = ((uint32_t)blk[0] | ((uint32_t)blk[1] << 8) | ((uint32_t)blk[2] << 16)) >> 4;
        } else {
            hs = 1;
            ln = blk[0] >> 3;
        }
        if (ln > cap) return TAMD_UNLZ_E_LITERALS;  // (more literals than the stream's maximum)
        W->lit_n = ln;
        if (type == 0) {
            if (hs + ln > n) return TAMD_UNLZ_E_SHORT;
            W->lit_at = hs;
            W->seq_at = hs + ln;
            TAMD_UNLZ_COUNT(TAMD_CNT_LIT_RAW);
        } else {
            if (hs + 1 > n) return TAMD_UNLZ_E_SHORT;
            W->lit_rle = blk[hs];
            W->seq_at = hs + 1;
            TAMD_UNLZ_COUNT(TAMD_CNT_LIT_RLE);
        }
        return TAMD_UNLZ_OK;
    }
    if (n < 5) return TAMD_UNLZ_E_SHORT;
    uint32_t hs, ln, cs;
    const uint32_t h = (uint32_t)blk[0] | ((uint32_t)blk[1] << 8) | ((uint32_t)blk[2] << 16) | ((uint32_t)blk[3] << 24);
    if (fmt < 2) {
        hs = 3;
        ln = (h >> 4) & 0x3ffu;
        cs = (h >> 14) & 0x3ffu;
    } else if (fmt == 2) {
        hs = 4;
        ln = (h >> 4) & 0x3fffu;
        cs = h >> 18;
    } else {
        hs = 5;
        ln = (h >> 4) & 0x3ffffu;
        cs = (h >> 22) + ((uint32_t)blk[4] << 10);
    }
    if (ln == 0 || ln > cap) return TAMD_UNLZ_E_LITERALS;
    if (cs == 0 || hs + cs > n) return TAMD_UNLZ_E_SHORT;
    W->lit_n = ln;
    W->n_streams = fmt == 0 ? 1u : 4u;
    W->tree_at = hs;
    W->tree_len = cs;  // (tree description + streams; the tree's part is found by tamd_unlz_huf_weights)
    W->seq_at = hs + cs;
    TAMD_UNLZ_COUNT(type == 2 ? TAMD_CNT_LIT_HUF : TAMD_CNT_LIT_TREELESS);
    return TAMD_UNLZ_OK;
}

// Huffman tree description (s4.2.1) at d[0..avail): weights of the symbols into W->weights, the
// last one implied; *used = its bytes.  Lane 0.
TAMD_HD static inline int32_t tamd_unlz_huf_weights(const uint8_t* d, uint32_t avail, tamd_unlz_work* W, uint32_t* log_out,
                                                    uint32_t* used) {
    if (avail < 1) return TAMD_UNLZ_E_SHORT;
    uint32_t nw = 0, hb = d[0];
    if (hb >= 128) {  // direct: 4 bits per weight
        nw = hb - 127u;
        const uint32_t bytes = (nw + 1u) / 2u;
        if (1u + bytes > avail) return TAMD_UNLZ_E_SHORT;
        for (uint32_t i = 0; i < nw; ++i) W->weights[i] = (i & 1u) ? (d[1 + i / 2] & 15u) : (d[1 + i / 2] >> 4);
        *used = 1u + bytes;
        TAMD_UNLZ_COUNT(TAMD_CNT_W_DIRECT);
    } else {  // FSE-compressed: two interleaved states over one backward stream (s4.2.1.2)
        if (hb == 0 || 1u + hb > avail) return TAMD_UNLZ_E_SHORT;
        uint32_t nsym = 0, lg = 0, nc = 0;
        const int32_t rc = tamd_unlz_ncount(d + 1, hb, 255, 6, W->norm, &nsym, &lg, &nc);
        if (rc) return TAMD_UNLZ_E_HUFTREE;
        if (nc >= hb) return TAMD_UNLZ_E_HUFTREE;
        // (at most 64 states, inside lane 0's weight walk: built by this lane alone)
        tamd_unlz_fse_table(W->norm, nsym, lg, W->wtab, W->spread, W->nxt, W->hpos, 0, 1);
        tamd_bitr r;
        if (!tamd_bitr_open(&r, d + 1 + nc, hb - nc)) return TAMD_UNLZ_E_HUFTREE;
        uint32_t s1 = tamd_bitr_read(&r, lg), s2 = tamd_bitr_read(&r, lg);
        if (r.over) return TAMD_UNLZ_E_HUFTREE;
        // a state's symbol is emitted, then its update is read; the update that runs past the
        // stream's start ends the walk with the other state's symbol
        for (;;) {
            if (nw > 253) return TAMD_UNLZ_E_HUFTREE;
            uint32_t e = W->wtab[s1];
            W->weights[nw++] = (uint8_t)e;
            s1 = (e >> 16) + tamd_bitr_read(&r, (e >> 8) & 0xffu);
            if (r.over) {
                W->weights[nw++] = (uint8_t)W->wtab[s2];
                break;
            }
            if (nw > 253) return TAMD_UNLZ_E_HUFTREE;
            e = W->wtab[s2];
            W->weights[nw++] = (uint8_t)e;
            s2 = (e >> 16) + tamd_bitr_read(&r, (e >> 8) & 0xffu);
            if (r.over) {
                W->weights[nw++] = (uint8_t)W->wtab[s1];
                break;
            }
        }
        *used = 1u + hb;
        TAMD_UNLZ_COUNT(TAMD_CNT_W_FSE);
    }
    // the implied last weight completes the sum of 2^(w-1) to a power of two
    uint32_t total = 0;
    for (uint32_t i = 0; i < nw; ++i) {
        if (W->weights[i] > TAMD_UNLZ_HUF_LOG) return TAMD_UNLZ_E_HUFTREE;
        total += (1u << W->weights[i]) >> 1;
    }
    if (total == 0) return TAMD_UNLZ_E_HUFTREE;
    const uint32_t lg = 32u - (uint32_t)__builtin_clz(total);
    if (lg > TAMD_UNLZ_HUF_LOG) return TAMD_UNLZ_E_HUFTREE;
    const uint32_t rest = (1u << lg) - total;
    if (rest == 0 || (rest & (rest - 1u))) return TAMD_UNLZ_E_HUFTREE;
    W->weights[nw] = (uint8_t)(32u - (uint32_t)__builtin_clz(rest));
    W->nsym = nw + 1u;
    // table positions: by increasing weight, then symbol (HUF_readDTableX2's order); at least two
    // symbols of weight 1 and an even number of them, as the reference checks
    uint32_t* rank = W->rank;
    for (uint32_t w = 0; w < 16; ++w) rank[w] = 0;
    for (uint32_t i = 0; i < W->nsym; ++i) ++rank[W->weights[i]];
    if (rank[1] < 2 || (rank[1] & 1u)) return TAMD_UNLZ_E_HUFTREE;
    uint32_t start = 0;
    for (uint32_t w = 1; w <= lg; ++w) {
        const uint32_t c = rank[w];
        rank[w] = start;
        start += c << (w - 1u);
    }
    W->nbig = 0;
    for (uint32_t i = 0; i < W->nsym; ++i) {
        const uint32_t w = W->weights[i];
        if (!w) continue;
        W->hpos[i] = (uint16_t)rank[w];
        rank[w] += 1u << (w - 1u);
        if ((1u << (w - 1u)) >= 64u) W->hbig[W->nbig++] = (uint16_t)i;  // (at most 32 of them)
    }
    *log_out = lg;
    return TAMD_UNLZ_OK;
}

// Fills the decoding table from W->weights / W->hpos: a lane per symbol for the short runs, all
// lanes on each long one.
TAMD_HD static inline void tamd_unlz_huf_fill(const tamd_unlz_work* W, uint32_t log, uint16_t* tab, uint32_t lane,
                                              uint32_t nl) {
    for (uint32_t s = lane; s < W->nsym; s += nl) {
        const uint32_t w = W->weights[s];
        if (!w) continue;
        const uint32_t len = 1u << (w - 1u);
        if (len >= 64u) continue;
        const uint16_t e = (uint16_t)(s | ((log + 1u - w) << 8));
        for (uint32_t i = 0; i < len; ++i) tab[W->hpos[s] + i] = e;
    }
    for (uint32_t b = 0; b < W->nbig; ++b) {
        const uint32_t s = W->hbig[b], w = W->weights[s], len = 1u << (w - 1u);
        const uint16_t e = (uint16_t)(s | ((log + 1u - w) << 8));
        for (uint32_t i = lane; i < len; i += nl) tab[W->hpos[s] + i] = e;
    }
}

// One Huffman stream (s4.2.2): `cnt` symbols into out; the stream must be consumed exactly.
TAMD_HD static inline int32_t tamd_unlz_huf_stream(const uint8_t* p, uint32_t n, const uint16_t* tab, uint32_t log,
                                                   uint8_t* out, uint32_t cnt) {
    tamd_bitr r;
    if (!tamd_bitr_open(&r, p, n)) return TAMD_UNLZ_E_HUFSTREAM;
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t e = tab[tamd_bitr_peek(&r, log)];
        tamd_bitr_skip(&r, e >> 8);
        out[i] = (uint8_t)e;
    }
    return (r.over || r.left != 0) ? TAMD_UNLZ_E_HUFSTREAM : TAMD_UNLZ_OK;
}

// The whole literals section.  Decoded literals go to `lit` (lit_cap bytes) when they fit, else to
// `lit2` (lit2_cap bytes, may be null).  After it W->lit_type 0 = the literals are blk + W->lit_at,
// 1 = W->lit_rle repeated, else they are in the buffer W->lit_sel names.
TAMD_HD static inline int32_t tamd_unlz_literals(tamd_unlz_state* S, tamd_unlz_work* W, const uint8_t* blk, uint32_t n,
                                                 uint32_t cap, uint8_t* lit, uint32_t lit_cap, uint8_t* lit2,
                                                 uint32_t lit2_cap, uint32_t lane, uint32_t nl) {
    if (lane == 0) {
        int32_t rc = tamd_unlz_lit_header(blk, n, cap, W);
        W->lit_sel = 0;
        if (!rc && W->lit_type >= 2 && W->lit_n > lit_cap) {
            W->lit_sel = 1;
            if (!lit2 || W->lit_n > lit2_cap) rc = TAMD_UNLZ_E_LITERALS;
        }
        uint32_t at = W->tree_at, len = W->tree_len;
        if (!rc && W->lit_type == 3 && !S->have_huf) rc = TAMD_UNLZ_E_NOTABLE;
        if (!rc && W->lit_type == 2) {
            uint32_t used = 0, lg = 0;
            rc = tamd_unlz_huf_weights(blk + at, len, W, &lg, &used);
            if (!rc && used >= len) rc = TAMD_UNLZ_E_SHORT;
            if (!rc) {
                S->huf_log = lg;
                S->have_huf = 1;
                at += used;
                len -= used;
            }
        }
        if (!rc && W->lit_type >= 2) {
            const uint32_t ln = W->lit_n;
            if (W->n_streams == 1) {
                W->st_off[0] = at;
                W->st_len[0] = len;
                W->st_out[0] = 0;
                W->st_cnt[0] = ln;
                TAMD_UNLZ_COUNT(TAMD_CNT_HUF_1);
            } else {
                // jump table: three 16-bit sizes; the four streams decode ceil(n / 4) symbols each,
                // the last one the rest
                const uint32_t seg = (ln + 3u) / 4u;
                if (len < 10) rc = TAMD_UNLZ_E_SHORT;
                else if (3u * seg > ln) rc = TAMD_UNLZ_E_LITERALS;
                else {
                    uint32_t o = at + 6u, sum = 0;
                    for (uint32_t k = 0; k < 4; ++k) {
                        uint32_t l = k < 3 ? ((uint32_t)blk[at + 2 * k] | ((uint32_t)blk[at + 2 * k + 1] << 8)) : 0;
                        if (k == 3) {
                            if (sum + 6u >= len) {
                                rc = TAMD_UNLZ_E_SHORT;
                                break;
                            }
                            l = len - 6u - sum;
                        }
                        W->st_off[k] = o;
                        W->st_len[k] = l;
                        W->st_out[k] = k * seg;
                        W->st_cnt[k] = k < 3 ? seg : ln - 3u * seg;
                        o += l;
                        sum += l;
                        if (sum + 6u > len) {
                            rc = TAMD_UNLZ_E_SHORT;
                            break;
                        }
                    }
                    TAMD_UNLZ_COUNT(TAMD_CNT_HUF_4);
                }
            }
        }
        W->status = rc;
    }
    TAMD_UNLZ_SYNC();
    if (W->status) return W->status;
    if (W->lit_type < 2) return TAMD_UNLZ_OK;
    if (W->lit_type == 2) {
        tamd_unlz_huf_fill(W, S->huf_log, S->huf, lane, nl);
        TAMD_UNLZ_SYNC();
    }
    uint8_t* to = W->lit_sel ? lit2 : lit;
    for (uint32_t k = lane; k < W->n_streams; k += nl)
        W->st_status[k] = tamd_unlz_huf_stream(blk + W->st_off[k], W->st_len[k], S->huf, S->huf_log,
                                               to + W->st_out[k], W->st_cnt[k]);
    TAMD_UNLZ_SYNC();
    for (uint32_t k = 0; k < W->n_streams; ++k)
        if (W->st_status[k]) return W->st_status[k];
    return TAMD_UNLZ_OK;
}

// ---- sequences section (s3.1.1.3.2) ---------------------------------------------------------
// Header: the number of sequences and the modes byte.  Lane 0.  Sets W->nseq, W->modes, W->tab_at.
TAMD_HD static inline int32_t tamd_unlz_seq_counts(tamd_unlz_work* W, const uint8_t* blk, uint32_t n) {
    uint32_t at = W->seq_at;
    if (at >= n) return TAMD_UNLZ_E_SHORT;
    uint32_t ns = blk[at++];
    if (ns == 0) {
        W->nseq = 0;
        TAMD_UNLZ_COUNT(TAMD_CNT_NOSEQ);
        return at == n ? TAMD_UNLZ_OK : TAMD_UNLZ_E_SEQHEADER;  // (nothing may follow)
    }
    if (ns >= 128) {
        if (ns == 255) {
            if (at + 2 > n) return TAMD_UNLZ_E_SHORT;
            ns = ((uint32_t)blk[at] | ((uint32_t)blk[at + 1] << 8)) + 0x7f00u;
            at += 2;
        } else {
            if (at >= n) return TAMD_UNLZ_E_SHORT;
            ns = ((ns - 128u) << 8) + blk[at++];
        }
    }
    W->nseq = ns;
    if (at + 4 > n) return TAMD_UNLZ_E_SHORT;  // (modes byte + the reference's minimum behind it)
    const uint32_t modes = blk[at++];
    if (modes & 3u) return TAMD_UNLZ_E_SEQHEADER;  // reserved bits
    W->modes = modes;
    W->tab_at = at;
    return TAMD_UNLZ_OK;
}

// Table k's (0 LL, 1 ML, 2 OF) description at W->tab_at, mode `mode`.  Lane 0.  An FSE
// description leaves its counts in W->norm / W->tab_nsym / W->tab_log for the build.
TAMD_HD static inline int32_t tamd_unlz_seq_table_desc(tamd_unlz_state* S, tamd_unlz_work* W, const uint8_t* blk, uint32_t n,
                                                       uint32_t k, uint32_t mode) {
    const uint32_t max_sym = k == 0 ? 35u : k == 1 ? 52u : 31u;
    const uint32_t max_log = k == 0 ? TAMD_UNLZ_LL_LOG : k == 1 ? TAMD_UNLZ_ML_LOG : TAMD_UNLZ_OF_LOG;
    uint32_t at = W->tab_at;
    if (mode == 0) {
        S->predef[k] = 1;
        S->log[k] = k == 2 ? 5u : 6u;
        TAMD_UNLZ_COUNT(k == 0 ? TAMD_CNT_LL_PREDEF : k == 1 ? TAMD_CNT_ML_PREDEF : TAMD_CNT_OF_PREDEF);
    } else if (mode == 1) {
        if (at >= n) return TAMD_UNLZ_E_SHORT;
        const uint32_t s = blk[at++];
        if (s > max_sym) return TAMD_UNLZ_E_SEQHEADER;
        S->fse[k][0] = s;  // one state, no bits
        S->log[k] = 0;
        S->predef[k] = 0;
        TAMD_UNLZ_COUNT(k == 0 ? TAMD_CNT_LL_RLE : k == 1 ? TAMD_CNT_ML_RLE : TAMD_CNT_OF_RLE);
    } else if (mode == 2) {
        uint32_t nsym = 0, lg = 0, used = 0;
        const int32_t rc = tamd_unlz_ncount(blk + at, n - at, max_sym, max_log, W->norm, &nsym, &lg, &used);
        if (rc) return rc;
        W->tab_nsym = nsym;
        W->tab_log = lg;
        S->log[k] = lg;
        S->predef[k] = 0;
        at += used;
        TAMD_UNLZ_COUNT(k == 0 ? TAMD_CNT_LL_FSE : k == 1 ? TAMD_CNT_ML_FSE : TAMD_CNT_OF_FSE);
    } else {
        if (!S->have_seq) return TAMD_UNLZ_E_NOTABLE;
        TAMD_UNLZ_COUNT(k == 0 ? TAMD_CNT_LL_REPEAT : k == 1 ? TAMD_CNT_ML_REPEAT : TAMD_CNT_OF_REPEAT);
    }
    W->tab_at = at;
    return TAMD_UNLZ_OK;
}

// The bit stream behind the descriptions: its initial states.  Lane 0.
TAMD_HD static inline int32_t tamd_unlz_seq_open(tamd_unlz_state* S, tamd_unlz_work* W, const uint8_t* blk, uint32_t n) {
    const uint32_t at = W->tab_at;
    S->have_seq = 1;
    if (at >= n) return TAMD_UNLZ_E_SHORT;
    tamd_bitr r;
    if (!tamd_bitr_open(&r, blk + at, n - at)) return TAMD_UNLZ_E_BITSTREAM;
    W->st[0] = tamd_bitr_read(&r, S->log[0]);  // initial states: LL, OF, ML
    W->st[2] = tamd_bitr_read(&r, S->log[2]);
    W->st[1] = tamd_bitr_read(&r, S->log[1]);
    if (r.over) return TAMD_UNLZ_E_BITSTREAM;
    W->br_at = at;
    W->br_n = n - at;
    W->br_left = r.left;
    return TAMD_UNLZ_OK;
}

// Header, the three tables, the bit stream's initial states.  All lanes: lane 0 reads the header
// and each description, every lane builds the tables (a lane per symbol, then per state).
TAMD_HD static inline int32_t tamd_unlz_seq_header(tamd_unlz_state* S, tamd_unlz_work* W, const uint8_t* blk, uint32_t n,
                                                   uint32_t lane, uint32_t nl) {
    if (lane == 0) W->status = tamd_unlz_seq_counts(W, blk, n);
    TAMD_UNLZ_SYNC();
    if (W->status || W->nseq == 0) return W->status;
    const uint32_t modes = W->modes;
    for (uint32_t i = 0; i < 3; ++i) {  // descriptions: LL, OF, ML
        const uint32_t k = i == 0 ? 0u : i == 1 ? 2u : 1u;
        const uint32_t mode = k == 0 ? modes >> 6 : k == 2 ? (modes >> 4) & 3u : (modes >> 2) & 3u;
        if (lane == 0) W->status = tamd_unlz_seq_table_desc(S, W, blk, n, k, mode);
        TAMD_UNLZ_SYNC();
        if (W->status) return W->status;
        if (mode == 2) {
            tamd_unlz_fse_table(W->norm, W->tab_nsym, W->tab_log, S->fse[k], W->spread, W->nxt, W->hpos, lane, nl);
        } else if (mode == 0 && !S->have_pre) {
            for (uint32_t t = 0; t < 3; ++t) {
                tamd_unlz_predefined(t, S->pre + 64u * t, W->norm, W->spread, W->nxt, W->hpos, lane, nl);
                TAMD_UNLZ_SYNC();  // (W->norm is free again)
            }
            if (lane == 0) S->have_pre = 1;
            TAMD_UNLZ_SYNC();
        }
    }
    if (lane == 0) W->status = tamd_unlz_seq_open(S, W, blk, n);
    TAMD_UNLZ_SYNC();
    return W->status;
}

// Where a match of `len` bytes at `off` back from ring position q reads: *src (ring offset) and
// *len1 = the bytes read there before the copy continues at the segment's start (offset 0); 0 when
// the whole match is inside the current segment.  An offset past the segment's start resolves
// into the external dictionary [0, dict_len), measured from its end; the bytes are read as they
// physically are, also where the current segment has already overwritten them.  Not followed:
// an offset beyond the dictionary's start, and an external read that touches the
// TAMD_UNLZ_GUARD bytes from q on -- there the reference's wide copies have written ahead of the
// output, so what it reads is not a property of the stream.
TAMD_HD static inline int32_t tamd_unlz_resolve(uint32_t q, uint32_t off, uint32_t len, uint32_t dict_len, uint32_t* src,
                                                uint32_t* len1) {
    if (off <= q) {
        *src = q - off;
        *len1 = 0;
        if (off < len) TAMD_UNLZ_COUNT(TAMD_CNT_OVERLAP);
        return TAMD_UNLZ_OK;
    }
    const uint32_t k = off - q;
    if (k > dict_len) return TAMD_UNLZ_E_OFFSET;
    const uint32_t a = dict_len - k, l1 = len < k ? len : k;
    if (a < q + TAMD_UNLZ_GUARD && a + l1 > q) return TAMD_UNLZ_E_OFFSET;
    *src = a;
    *len1 = l1;
    TAMD_UNLZ_COUNT(TAMD_CNT_EXT_MATCH);
    if (len > k) TAMD_UNLZ_COUNT(TAMD_CNT_EXT_CROSS);
    return TAMD_UNLZ_OK;
}

// Decodes up to TAMD_UNLZ_CHUNK sequences into W->seq_* (lane 0): the FSE state walk, the value
// bits (offset, match length, literal length), the repeat offsets, and every bound the execution
// depends on.  q0 = ring offset of the block's first byte.
TAMD_HD static inline int32_t tamd_unlz_seq_chunk(const tamd_unlz_state* S, tamd_unlz_work* W, const uint8_t* blk,
                                                  uint32_t cap, uint32_t q0) {
    tamd_bitr r;
    tamd_bitr_resume(&r, blk + W->br_at, W->br_n, W->br_left);
    uint32_t done = W->seq_done, c = 0;
    uint32_t r0 = W->rep[0], r1 = W->rep[1], r2 = W->rep[2];
    uint32_t sl = W->st[0], sm = W->st[1], so = W->st[2];
    uint32_t lit_used = W->lit_used, produced = W->produced;
    int32_t rc = TAMD_UNLZ_OK;
    const uint32_t* tl = S->predef[0] ? S->pre : S->fse[0];
    const uint32_t* tm = S->predef[1] ? S->pre + 64 : S->fse[1];
    const uint32_t* to = S->predef[2] ? S->pre + 128 : S->fse[2];
    while (c < TAMD_UNLZ_CHUNK && done < W->nseq) {
        const uint32_t el = tl[sl], em = tm[sm], eo = to[so];
        const uint32_t llc = el & 0xffu, mlc = em & 0xffu, ofc = eo & 0xffu;
        uint32_t ov = ofc ? (1u << ofc) + tamd_bitr_read(&r, ofc) : 1u;  // Offset_Value (s3.1.1.3.2.1.1)
        const uint32_t ml = tamd_ml_base(mlc) + tamd_bitr_read(&r, tamd_ml_bits(mlc));
        const uint32_t ll = tamd_ll_base(llc) + tamd_bitr_read(&r, tamd_ll_bits(llc));
        uint32_t off;
        if (ov > 3) {
            off = ov - 3u;
            r2 = r1;
            r1 = r0;
            r0 = off;
            TAMD_UNLZ_COUNT(TAMD_CNT_OFF_NEW);
        } else {
            const uint32_t idx = ov - 1u + (ll == 0 ? 1u : 0u);  // with no literals the repeat codes shift by one
            if (idx == 0) {
                off = r0;
                TAMD_UNLZ_COUNT(TAMD_CNT_REP0);
            } else {
                uint32_t t = idx == 3 ? r0 - 1u : idx == 1 ? r1 : r2;
                if (t == 0) t = 1;  // (rep[0] - 1 = 0: the reference decodes with offset 1)
                if (idx != 1) r2 = r1;
                r1 = r0;
                r0 = off = t;
                if (ll) TAMD_UNLZ_COUNT(idx == 1 ? TAMD_CNT_REP1 : TAMD_CNT_REP2);
                else TAMD_UNLZ_COUNT(idx == 1 ? TAMD_CNT_REP_LL0_1 : idx == 2 ? TAMD_CNT_REP_LL0_2 : TAMD_CNT_REP_LL0_DEC);
            }
        }
        ++done;
        if (done < W->nseq) {  // state updates: LL, ML, OF
            sl = (el >> 16) + tamd_bitr_read(&r, (el >> 8) & 0xffu);
            sm = (em >> 16) + tamd_bitr_read(&r, (em >> 8) & 0xffu);
            so = (eo >> 16) + tamd_bitr_read(&r, (eo >> 8) & 0xffu);
        }
        if (r.over) {
            rc = TAMD_UNLZ_E_BITSTREAM;
            break;
        }
        if (ll > W->lit_n - lit_used) {
            rc = TAMD_UNLZ_E_LITOVER;
            break;
        }
        if (ll > cap - produced || ml > cap - produced - ll) {
            rc = TAMD_UNLZ_E_DSTCAP;
            break;
        }
        uint32_t src, len1;
        rc = tamd_unlz_resolve(q0 + produced + ll, off, ml, S->dict_len, &src, &len1);
        if (rc) break;
        W->seq_ll[c] = ll;
        W->seq_ml[c] = ml;
        W->seq_off[c] = off;
        lit_used += ll;
        produced += ll + ml;
        ++c;
    }
    if (!rc && done == W->nseq && r.left != 0) rc = TAMD_UNLZ_E_BITSTREAM;  // (consumed exactly)
    W->chunk_n = c;
    W->seq_done = done;
    W->rep[0] = r0;
    W->rep[1] = r1;
    W->rep[2] = r2;
    W->st[0] = sl;
    W->st[1] = sm;
    W->st[2] = so;
    W->lit_used = lit_used;
    W->produced = produced;
    W->br_left = r.left;
    return rc;
}

// `len` literals from position lp on to ring[q..] and out[o..] (all lanes).
TAMD_HD static inline void tamd_unlz_put_literals(const tamd_unlz_work* W, const uint8_t* blk, const uint8_t* lit,
                                                  uint32_t lp, uint32_t len, uint8_t* ring, uint32_t q, uint8_t* out,
                                                  uint32_t o, uint32_t lane, uint32_t nl) {
    const uint8_t* from = W->lit_type == 0 ? blk + W->lit_at : lit;
    for (uint32_t i = lane; i < len; i += nl) {
        const uint8_t b = W->lit_type == 1 ? (uint8_t)W->lit_rle : from[lp + i];
        ring[q + i] = b;
        out[o + i] = b;
    }
}

// ring[q + i] = out[o + i] = ring[src + (i mod period)], i < len (all lanes; period 0: no wrap).
TAMD_HD static inline void tamd_unlz_put_match(uint8_t* ring, uint32_t q, uint32_t src, uint32_t len, uint32_t period,
                                               uint8_t* out, uint32_t o, uint32_t lane, uint32_t nl) {
    for (uint32_t i = lane; i < len; i += nl) {
        const uint8_t b = ring[src + (period ? i % period : i)];
        ring[q + i] = b;
        out[o + i] = b;
    }
}

// One compressed block of a stream: restores it to out[0..) and to the ring at S->next (the
// caller has placed the message: tamd_unlz_place).  S and W are shared by the lanes; lit / lit2:
// the literal buffers (tamd_unlz_literals).  On success *restored = the bytes and the stream's state has
// moved on; on failure the state is left as it was wherever it matters (the caller marks the
// stream failed).
TAMD_HD static inline int32_t tamd_unlz_block(tamd_unlz_state* S, tamd_unlz_work* W, uint8_t* ring, const uint8_t* blk,
                                              uint32_t n, uint32_t cap, uint8_t* out, uint8_t* lit, uint32_t lit_cap,
                                              uint8_t* lit2, uint32_t lit2_cap, uint32_t lane, uint32_t nl,
                                              uint32_t* restored) {
    int32_t rc = tamd_unlz_literals(S, W, blk, n, cap, lit, lit_cap, lit2, lit2_cap, lane, nl);
    if (rc) return rc;
    if (W->lit_sel) lit = lit2;
    const uint32_t q0 = S->next;
    if (lane == 0) {
        W->seq_done = W->lit_used = W->produced = 0;
        for (uint32_t k = 0; k < 3; ++k) W->rep[k] = S->rep[k];
    }
    TAMD_UNLZ_SYNC();
    if (tamd_unlz_seq_header(S, W, blk, n, lane, nl)) return W->status;
    uint32_t lp = 0, p = 0;  // literals used, bytes produced by the executed sequences
    // bytes written since the last TAMD_UNLZ_SYNC are ring[dirty, q0 + p): a match that reads
    // them waits for them first
    uint32_t dirty = q0;
    while (W->seq_done < W->nseq) {
        TAMD_UNLZ_SYNC();  // (the chunk arrays are free again)
        if (lane == 0) W->status = tamd_unlz_seq_chunk(S, W, blk, cap, q0);
        TAMD_UNLZ_SYNC();
        dirty = q0 + p;
        const uint32_t cn = W->chunk_n;
        for (uint32_t c = 0; c < cn; ++c) {
            const uint32_t ll = W->seq_ll[c], ml = W->seq_ml[c], off = W->seq_off[c];
            tamd_unlz_put_literals(W, blk, lit, lp, ll, ring, q0 + p, out, p, lane, nl);
            lp += ll;
            p += ll;
            const uint32_t q = q0 + p;
            uint32_t src = 0, len1 = 0;
            tamd_unlz_resolve(q, off, ml, S->dict_len, &src, &len1);  // (checked by tamd_unlz_seq_chunk)
            if (len1) {  // external dictionary, then (maybe) on from the segment's start
                if (src + len1 > dirty && src < q) {
                    TAMD_UNLZ_COUNT(TAMD_CNT_WAIT_EXT);
                    TAMD_UNLZ_SYNC();
                    dirty = q;
                } else {
                    TAMD_UNLZ_COUNT(TAMD_CNT_NOWAIT_EXT);
                }
                tamd_unlz_put_match(ring, q, src, len1, 0, out, p, lane, nl);
                if (ml > len1) {
                    TAMD_UNLZ_COUNT(TAMD_CNT_CROSS_REST);
                    TAMD_UNLZ_SYNC();  // (the rest may read what was just written: distance = off)
                    dirty = q + len1;
                    tamd_unlz_put_match(ring, q + len1, 0, ml - len1, off, out, p + len1, lane, nl);
                } else {
                    TAMD_UNLZ_COUNT(TAMD_CNT_CROSS_NONE);
                }
            } else {
                if (q > dirty && src + (ml < off ? ml : off) > dirty) {
                    TAMD_UNLZ_COUNT(TAMD_CNT_WAIT_MATCH);
                    TAMD_UNLZ_SYNC();
                    dirty = q;
                } else {
                    TAMD_UNLZ_COUNT(TAMD_CNT_NOWAIT_MATCH);
                }
                tamd_unlz_put_match(ring, q, src, ml, off < ml ? off : 0u, out, p, lane, nl);
            }
            p += ml;
        }
        if (W->status) return W->status;
    }
    // the literals after the last sequence
    const uint32_t last = W->lit_n - lp;
    if (last > cap - p) return TAMD_UNLZ_E_DSTCAP;
    tamd_unlz_put_literals(W, blk, lit, lp, last, ring, q0 + p, out, p, lane, nl);
    p += last;
    if (p == 0) return TAMD_UNLZ_E_EMPTY;
    TAMD_UNLZ_SYNC();
    if (lane == 0) {
        for (uint32_t k = 0; k < 3; ++k) S->rep[k] = W->rep[k];
        S->next = q0 + p;
    }
    TAMD_UNLZ_SYNC();
    *restored = p;
    return TAMD_UNLZ_OK;
}

// MessageDecompressor::InsertUncompressed: the message enters the ring (and the output slot);
// the entropy state is untouched.
TAMD_HD static inline void tamd_unlz_insert(tamd_unlz_state* S, uint8_t* ring, const uint8_t* msg, uint32_t n, uint8_t* out,
                                            uint32_t lane, uint32_t nl) {
    const uint32_t q0 = S->next;
    for (uint32_t i = lane; i < n; i += nl) {
        const uint8_t b = msg[i];
        ring[q0 + i] = b;
        if (out) out[i] = b;
    }
    TAMD_UNLZ_SYNC();
    if (lane == 0) S->next = q0 + n;
    TAMD_UNLZ_SYNC();
}
