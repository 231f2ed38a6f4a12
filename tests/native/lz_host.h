// lz_host.h -- TEST ONLY.  The host compressor of the check programs (lz_check.cpp,
// unlz_check.cpp, lz_blocks.cpp): a plain greedy matcher standing in for the kernel's parse
// (lz_host_parse), then (lz_host_write, which lz_blocks also gives the kernel's own parse) the block as
// the kernel writes it through the host block writer of tonk_amd/csrc/lz.h: the literals as the
// smaller of the raw and the Huffman section, the sequence tables chosen by tamd_seq_choose, the
// backward sequence bit stream.
#pragma once
#include "../../tonk_amd/csrc/lz.h"

#include <string.h>
#include <vector>

struct LzHostOptions {
    // what lz_check varies
    bool huffman = true;      // Huffman literals where they are smaller than raw ones
    uint32_t minmatch = 4;    // shortest match taken
    bool fitted = true;       // block-fitted / RLE sequence tables (else the predefined ones)
    // guards of unlz_check (the defaults guard nothing)
    uint32_t floor = 0;       // a message below this many bytes is sent as is
    uint32_t len_cap = ~0u;   // match lengths and literal runs stay below this
    uint32_t max = ~0u;       // a block above the stream's maximum is not sent
    // what lz_blocks breaks on purpose (the defaults break nothing)
    uint32_t slack = 0;       // a block may exceed the message's length - 1 by this much
    uint32_t win_back = 0;    // matches may start this many bytes before the window
};

struct LzHostStats {
    std::vector<uint32_t> lo, off;  // the parse: literal length | match length << 16, match offset
    uint32_t lits = 0;              // literal bytes
    bool small = false;             // every literal is below TAMD_HUF_SYMS (a Huffman section is possible)
    bool huffman = false;           // the literals section is the Huffman one
    tamd_seq_tables tt;             // the block's tables (opt.fitted only)
    uint32_t hs = 0, dl = 0;        // bytes of the sequences header and of the table descriptions
    // the sequence bit stream: its offset in the block, the room it had (0: not written, the
    // block was already too long) and its bytes (0: it did not fit)
    uint32_t seq_at = 0, seq_room = 0, seq_bytes = 0;
};

// The parse: greedy matches of the n bytes at s + pos into st->lo / st->off; matches start at or
// after s + win (RingTrack::place).  `table`: the stream's hash table (1 << 14 entries, -1 when
// empty), updated.
static inline void lz_host_parse(const uint8_t* s, uint64_t pos, uint32_t n, uint64_t win, std::vector<int64_t>& table,
                                 const LzHostOptions& opt, LzHostStats* st) {
    std::vector<uint32_t>&lo = st->lo, &off = st->off;
    auto hash = [&](uint64_t p) {
        uint32_t w;
        memcpy(&w, s + p, 4);
        return (w * 2654435761u) >> 18;
    };
    uint32_t lit_start = 0, i = 0;
    while (i + 4 <= n) {  // greedy parse
        const uint64_t p = pos + i;
        const int64_t c = table[hash(p)];
        table[hash(p)] = (int64_t)p;
        uint32_t len = 0;
        if (c >= 0 && (uint64_t)c + opt.win_back >= win && (uint64_t)c < p)
            while (len < n - i && len < opt.len_cap && s[c + len] == s[p + len]) ++len;
        if (len >= opt.minmatch && i - lit_start < opt.len_cap) {
            lo.push_back((i - lit_start) | (len << 16));
            off.push_back((uint32_t)(p - (uint64_t)c));
            for (uint32_t j = 1; j < len && i + j + 4 <= n; ++j) table[hash(p + j)] = (int64_t)(p + j);
            i += len;
            lit_start = i;
        } else {
            ++i;
        }
    }
}

// The block of a parse (st->lo / st->off, made by lz_host_parse or read back from a block) of the
// n bytes at msg, as the kernel writes it.  Returns the block's size with the block in `out`, or 0
// when the message is to be sent as is.
static inline uint32_t lz_host_write(const uint8_t* msg, uint32_t n, const uint8_t* fse, const LzHostOptions& opt,
                                     std::vector<uint8_t>* outp, LzHostStats* st) {
    const std::vector<uint32_t>&lo = st->lo, &off = st->off;
    if (lo.empty() || n < opt.floor) return 0;
    uint32_t lit_start = 0;  // the end of the last match
    for (uint32_t v : lo) lit_start += (v & 0xffffu) + (v >> 16);
    std::vector<uint8_t>& out = *outp;
    out.assign(2 * (size_t)n + 256, 0);
    uint32_t lits = n - lit_start;
    for (uint32_t v : lo) lits += v & 0xffffu;
    st->lits = lits;
    // the literals in order, then the smaller of the raw and Huffman sections
    std::vector<uint8_t> litbuf;
    uint32_t src = 0;
    for (size_t q = 0; q <= lo.size(); ++q) {
        const uint32_t ll = q < lo.size() ? (lo[q] & 0xffffu) : n - lit_start;
        litbuf.insert(litbuf.end(), msg + src, msg + src + ll);
        if (q < lo.size()) src += ll + (lo[q] >> 16);
    }
    uint32_t count[TAMD_HUF_SYMS] = {0};
    st->small = true;
    for (uint8_t c : litbuf) {
        if (c >= TAMD_HUF_SYMS) st->small = false;
        else ++count[c];
    }
    const uint32_t raw = tamd_lits_header(lits, out.data()) + lits;
    uint32_t huf = 0;
    std::vector<uint8_t> hsec(raw + 64);
    if (opt.huffman && st->small) huf = tamd_huf_section(litbuf.data(), lits, count, hsec.data(), raw);
    uint32_t w;
    if (huf && huf < raw) {
        memcpy(out.data(), hsec.data(), huf);
        w = huf;
        st->huffman = true;
    } else {
        w = tamd_lits_header(lits, out.data());
        if (lits) memcpy(&out[w], litbuf.data(), lits);  // (no literals: litbuf has no data to point at)
        w += lits;
    }
    uint8_t h[4];
    const uint32_t hs = st->hs = tamd_seq_header((uint32_t)lo.size(), h);
    // the block's tables: codes packed as the kernel packs them
    std::vector<uint32_t> codes(lo.size());
    for (size_t q = 0; q < lo.size(); ++q)
        codes[q] = tamd_ll_code(lo[q] & 0xffffu) | (tamd_ml_code(lo[q] >> 16) << 8) |
                   ((31u - (uint32_t)__builtin_clz(off[q] + 3u)) << 16);
    if (opt.fitted) {
        st->dl = tamd_seq_choose(codes.data(), (uint32_t)codes.size(), fse, &st->tt);
        h[hs - 1] = (uint8_t)tamd_modes_byte(st->tt.mode);
    }
    memcpy(&out[w], h, hs);
    w += hs;
    if (opt.fitted) {
        const uint32_t order[3] = {0u, 2u, 1u};  // descriptions: LL, OF, ML
        for (uint32_t k : order) {
            memcpy(&out[w], st->tt.desc[k], st->tt.desc_len[k]);
            w += st->tt.desc_len[k];
        }
    }
    const uint32_t limit = n - 1 + opt.slack;  // the block stays below the message
    if (w >= limit) return 0;
    st->seq_at = w;
    st->seq_room = limit - w;
    st->seq_bytes = tamd_fse_sequences_t(lo.data(), off.data(), (uint32_t)lo.size(), fse, opt.fitted ? &st->tt : nullptr,
                                         &out[w], st->seq_room);
    w = st->seq_bytes ? w + st->seq_bytes : 0;
    return w && w <= limit && w <= opt.max ? w : 0;
}

// Compresses the n bytes at s + pos: the parse, then its block.
static inline uint32_t lz_host_block(const uint8_t* s, uint64_t pos, uint32_t n, uint64_t win, std::vector<int64_t>& table,
                                     const uint8_t* fse, const LzHostOptions& opt, std::vector<uint8_t>* outp,
                                     LzHostStats* st) {
    lz_host_parse(s, pos, n, win, table, opt, st);
    return lz_host_write(s + pos, n, fse, opt, outp, st);
}
