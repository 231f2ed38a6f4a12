// transcript.h -- text transcript of one workload stream, written the
// same way for every backend so runs can be compared line by line against the reference.
//
// Lines:
//   E rc len row cs sc ldpc h     encode: packet bytes (data+footer), footer metadata, FNV-1a
//   D rc n [num:len:h ...]        decode result and recovered packets (len = payload bytes)
//   K rd used h re next           decoder ack (result, bytes, digest) -> encoder ack result
//   a|O|R|X|T rc x y              add/original/recovery/ARQ/retransmit-delivery events with a
//                                 non-zero result
//   T rc [num bytes h]            siamese_encoder_retransmit: result, packet, payload digest
//   S e0..e7 d0..d9               final stats (the allocator-dependent MemoryUsed is omitted)
#pragma once
#include <stdio.h>
#include <stdarg.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "workload.h"

namespace tamd {
namespace wl {

struct TextSink {
    std::string text;
    void line(const char* s) { text += s; text += '\n'; }
    void put(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        text += buf;
    }
};

inline void fmt_encode_error(TextSink& t, int rc) { t.put("E %d\n", rc); }
inline void fmt_encode(TextSink& t, size_t total, unsigned row, unsigned cs, unsigned sc, unsigned ldpc, uint64_t h) {
    t.put("E 0 %zu %u %u %u %u %016llx\n", total, row, cs, sc, ldpc, (unsigned long long)h);
}
// A decode line: the head, one entry per recovered packet, and a newline.
inline void fmt_decode_head(TextSink& t, int rc, size_t n) { t.put("D %d %zu", rc, n); }
inline void fmt_decode_entry(TextSink& t, uint32_t num) { t.put(" %u", num); }
inline void fmt_decode_digest(TextSink& t, size_t len, uint64_t h) { t.put(":%zu:%016llx", len, (unsigned long long)h); }

inline void fmt_ack(TextSink& t, int rd, const uint8_t* buf, uint32_t used, int re, uint32_t next) {
    t.put("K %d %u %016llx %d %u\n", rd, used, (unsigned long long)fnv1a(buf, used), re, next);
}

inline void fmt_event(TextSink& t, char kind, int rc, uint32_t a, uint32_t b) {
    if (rc != 0) t.put("%c %d %u %u\n", kind, rc, a, b);
}

inline void fmt_retransmit(TextSink& t, int rc, uint32_t num, uint32_t bytes, uint64_t h) {
    if (rc != 0) t.put("T %d\n", rc);
    else t.put("T 0 %u %u %016llx\n", num, bytes, (unsigned long long)h);
}

inline void fmt_stats(TextSink& t, const uint64_t enc[9], const uint64_t dec[11]) {
    t.put("S");
    for (int i = 0; i < 8; ++i) t.put(" %llu", (unsigned long long)enc[i]);
    t.put(" |");
    for (int i = 0; i < 10; ++i) t.put(" %llu", (unsigned long long)dec[i]);
    t.put("\n");
}

// The transcript of a backend whose rows are computed after the line that reports them is due
// (programs run later, on the device or in the oracle's interpreter): an encode line is
// appended as "E ?" and a decode line with "#" after every packet number, and the owner fills
// them in (resolve_*) once it has the rows' digests.  `tag` is the owner's (where entry k's
// digest will be found).
struct DeferredTranscript {
    struct Enc { uint32_t row, total; unsigned meta[4]; size_t pos; uint64_t tag; };
    struct Dec { uint32_t row, upper; size_t pos; uint64_t tag; };
    std::vector<std::string> lines;
    std::vector<Enc> pend_enc;
    std::vector<Dec> pend_dec;

    void add(const TextSink& t) {  // one formatted line (or none)
        if (!t.text.empty()) lines.push_back(t.text.substr(0, t.text.size() - 1));
    }
    void encode(int rc, uint32_t row, uint32_t total, unsigned mrow, unsigned cs, unsigned sc, unsigned ldpc) {
        if (rc != 0) {
            TextSink t;
            fmt_encode_error(t, rc);
            return add(t);
        }
        pend_enc.push_back(Enc{row, total, {mrow, cs, sc, ldpc}, lines.size(), 0});
        lines.push_back("E ?");
    }
    // A recovered packet of the decode line appended next, in the line's order.
    void recovered(uint32_t row, uint32_t upper) { pend_dec.push_back(Dec{row, upper, lines.size(), 0}); }
    void decode(int rc, const std::vector<uint32_t>& nums) {
        TextSink t;
        fmt_decode_head(t, rc, nums.size());
        for (uint32_t n : nums) {
            fmt_decode_entry(t, n);
            t.text += '#';
        }
        lines.push_back(t.text);
    }
    void ack(int rd, const uint8_t* buf, uint32_t used, int re, uint32_t next) {
        TextSink t;
        fmt_ack(t, rd, buf, used, re, next);
        add(t);
    }
    void event(char kind, int rc, uint32_t a, uint32_t b) {
        TextSink t;
        fmt_event(t, kind, rc, a, b);
        add(t);
    }
    void retransmit(int rc, uint32_t num, uint32_t bytes, uint64_t h) {
        TextSink t;
        fmt_retransmit(t, rc, num, bytes, h);
        add(t);
    }
    void stats(const uint64_t e[9], const uint64_t d[11]) {
        TextSink t;
        fmt_stats(t, e, d);
        add(t);
    }
    void resolve_enc(size_t k, uint64_t h) {
        const Enc& e = pend_enc[k];
        TextSink t;
        fmt_encode(t, e.total, e.meta[0], e.meta[1], e.meta[2], e.meta[3], h);
        lines[e.pos] = t.text.substr(0, t.text.size() - 1);
    }
    void resolve_dec(size_t k, size_t len, uint64_t h) {
        std::string& ln = lines[pend_dec[k].pos];
        TextSink t;
        fmt_decode_digest(t, len, h);
        const size_t at = ln.find('#');
        if (at != std::string::npos) ln.replace(at, 1, t.text);
    }
    void resolved() {
        pend_enc.clear();
        pend_dec.clear();
    }
};

} // namespace wl
} // namespace tamd
