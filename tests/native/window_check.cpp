// window_check.cpp -- TEST ONLY.  The codecs' windows under batched adds against single adds, with
// no device (tests/test_window_runs.py).
//
// enc: two encoders on device-less contexts run under a virtual clock and receive one seeded
// schedule: adds of 1-63 packets (one through Encoder::add_run, with or without a layout, the
// other through single Encoder::add calls), clock steps of 0-30 ms, acknowledgements with 0-3
// loss ranges that cut segments mid-run (some acknowledge everything, so the next window starts
// with placeholders when its column is no multiple of 8), retransmit ticks and encodes (which move
// the window).  After every call both must agree on every live element's packet (row, offset,
// bytes, column, send time), the remaining slots, and the window / acknowledgement state line
// (count, next column, next expected column, RTO); every retransmit and encode result must agree
// too.  Each element's send time is also held against a per-element record kept here: the time
// of its add, moved by every retransmit that returned it.
//
// dec: two decoders receive the same in-order runs with gaps, one through
// Decoder::add_run_inorder, the other through add_original + is_ready; after every run their
// acknowledgements (next expected, got bits as loss ranges) and every element's packet agree.
//
// usage: window_check enc|dec seeds=S n=N [start=COLUMN] [trace=1]   (start: the encoder's first column)
// Prints one JSON line {"seeds":S,"checks":C,...} and exits 0, or the first difference and 1.
#include "../../tonk_amd/csrc/decoder.h"

#include <memory>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <string.h>

using namespace tamd;

static const uint32_t kRows = 2400, kRowBytes = 1344, kMaxUnacked = 300;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 0x1234567ull) {}
    uint32_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)(s >> 16);
    }
    uint32_t below(uint32_t n) { return next() % n; }
};

struct Side {
    Context ctx;
    std::unique_ptr<Encoder> enc;
    std::unique_ptr<Decoder> dec;
    uint64_t clock = 5000;
    std::vector<RowId> rows;
    uint32_t stride = 0;
    Side() {
        ctx.rows.init((uint64_t)kRows * kRowBytes + (64u << 20));
        for (uint32_t i = 0; i < kRows; ++i) rows.push_back(ctx.alloc(kRowBytes));
        stride = ctx.rows.offset(rows[1]) - ctx.rows.offset(rows[0]);
    }
    // the layout of rows[i..i + k), as the session's backend passes it (0: not one affine stretch)
    uint64_t layout(uint32_t i, uint32_t k) const {
        if (!consecutive_handles(&rows[i], k) || !ctx.rows.affine(rows[i], k, stride)) return 0;
        return (uint64_t)ctx.rows.offset(rows[i]) << 32 | stride;
    }
    void flush() {
        const uint64_t e = ctx.epoch;
        ctx.prepare_flush();
        ctx.finish_flush();
        ctx.rows.release_up_to(e);
    }
};

static uint64_t g_checks = 0;
static bool g_trace = false;  // trace=1: the state line after every call (to compare two builds of the codec)
// what the schedules reached: retransmits and encodes that returned a packet, loss ranges,
// windows that restarted on placeholders
static uint64_t g_retransmits = 0, g_encodes = 0, g_ranges = 0, g_placeholders = 0;
static int fail(const char* what, uint64_t seed, uint64_t call, const std::string& a, const std::string& b) {
    printf("seed %llu call %llu: %s differs\n  batched: %s\n  single:  %s\n", (unsigned long long)seed,
           (unsigned long long)call, what, a.c_str(), b.c_str());
    return 1;
}
static std::string show(int rc, const StoredOriginal& o) {
    char buf[160];
    snprintf(buf, sizeof(buf), "rc=%d row=%u off=%u bytes=%u column=%u send_msec=%u header=%u owned=%u", rc, o.row, o.off,
             o.bytes, o.column, o.send_msec, o.header_bytes, o.owned);
    return buf;
}

// ---- encoder ----

struct EncState {
    uint32_t next_col = 0;                 // the next add's column
    std::vector<uint32_t> sent;            // per column (mod period): the send time on record
    EncState() : sent(kColumnPeriod, 0) {}
};

static int enc_compare(Side& a, Side& b, const EncState& st, uint64_t seed, uint64_t call) {
    ++g_checks;
    if (a.enc->disabled() || b.enc->disabled()) return fail("disabled", seed, call, "-", "-");
    if (a.enc->remaining_slots() != b.enc->remaining_slots())
        return fail("remaining_slots", seed, call, std::to_string(a.enc->remaining_slots()),
                    std::to_string(b.enc->remaining_slots()));
    char la[512], lb[512];
    a.enc->debug_state(la, sizeof(la));
    b.enc->debug_state(lb, sizeof(lb));
    if (strcmp(la, lb)) return fail("state", seed, call, la, lb);
    if (g_trace) printf("%llu %llu %s\n", (unsigned long long)seed, (unsigned long long)call, la);
    const uint32_t count = kMaxPackets - a.enc->remaining_slots();
    const uint32_t column_start = col_sub(st.next_col, count);
    for (uint32_t e = 0; e < count; ++e) {
        const uint32_t col = col_add(column_start, e);
        StoredOriginal oa, ob;
        const int ra = a.enc->get(col, &oa), rb = b.enc->get(col, &ob);
        if (ra != rb || oa.row != ob.row || oa.off != ob.off || oa.bytes != ob.bytes || oa.column != ob.column ||
            oa.send_msec != ob.send_msec || oa.header_bytes != ob.header_bytes || oa.owned != ob.owned)
            return fail("element", seed, call, show(ra, oa), show(rb, ob));
        if (ra == kSuccess && (oa.column != col || oa.send_msec != st.sent[col]))
            return fail("element against the record", seed, call, show(ra, oa),
                        "column=" + std::to_string(col) + " send_msec=" + std::to_string(st.sent[col]));
    }
    return 0;
}

static int enc_seed(uint64_t seed, uint32_t n, uint32_t start) {
    Side a, b;
    a.enc.reset(new Encoder(&a.ctx, kRowBytes));
    b.enc.reset(new Encoder(&b.ctx, kRowBytes));
    a.enc->set_clock(&a.clock);
    b.enc->set_clock(&b.clock);
    Rng rng(seed);
    EncState st;
    uint64_t call = 0;
    uint32_t acked = 0;  // the last acknowledgement's next expected column
    // Reach the start column: batches that are acknowledged whole (both encoders alike).
    while (st.next_col != start) {
        const uint32_t k = std::min<uint32_t>(2048, start - st.next_col);
        uint32_t c0 = 0, c1 = 0;
        const uint32_t len = 700, hb = length_header_bytes(len);
        if (!a.enc->add_run(a.rows.data(), k, hb + len, hb, len, true, &c0) ||
            !b.enc->add_run(b.rows.data(), k, hb + len, hb, len, true, &c1) || c0 != st.next_col || c1 != c0)
            return fail("start run", seed, call, std::to_string(c0), std::to_string(c1));
        for (uint32_t j = 0; j < k; ++j) st.sent[col_add(c0, j)] = (uint32_t)a.clock;
        st.next_col = col_add(st.next_col, k);
        uint8_t buf[16] = {0};
        const uint32_t used = put_pnum_header(st.next_col, buf);
        uint32_t na = 0, nb = 0;
        if (a.enc->acknowledge(buf, used, &na) != kSuccess || b.enc->acknowledge(buf, used, &nb) != kSuccess)
            return fail("start acknowledgement", seed, call, std::to_string(na), std::to_string(nb));
        acked = st.next_col;
    }
    uint32_t added = 0, row_at = 0, len = 700;
    while (added < n) {
        ++call;
        const uint32_t unacked = col_sub(st.next_col, acked);
        uint32_t what = rng.below(100);
        if (what < 50 && unacked + 63 > kMaxUnacked) what = 70;  // (the window is bounded: acknowledge)
        if (what < 50) {
            const uint32_t k = 1 + rng.below(63);
            if (rng.below(4) == 0) len = rng.below(3) == 0 ? 60 : rng.below(2) ? 700 : 1300;
            if (rng.below(8) == 0) ++row_at;  // (the next handle is not the last one's successor)
            if (row_at + k + 1 > kRows) row_at = rng.below(7);
            const uint32_t hb = length_header_bytes(len);
            const uint64_t layout = rng.below(2) ? a.layout(row_at, k) : 0;
            uint32_t c0 = 0;
            if (!a.enc->add_run(&a.rows[row_at], k, hb + len, hb, len, true, &c0, layout))
                return fail("add_run", seed, call, "false", "-");
            for (uint32_t j = 0; j < k; ++j) {
                uint32_t c = 0;
                const int rc = b.enc->add(b.rows[row_at + j], hb + len, hb, len, nullptr, &c, true);
                if (rc != kSuccess || c != col_add(c0, j))
                    return fail("add", seed, call, std::to_string(col_add(c0, j)), std::to_string(c));
                st.sent[c] = (uint32_t)a.clock;
            }
            if (unacked == 0 && a.enc->remaining_slots() == kMaxPackets - k - c0 % kLanes && c0 % kLanes) ++g_placeholders;
            if (c0 != st.next_col) return fail("first column", seed, call, std::to_string(c0), std::to_string(st.next_col));
            st.next_col = col_add(st.next_col, k);
            row_at += k;
            added += k;
        } else if (what < 65) {
            a.clock += rng.below(31);
            b.clock = a.clock;
        } else if (what < 85) {
            // next expected anywhere in the unacknowledged range (its end: everything), then up to
            // three loss ranges; most fall inside the window, some leave it
            const uint32_t adv = rng.below(6) == 0 ? unacked : rng.below(unacked + 1);
            const uint32_t next = col_add(acked, adv);
            uint8_t buf[64] = {0};
            uint32_t used = put_pnum_header(next, buf);
            const uint32_t ranges = adv == unacked ? 0 : rng.below(4);
            for (uint32_t r = 0; r < ranges; ++r)
                used += put_nack_range(r ? rng.below(40) : 0, rng.below(5) == 0 ? rng.below(40) : rng.below(3), buf + used);
            uint32_t na = 0, nb = 0;
            const int ra = a.enc->acknowledge(buf, used, &na), rb = b.enc->acknowledge(buf, used, &nb);
            if (ra != rb || na != nb)
                return fail("acknowledge", seed, call, std::to_string(ra) + " next " + std::to_string(na),
                            std::to_string(rb) + " next " + std::to_string(nb));
            if (ra == kSuccess) acked = na;
            g_ranges += ranges;
        } else if (what < 95) {
            StoredOriginal oa, ob;
            const int ra = a.enc->retransmit(&oa), rb = b.enc->retransmit(&ob);
            if (ra != rb || (ra == kSuccess && (oa.row != ob.row || oa.off != ob.off || oa.bytes != ob.bytes ||
                                                oa.column != ob.column || oa.send_msec != ob.send_msec)))
                return fail("retransmit", seed, call, show(ra, oa), show(rb, ob));
            if (ra == kSuccess) {
                st.sent[oa.column] = (uint32_t)a.clock;
                ++g_retransmits;
            }
        } else {
            RecoveryOut ra, rb;
            const int ca = a.enc->encode(ra), cb = b.enc->encode(rb);
            if (ca != cb || ra.row != rb.row || ra.data_len != rb.data_len || ra.footer_len != rb.footer_len ||
                memcmp(ra.footer, rb.footer, sizeof(ra.footer)))
                return fail("encode", seed, call, std::to_string(ca) + " bytes " + std::to_string(ra.total()),
                            std::to_string(cb) + " bytes " + std::to_string(rb.total()));
            if (ca == kSuccess) {
                ++g_encodes;
                a.ctx.rows.free_deferred(ra.row);
                b.ctx.rows.free_deferred(rb.row);
            }
            if (rng.below(4) == 0) {
                a.flush();
                b.flush();
            }
        }
        if (enc_compare(a, b, st, seed, call)) return 1;
    }
    return 0;
}

// ---- decoder ----

static int dec_compare(Side& a, Side& b, uint32_t lo, uint32_t hi, uint64_t seed, uint64_t call) {
    ++g_checks;
    if (a.dec->disabled() || b.dec->disabled()) return fail("disabled", seed, call, "-", "-");
    uint8_t ba[2048], bb[2048];
    uint32_t ua = 0, ub = 0;
    const int ra = a.dec->ack(ba, sizeof(ba), &ua), rb = b.dec->ack(bb, sizeof(bb), &ub);
    if (ra != rb || ua != ub || memcmp(ba, bb, ua))
        return fail("acknowledgement", seed, call, std::to_string(ra) + " bytes " + std::to_string(ua),
                    std::to_string(rb) + " bytes " + std::to_string(ub));
    for (uint32_t col = lo; col < hi; ++col) {
        StoredOriginal* pa = nullptr;
        StoredOriginal* pb = nullptr;
        const int ga = a.dec->get(col, &pa), gb = b.dec->get(col, &pb);
        const StoredOriginal oa = ga == kSuccess ? *pa : StoredOriginal(), ob = gb == kSuccess ? *pb : StoredOriginal();
        if (ga != gb || oa.row != ob.row || oa.off != ob.off || oa.bytes != ob.bytes || oa.column != ob.column ||
            oa.header_bytes != ob.header_bytes)
            return fail("element", seed, call, show(ga, oa), show(gb, ob));
    }
    uint64_t sa[11], sb[11];
    a.dec->stats(sa, 11);
    b.dec->stats(sb, 11);
    if (memcmp(sa, sb, sizeof(sa))) return fail("statistics", seed, call, std::to_string(sa[0]), std::to_string(sb[0]));
    return 0;
}

static int dec_seed(uint64_t seed, uint32_t n) {
    Side a, b;
    a.dec.reset(new Decoder(&a.ctx, kRowBytes));
    b.dec.reset(new Decoder(&b.ctx, kRowBytes));
    Rng rng(seed);
    uint32_t col = 0, row_at = 0, len = 700;
    uint64_t call = 0;
    while (col < n) {
        ++call;
        if (rng.below(3) == 0) col += 1 + rng.below(3);  // lost originals before the run
        const uint32_t k = 1 + rng.below(63);
        if (rng.below(4) == 0) len = rng.below(3) == 0 ? 60 : rng.below(2) ? 700 : 1300;
        if (rng.below(8) == 0) ++row_at;
        if (row_at + k + 1 > kRows) row_at = rng.below(7);
        const uint32_t hb = length_header_bytes(len);
        const uint64_t layout = rng.below(2) ? a.layout(row_at, k) : 0;
        if (!a.dec->add_run_inorder(col, &a.rows[row_at], k, hb + len, hb, len, true, layout))
            return fail("add_run_inorder", seed, call, "false", "-");
        for (uint32_t j = 0; j < k; ++j) {
            bool took = false;
            const int rc = b.dec->add_original(col + j, b.rows[row_at + j], hb + len, hb, len, nullptr, &took, true);
            if (rc != kSuccess || b.dec->is_ready() == kSuccess)
                return fail("add_original", seed, call, "-", std::to_string(rc));
        }
        col += k;
        row_at += k;
        if (dec_compare(a, b, col > 400 ? col - 400 : 0, col + 8, seed, call)) return 1;
    }
    return dec_compare(a, b, 0, col + 8, seed, call);
}

int main(int argc, char** argv) {
    gf_init();
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    uint64_t seeds = 1, n = 2000, start = 0;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        const std::string k(argv[i], eq ? eq - argv[i] : 0);
        const unsigned long long v = eq ? strtoull(eq + 1, nullptr, 0) : 0;
        if (k == "seeds") seeds = v;
        else if (k == "n") n = v;
        else if (k == "start") start = v;
        else if (k == "trace") g_trace = v != 0;
        else return 2;
    }
    if (mode != "enc" && mode != "dec") return 2;
    if (start >= kColumnPeriod) return 2;
    for (uint64_t s = 0; s < seeds; ++s)
        if (mode == "enc" ? enc_seed(s, (uint32_t)n, (uint32_t)start) : dec_seed(s, (uint32_t)n)) return 1;
    printf("{\"mode\": \"%s\", \"seeds\": %llu, \"n\": %llu, \"start\": %llu, \"checks\": %llu, \"retransmits\": %llu, "
           "\"encodes\": %llu, \"loss_ranges\": %llu, \"placeholder_windows\": %llu}\n",
           mode.c_str(), (unsigned long long)seeds, (unsigned long long)n, (unsigned long long)start,
           (unsigned long long)g_checks, (unsigned long long)g_retransmits, (unsigned long long)g_encodes,
           (unsigned long long)g_ranges, (unsigned long long)g_placeholders);
    return 0;
}
