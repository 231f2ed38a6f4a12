// impaired.h -- TEST INFRASTRUCTURE.  A second channel model beside tamd::wl::Runner
// (tonk_amd/csrc/workload.h): the same stream of originals, recovery packets, acknowledgements,
// ARQ and retransmissions, over a channel that also REORDERS and DUPLICATES packets and drops,
// delays and repeats acknowledgements -- a reliable-UDP transport's ordinary weather, which
// Runner's in-order channel never produces.
//
// The driver is a template over the Backend and Transcript concepts of workload.h:221-247 and
// makes single calls only (no enc_add_run / dec_add_run).  Two more backend methods:
//   RecRef   rec_copy(const RecRef&)   -- a second packet holding the same bytes (a recovery
//                                         packet handed over twice: the decoder may have taken
//                                         the first)
//   uint32_t rec_end(const RecRef&)    -- (ColumnStart + SumCount) mod 2^22 of its footer
//
// All decisions are integer arithmetic.  The loss draws are LossChannel's, one per packet sent,
// in Runner's order; every new draw comes from one PCG stream of its own (seed_impair), a fixed
// number per event, so a scenario's loss pattern -- and every other impairment's draws -- stay
// where they are when one impairment is switched on.  With every impairment zero the driver makes
// exactly Runner's calls and writes exactly Runner's transcript.
//
// Slots.  One slot is one packet sent through the lossy channel: an original, a recovery packet
// or a retransmission, in send order.  A packet the loss process delivers arrives at once,
// unless a draw below `reorder` holds it for 1 + draw % reach slots (the first `hold_first`
// originals are held for hold_first slots whatever the draw); a draw below `dup` schedules a
// second copy, held for 1 + draw % reach slots.  Held packets arrive after the packet of their
// due slot, in (due slot, send sequence) order, before that slot's recovery tokens,
// acknowledgement, retransmission tick and ARQ.  have_, ARQ and retransmission follow Runner's
// rules: an original not yet arrived when its ARQ lag runs out is redelivered, and its held copy
// then arrives as a duplicate.  At the end every held packet (then every held acknowledgement)
// is delivered before the lossless, undelayed flush begins.
//
// Acknowledgements.  One the decoder writes is dropped on a draw below `ackloss`, else held for
// draw % (ackreach + 1) acknowledgement intervals on a draw below `ackdelay`, else due now; due
// ones are delivered oldest-due first, so a held one reaches the encoder after a newer one (the
// stale acknowledgement).  A draw below `ackdup` delivers it twice in succession (the repeat).
//
// Transcript: transcript.h's lines, and five event letters of this driver (first field after the
// letter is never 0, so the line is always written):
//   H copy col rc        an original arriving late: copy 1 held, 2 second copy; rc of add_original
//   Q copy behind rc     a recovery packet arriving late: copy as above; behind = 1 when its
//                        ColumnStart + SumCount lies below that of an earlier delivered one
//   L 1 seq used         an acknowledgement dropped (its K line follows, encoder result -1)
//   V 1 seq newest       an acknowledgement arriving after a newer one (its K line follows)
//   P 1 seq 0            the repeat of an acknowledgement (its second K line follows)
#pragma once

#include "../tonk_amd/csrc/workload.h"

#include <map>
#include <utility>

namespace tamd {
namespace wl {

// Thresholds are in 1/2^32 units, as Params::loss_thresh.
struct Impair {
    uint32_t reorder = 0, reach = 1, dup = 0;
    uint32_t ackloss = 0, ackdelay = 0, ackreach = 0, ackdup = 0;
    uint32_t hold_first = 0;
    uint64_t seed_impair = 3000;
};

inline bool parse_impair(Impair& m, const std::string& k, unsigned long long v) {
    if (k == "reorder") m.reorder = (uint32_t)v;
    else if (k == "reach") m.reach = (uint32_t)v;
    else if (k == "dup") m.dup = (uint32_t)v;
    else if (k == "ackloss") m.ackloss = (uint32_t)v;
    else if (k == "ackdelay") m.ackdelay = (uint32_t)v;
    else if (k == "ackreach") m.ackreach = (uint32_t)v;
    else if (k == "ackdup") m.ackdup = (uint32_t)v;
    else if (k == "hold_first") m.hold_first = (uint32_t)v;
    else if (k == "seed_impair") m.seed_impair = v;
    else return false;
    return true;
}

template <class Backend, class Transcript>
class ImpairedRunner {
public:
    ImpairedRunner(const Params& p, const Impair& m, Backend& be, Transcript& tr) : p_(p), m_(m), be_(be), tr_(tr) {
        ch_.init(p_);
        rng_.seed(m_.seed_impair, 0);
        ack_countdown_ = p_.ack_every;
        rtx_countdown_ = p_.rtx_every;
        now_ms_ = kVirtualClockStart;
        have_.assign(p_.n_originals, 0);
        col_of_.assign(p_.n_originals, 0);
    }

    const Summary& summary() const { return s_; }

    void finish() {
        for (uint32_t i = 0; i < p_.n_originals; ++i) one(i);
        deliver_due(~0ull);
        deliver_acks(~0ull);
        for (uint32_t k = 0; k < p_.flush_max; ++k) {
            while (scan_ < p_.n_originals && have_[scan_]) ++scan_;
            if (scan_ == p_.n_originals) break;
            ++s_.flush_encodes;
            send_recovery(false);
        }
        for (uint32_t i = 0; i < p_.n_originals; ++i) if (!have_[i]) ++s_.missing_at_end;
        uint64_t es[9] = {0}, ds[11] = {0};
        be_.stats(es, ds);
        tr_.on_stats(es, ds);
    }

private:
    typedef typename Backend::RecRef RecRef;
    struct Held {
        char kind;       // 'O' original, 'T' retransmitted original, 'R' recovery packet
        uint32_t copy;   // 1 the held packet, 2 its second copy
        uint32_t col, idx, len;
        RecRef rec;
    };
    struct Ack {
        uint32_t seq;
        int rd;
        std::vector<uint8_t> bytes;
        bool twice;
    };
    typedef std::pair<uint64_t, uint64_t> Key;  // (due, send sequence)

    const Params& p_;
    const Impair& m_;
    Backend& be_;
    Transcript& tr_;
    Summary s_;
    LossChannel ch_;
    Pcg rng_;
    std::vector<uint8_t> have_;
    std::vector<uint32_t> col_of_, pending_arq_;
    size_t arq_head_ = 0;
    uint32_t tokens_ = 0, top_ = 0, scan_ = 0;
    uint32_t ack_countdown_ = 0, rtx_countdown_ = 0;
    uint64_t now_ms_ = 0;
    std::vector<uint32_t> nums_;
    std::vector<uint8_t> rtx_buf_;
    uint64_t slot_ = 0, seq_ = 0;
    std::map<Key, Held> held_;
    uint64_t ack_time_ = 0;         // acknowledgement intervals so far
    uint32_t ack_seq_ = 0;          // acknowledgements written
    uint32_t newest_ack_ = 0;       // newest delivered (any_ack_)
    bool any_ack_ = false;
    std::map<Key, Ack> acks_;
    uint32_t latest_end_ = 0;       // highest ColumnStart + SumCount delivered (any_rec_)
    bool any_rec_ = false;

    // The impairment draws of one packet the loss process delivered: four, whatever is on.
    struct Fate { uint32_t hold, dup_hold; };
    Fate fate() {
        const uint32_t a = rng_.next(), b = rng_.next(), c = rng_.next(), d = rng_.next();
        const uint32_t reach = m_.reach ? m_.reach : 1;
        Fate f = {0, 0};
        if (a < m_.reorder) f.hold = 1 + b % reach;
        if (c < m_.dup) f.dup_hold = 1 + d % reach;
        return f;
    }

    void decode_loop() {
        while (be_.dec_is_ready() == 0) {
            nums_.clear();
            typename Backend::DecRef dref;
            const int rc = be_.dec_decode(nums_, dref);
            ++s_.decode_calls;
            tr_.on_decode(rc, nums_, dref);
            if (rc != 0) break;
            for (uint32_t c : nums_) {
                const uint32_t i = index_of_column(c, top_);
                if (i < p_.n_originals && !have_[i]) { have_[i] = 1; ++s_.recovered; }
            }
            if (nums_.empty()) break;
        }
    }

    // An original reaches the decoder (`copy` 0: at once, as Runner delivers it).
    void deliver_original(char kind, uint32_t copy, uint32_t col, uint32_t idx, uint32_t len) {
        const int ro = be_.dec_add_original(col, idx, len);
        if (copy) tr_.on_event('H', (int)copy, col, (uint32_t)ro);
        else tr_.on_event(kind, ro, col, 0);
        if (!have_[idx]) have_[idx] = 1;
        decode_loop();
    }

    void deliver_recovery(const RecRef& r, uint32_t copy) {
        const uint32_t end = be_.rec_end(r) & 0x3fffffu;
        const bool behind = any_rec_ && (((end - latest_end_) & 0x3fffffu) >> 21) != 0;
        if (!behind) {
            latest_end_ = end;
            any_rec_ = true;
        }
        const int rr = be_.dec_add_recovery(r);
        if (copy) tr_.on_event('Q', (int)copy, behind ? 1 : 0, (uint32_t)rr);
        else tr_.on_event('R', rr, 0, 0);
        decode_loop();
    }

    // Held packets due at or before `slot`, in (due slot, send sequence) order.
    void deliver_due(uint64_t slot) {
        while (!held_.empty() && held_.begin()->first.first <= slot) {
            Held h = std::move(held_.begin()->second);
            held_.erase(held_.begin());
            if (h.kind == 'R') deliver_recovery(h.rec, h.copy);
            else deliver_original(h.kind, h.copy, h.col, h.idx, h.len);
        }
    }
    void end_slot() {
        deliver_due(slot_);
        ++slot_;
    }

    // An original (first transmission 'O' or retransmission 'T') the loss process delivered.
    // Returns false when its first copy is held.
    bool send_original(char kind, uint32_t col, uint32_t idx, uint32_t len) {
        Fate f = fate();
        if (kind == 'O' && idx < m_.hold_first && f.hold < m_.hold_first) f.hold = m_.hold_first;
        if (f.dup_hold) held_.emplace(Key(slot_ + f.dup_hold, seq_++), Held{kind, 2, col, idx, len, RecRef()});
        if (f.hold) {
            held_.emplace(Key(slot_ + f.hold, seq_++), Held{kind, 1, col, idx, len, RecRef()});
            return false;
        }
        deliver_original(kind, 0, col, idx, len);
        return true;
    }

    void send_recovery(bool lossy) {
        RecRef r;
        const int rc = be_.enc_encode(r);
        tr_.on_encode(rc, r);
        if (rc != 0) return;
        ++s_.recoveries;
        if (!lossy) return deliver_recovery(r, 0);  // (the flush: no slot, undelayed)
        if (p_.loss_on_recovery && ch_.lost()) {
            ++s_.lost_recoveries;
            be_.recovery_lost(r);
            return end_slot();
        }
        const Fate f = fate();
        // (the copy first: the decoder may take the packet it is handed)
        if (f.dup_hold) held_.emplace(Key(slot_ + f.dup_hold, seq_++), Held{'R', 2, 0, 0, 0, be_.rec_copy(r)});
        if (f.hold) held_.emplace(Key(slot_ + f.hold, seq_++), Held{'R', 1, 0, 0, 0, r});
        else deliver_recovery(r, 0);
        end_slot();
    }

    void retransmit_tick() {
        for (uint32_t k = 0; k < kRtxPerTick; ++k) {
            uint32_t num = 0, bytes = 0;
            const uint8_t* data = nullptr;
            const int rc = be_.enc_retransmit(&num, &bytes, &data);
            uint64_t h = 0;
            const uint32_t idx = index_of_column(num, top_);
            if (rc == 0) {
                if (!data && idx < p_.n_originals) {
                    rtx_buf_.resize(bytes ? bytes : 1);
                    payload_bytes(p_, idx, rtx_buf_.data(), bytes);
                    data = rtx_buf_.data();
                }
                h = data ? fnv1a(data, bytes) : 0;
            }
            tr_.on_retransmit(rc, num, bytes, h);
            if (rc != 0) break;
            ++s_.retransmits;
            if (!ch_.lost() && idx < p_.n_originals) send_original('T', num, idx, bytes);
            end_slot();
        }
    }

    void deliver_ack(const Ack& a) {
        const bool stale = any_ack_ && a.seq < newest_ack_;
        if (stale) tr_.on_event('V', 1, a.seq, newest_ack_);
        else {
            newest_ack_ = a.seq;
            any_ack_ = true;
        }
        for (int round = 0; round < (a.twice ? 2 : 1); ++round) {
            if (round) tr_.on_event('P', 1, a.seq, 0);
            uint32_t next = 0;
            const int re = be_.enc_ack(a.bytes.data(), (uint32_t)a.bytes.size(), &next);
            tr_.on_ack(a.rd, a.bytes.data(), (uint32_t)a.bytes.size(), re, next);
        }
    }
    void deliver_acks(uint64_t time) {
        while (!acks_.empty() && acks_.begin()->first.first <= time) {
            const Ack a = std::move(acks_.begin()->second);
            acks_.erase(acks_.begin());
            deliver_ack(a);
        }
    }

    // The decoder's acknowledgement and its way to the encoder: four draws, whatever is on.
    void ack_tick() {
        uint8_t buf[2048];
        const uint32_t limit = p_.ack_bytes < sizeof(buf) ? p_.ack_bytes : (uint32_t)sizeof(buf);
        uint32_t used = 0;
        const int rd = be_.dec_ack(buf, limit, &used);
        ++s_.acks;
        const uint32_t a = rng_.next(), b = rng_.next(), c = rng_.next(), d = rng_.next();
        const uint32_t seq = ack_seq_++;
        if (rd != 0 || used == 0) {
            tr_.on_ack(rd, buf, used, -1, 0);  // nothing to send (as Runner::exchange_ack)
        } else if (a < m_.ackloss) {
            tr_.on_event('L', 1, seq, used);
            tr_.on_ack(rd, buf, used, -1, 0);
        } else {
            const uint64_t wait = b < m_.ackdelay ? c % (m_.ackreach + 1) : 0;
            acks_.emplace(Key(ack_time_ + wait, seq), Ack{seq, rd, std::vector<uint8_t>(buf, buf + used), d < m_.ackdup});
        }
        deliver_acks(ack_time_);
        ++ack_time_;
    }

    // One original: add, channel (a slot), then what Runner::events_after does.
    void one(uint32_t i) {
        if (p_.rtx_every) {
            now_ms_ += p_.rtx_msec;
            be_.set_time(now_ms_);
        }
        const uint32_t len = payload_length(p_, i);
        uint32_t col = 0;
        const int ra = be_.enc_add(i, len, &col);
        tr_.on_event('a', ra, i, col);
        if (ra == 0) top_ = i + 1;
        col_of_[i] = col;
        ++s_.originals;
        if (ch_.lost()) {
            ++s_.lost_originals;
            pending_arq_.push_back(i);
        } else if (!send_original('O', col, i, len)) {
            pending_arq_.push_back(i);  // held: ARQ redelivers it if its lag runs out first
        }
        end_slot();

        tokens_ += p_.fec_rate_q16;
        while (tokens_ >= 65536u) {
            tokens_ -= 65536u;
            send_recovery(true);
        }
        if (p_.ack_every && --ack_countdown_ == 0) {
            ack_countdown_ = p_.ack_every;
            ack_tick();
        }
        if (p_.rtx_every && --rtx_countdown_ == 0) {
            rtx_countdown_ = p_.rtx_every;
            retransmit_tick();
        }
        if (p_.arq_lag) {
            while (arq_head_ < pending_arq_.size() && i - pending_arq_[arq_head_] >= p_.arq_lag) {
                const uint32_t j = pending_arq_[arq_head_++];
                if (!have_[j]) {
                    const int ro = be_.dec_add_original(col_of_[j], j, payload_length(p_, j));
                    tr_.on_event('X', ro, col_of_[j], 0);
                    have_[j] = 1;
                    ++s_.arq_redelivered;
                    decode_loop();
                }
            }
        }
    }
};

template <class Backend, class Transcript>
Summary run_impaired(const Params& p, const Impair& m, Backend& be, Transcript& tr) {
    ImpairedRunner<Backend, Transcript> r(p, m, be, tr);
    r.finish();
    return r.summary();
}

} // namespace wl
} // namespace tamd
