// encoder.cpp -- Siamese encoder control plane.  Each function names the reference routine it
// restates (SiameseEncoder.cpp line numbers); byte work becomes symbolic terms (engine.h).
#include "encoder.h"
#include "prof.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include <time.h>

namespace tamd {

// Test hook (tamd_set_clock): a virtual millisecond clock replacing the monotonic one.
static uint64_t (*g_clock_fn)() = nullptr;
void set_clock_source(uint64_t (*fn)()) { g_clock_fn = fn; }

// GetTimeMsec (SiameseTools.cpp:105-117): wall-clock milliseconds, the time base the reference's
// 32-bit send timestamps and RTT arithmetic run on.  Read once per original.
uint64_t time_msec() {
    if (g_clock_fn) return g_clock_fn();
    timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);  // gettimeofday's clock, as the reference (vDSO, no syscall)
    return (uint64_t)ts.tv_sec * 1000u + (uint64_t)ts.tv_nsec / 1000000u;
}

Encoder::Encoder(Context* ctx, uint32_t row_bytes, HostRelease release, void* user)
    : ctx_(ctx), row_bytes_(row_bytes), release_(release), user_(user) {
    // ClearWindow (SiameseEncoder.cpp:64-83)
    for (unsigned l = 0; l < kLanes; ++l) lanes_[l].next_abs = l;
    ctx_->attach(this);
}

Encoder::~Encoder() {
    pre_flush();  // snapshots already referenced by the pending program must still be written
    drop_all();
    for (unsigned l = 0; l < kLanes; ++l) lanes_[l].sums.release(ctx_->rows);
    ctx_->detach(this);
}

void Encoder::release_segment(const Segment& s, uint32_t from, uint32_t n) {
    if (s.owned)
        for (uint32_t j = from; j < from + n; ++j) ctx_->rows.free_deferred(s.row(j));
    if (s.host && release_ && from == 0 && n == s.count) release_(s.host, user_);
}

void Encoder::drop_all() {
    if (held_)
        for (size_t i = 0; i < segs_.size(); ++i) release_segment(segs_[i], 0, segs_[i].count);
    held_ = 0;
    seg_base_ += (uint32_t)segs_.size();
    segs_.clear();
    times_.clear();
    wsize_ = 0;
    base_ = 0;
}

size_t Encoder::time_index(uint32_t e) const {
    const uint32_t a = base_ + e;
    const size_t n = times_.size();
    auto holds = [&](size_t i) {
        return (int32_t)(a - times_[i].first) >= 0 && (i + 1 == n || (int32_t)(a - times_[i + 1].first) < 0);
    };
    size_t i = time_cur_;
    if (i < n && holds(i)) return i;
    if (++i < n && holds(i)) return time_cur_ = i;
    size_t lo = 0, hi = n;  // the last run that starts at or before a
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if ((int32_t)(a - times_[mid].first) >= 0) lo = mid;
        else hi = mid;
    }
    return time_cur_ = lo;
}

void Encoder::push_time(uint32_t abs_first, uint32_t msec) {
    if (times_.empty() || times_.back().msec != msec) times_.push_back(TimeRun{abs_first, msec});
}

// The run holding e becomes up to three: the elements before e, e alone, those after it.  Equal
// neighbours merge again, so elements resent at one time stay one run.
void Encoder::set_msec(uint32_t e, uint32_t msec) {
    size_t i = time_index(e);
    if (times_[i].msec == msec) return;
    const uint32_t a = base_ + e;
    const uint32_t old = times_[i].msec;
    const uint32_t end = i + 1 < times_.size() ? times_[i + 1].first : base_ + wsize_;
    if ((int32_t)(a - times_[i].first) > 0) {  // (a first run that begins below the window included)
        times_.insert(times_.begin() + (i + 1), TimeRun{a, msec});
        ++i;
    } else if (i > 0 && times_[i - 1].msec == msec) {
        times_.erase(times_.begin() + i);  // e joins the run before it
        --i;
    } else {
        times_[i] = TimeRun{a, msec};
    }
    // run i now ends with e; what followed e in the old run keeps the old time
    if (a + 1 != end) {
        times_.insert(times_.begin() + (i + 1), TimeRun{a + 1, old});
    } else if (i + 1 < times_.size() && times_[i + 1].msec == msec) {
        times_.erase(times_.begin() + (i + 1));
    }
}

uint32_t Encoder::longest_age(uint32_t lo, uint32_t hi, uint32_t now, uint32_t longest) const {
    if (lo >= hi) return longest;
    const uint32_t end = base_ + hi;
    for (size_t i = time_index(lo); i < times_.size() && (int32_t)(times_[i].first - end) < 0; ++i) {
        const int32_t d = (int32_t)(now - times_[i].msec);
        if ((uint32_t)d > longest && d > 0) longest = (uint32_t)d;
    }
    return longest;
}

StoredOriginal Encoder::view(uint32_t e) const {
    const Segment& s = seg_of(e);
    const uint32_t j = e + base_ - s.first;
    StoredOriginal o;
    o.row = s.row(j);
    o.bytes = s.bytes;
    o.column = to_column(e);
    o.send_msec = msec_of(e);
    o.off = s.off(j);
    o.header_bytes = s.header_bytes;
    o.owned = s.owned;
    o.host = s.host;
    return o;
}

void Encoder::pre_flush() {
    emit_cauchy_group();
    emit_dense_group();
    for (unsigned l = 0; l < kLanes; ++l) lanes_[l].sums.flush(ctx_->rows, ctx_->pb, ctx_->ex);
}

void Encoder::append(const RowId* rows, uint32_t k, uint32_t framed_bytes, uint32_t header_bytes, uint8_t owned,
                     void* host, uint32_t now, uint64_t layout) {
    const RowTable& rt = ctx_->rows;
    uint32_t e_abs = base_ + wsize_;
    uint32_t col = next_column_;
    push_time(e_abs, now);
    wsize_ += k;
    // Fast path: the k packets are consecutive handles at one offset stride with no column wrap
    // inside (a stretch of a session's inputs): they continue the last segment or open one.
    if (k >= 2 && !host && col + k - 1 < kColumnPeriod && col != 0 && (layout || consecutive_handles(rows, k))) {
        const uint32_t o0 = layout ? (uint32_t)(layout >> 32) : rt.offset(rows[0]);
        const uint32_t o1 = layout ? o0 + (uint32_t)layout : rt.offset(rows[1]);
        const uint32_t stride = o1 - o0;
        if (o1 > o0 && (layout || rt.affine(rows[0], k, stride))) {
            Segment* last = segs_.empty() ? nullptr : &segs_.back();
            const bool cont = last && !last->host && last->row0 != kNoRow && last->end() == e_abs &&
                              last->bytes == framed_bytes && last->header_bytes == header_bytes &&
                              last->owned == owned && rows[0] == last->row0 + last->count && o0 > last->off0 &&
                              (last->count == 1 ? o0 - last->off0 == stride
                                                : last->stride == stride && o0 == last->off(last->count));
            if (cont) {
                last->stride = stride;
                last->count += k;
            } else {
                Segment sg;
                sg.first = e_abs;
                sg.count = k;
                sg.row0 = rows[0];
                sg.off0 = o0;
                sg.stride = stride;
                sg.bytes = framed_bytes;
                sg.column0 = col;
                sg.header_bytes = (uint8_t)header_bytes;
                sg.owned = owned;
                segs_.push_back(sg);
                if (owned) ++held_;
            }
            return;
        }
    }
    // (a run with a layout names its first handle only)
    auto row_at = [&](uint32_t x) { return layout ? rows[0] + x : rows[x]; };
    uint32_t j = 0;
    while (j < k) {
        // extend the last segment when this packet continues it, else open one
        Segment* last = segs_.empty() ? nullptr : &segs_.back();
        const RowId r = row_at(j);
        const uint32_t off = rt.offset(r);
        const bool cont = last && !host && !last->host && last->row0 != kNoRow && last->end() == e_abs &&
                          last->bytes == framed_bytes && last->header_bytes == header_bytes && last->owned == owned &&
                          r == last->row0 + last->count && off > last->off0 && col != 0 &&
                          (last->count == 1 || off == last->off(last->count));
        if (cont) {
            if (last->count == 1) last->stride = off - last->off0;
            ++last->count;
        } else {
            Segment sg;
            sg.first = e_abs;
            sg.count = 1;
            sg.row0 = r;
            sg.off0 = off;
            sg.bytes = framed_bytes;
            sg.column0 = col;
            sg.header_bytes = (uint8_t)header_bytes;
            sg.owned = owned;
            sg.host = host;
            segs_.push_back(sg);
            if (owned || host) ++held_;
            last = &segs_.back();
        }
        ++e_abs;
        col = col_inc(col);
        ++j;
        // the rest of the run while rows keep both strides (one contiguous scan of the handles'
        // offsets)
        if (last->count >= 2) {
            uint32_t n = last->count;
            while (j < k && row_at(j) == last->row0 + n && col != 0 && rt.offset(row_at(j)) == last->off(n)) {
                ++n;
                ++j;
                col = col_inc(col);
            }
            e_abs += n - last->count;
            last->count = n;
        }
    }
}

// EncoderPacketWindow::Add (SiameseEncoder.cpp:85-161)
Result Encoder::add(RowId row, uint32_t framed_bytes, uint32_t header_bytes, uint32_t payload_bytes,
                    void* host, uint32_t* packet_num, bool borrowed) {
    if (disabled_) return kDisabled;
    if (remaining_slots() <= 0) return kMaxPacketsReached;
    *packet_num = add_first(row, framed_bytes, header_bytes, payload_bytes, host, borrowed);
    return kSuccess;
}

// The window part of Add for one packet: a new window when the previous one is empty (elements
// below column % kLanes of a fresh window are placeholders: only the RTT scan reads them, and only
// their send timestamps), then the packet at the window end.
uint32_t Encoder::add_first(RowId row, uint32_t framed_bytes, uint32_t header_bytes, uint32_t payload_bytes,
                            void* host, bool borrowed) {
    const uint32_t column = next_column_;
    const uint32_t now = (uint32_t)now_msec();
    if (count_ > 0) {
        ++count_;
    } else {
        start_new_window(column);
        const uint32_t element = column % kLanes;
        if (element) {
            Segment ph;
            ph.first = base_;
            ph.count = element;
            ph.column0 = column - element;
            segs_.push_back(ph);
            for (uint32_t e = 0; e < element; ++e) push_time(base_ + e, placeholder_msec_[e]);
            wsize_ = element;
        }
    }
    append(&row, 1, framed_bytes, header_bytes, borrowed ? 0 : 1, host, now);
    next_column_ = col_inc(next_column_);
    Lane& lane = lanes_[column % kLanes];
    if (lane.longest < framed_bytes) lane.longest = framed_bytes;
    if (longest_ < framed_bytes) longest_ = framed_bytes;
    stats_[0]++;
    stats_[1] += payload_bytes;
    return column;
}

// k consecutive add() calls that all succeed.
bool Encoder::add_run(const RowId* rows, uint32_t k, uint32_t framed_bytes, uint32_t header_bytes,
                      uint32_t payload_bytes, bool borrowed, uint32_t* first_col, uint64_t layout) {
    if (disabled_ || remaining_slots() < k || !k) return false;
    // A first add that starts a window goes alone; the rest (all k when the window is open)
    // append at once (count_ > 0, element == count_).
    uint32_t skip = 0;
    if (count_ == 0) {
        *first_col = add_first(rows[0], framed_bytes, header_bytes, payload_bytes, nullptr, borrowed);
        if (k == 1) return true;
        skip = 1;
    } else {
        *first_col = next_column_;
    }
    const uint32_t m = k - skip;
    append(rows + skip, m, framed_bytes, header_bytes, borrowed ? 0 : 1, nullptr, (uint32_t)now_msec(),
           layout && skip ? layout + ((layout & 0xffffffffull) << 32) : layout);  // (rows + 1: one stride on)
    count_ += m;
    const uint32_t first = next_column_;
    next_column_ = col_add(next_column_, m);
    // every lane one of these columns fell on (all m have the same length), unless none of the
    // lanes is below it
    if (framed_bytes > lanes_longest_min_) {
        for (uint32_t j = 0; j < m && j < kLanes; ++j) {
            Lane& lane = lanes_[(first + j) % kLanes];
            if (lane.longest < framed_bytes) lane.longest = framed_bytes;
        }
        if (m >= kLanes) lanes_longest_min_ = framed_bytes;  // (each lane got one)
        if (longest_ < framed_bytes) longest_ = framed_bytes;
    }
    stats_[0] += m;
    stats_[1] += (uint64_t)payload_bytes * m;
    return true;
}

// EncoderPacketWindow::StartNewWindow (SiameseEncoder.cpp:163-181)
void Encoder::start_new_window(uint32_t column) {
    // Everything from the previous window is unreachable once Count reached zero (only the send
    // timestamps of its first elements stay visible to the RTT scan, see placeholder_msec_).
    for (uint32_t e = 0; e < kLanes && e < wsize_; ++e) placeholder_msec_[e] = msec_of(e);
    ++window_gen_;  // (a pending Cauchy group does not extend into the new window)
    drop_all();
    const uint32_t element = column % kLanes;
    column_start_ = column - element;
    sum_start_ = element;
    sum_end_ = element;
    first_unremoved_ = element;
    count_ = element + 1;
    longest_ = 0;
    for (unsigned l = 0; l < kLanes; ++l) lanes_[l].longest = 0;
    lanes_longest_min_ = 0;
}

// EncoderPacketWindow::RemoveBefore (SiameseEncoder.cpp:183-216)
void Encoder::remove_before(uint32_t first_kept_column) {
    if (disabled_) return;
    const uint32_t e = to_element(first_kept_column);
    if (e >= count_) {
        if (!col_delta_negative(e)) count_ = 0;  // removed everything
    } else if (first_unremoved_ < e) {
        first_unremoved_ = e;
    }
}

// EncoderPacketWindow::ResetSums (SiameseEncoder.cpp:218-237)
void Encoder::reset_sums(uint32_t element_start) {
    for (unsigned l = 0; l < kLanes; ++l) {
        lanes_[l].next_abs = base_ + next_lane_element(element_start, l);
        lanes_[l].sums.reset(ctx_->rows);
    }
    sum_start_ = element_start;
    sum_end_ = element_start;
    sum_column_start_ = to_column(element_start);
    sum_erased_ = 0;
    drop_segments_below(base_);  // (segments kept for the previous sums)
}

void Encoder::drop_segments_below(uint32_t drop) {
    while (!segs_.empty() && (int32_t)(segs_.front().end() - drop) <= 0) {
        const Segment& f = segs_.front();
        if (f.owned || f.host) {
            release_segment(f, 0, f.count);
            --held_;
        }
        segs_.pop_front(1);
        ++seg_base_;
    }
    if (!segs_.empty() && (int32_t)(segs_.front().first - drop) < 0) {
        Segment& f = segs_.front();
        const uint32_t d = drop - f.first;
        release_segment(f, 0, d);  // (a straddling segment holds no host copy: count > 1)
        f.first = drop;
        f.count -= d;
        if (f.row0 != kNoRow) f.row0 += d;
        f.off0 += d * f.stride;
        f.column0 = col_add(f.column0, d);
    }
}

// EncoderPacketWindow::RemoveElements (SiameseEncoder.cpp:239-357)
void Encoder::remove_elements() {
    TAMD_PROF_SCOPE(kEncRemove);
    const uint32_t first_kept_sub = first_unremoved_ / kSubwindow;
    const uint32_t removed = first_kept_sub * kSubwindow;

    // While the running sums are active, the lanes accumulate lazily (the reference advances them
    // here, GetSum up to the removed elements): the segments of the sum range are kept -- with the
    // rows they own -- until the sums reset, so a later lane read (or a direct dense read) still
    // finds every packet of the range.
    const uint32_t cut = base_ + removed;
    uint32_t drop = cut;
    if (sum_end_ > sum_start_) {
        const uint32_t keep = sum_abs_start();
        if ((int32_t)(keep - drop) < 0) drop = keep;
        if (removed > sum_start_) sum_erased_ += removed - sum_start_;
        sum_end_ = sum_end_ > removed ? sum_end_ - removed : 0;
        sum_start_ = sum_start_ > removed ? sum_start_ - removed : 0;
    }

    // segments below `drop` leave (what they own is released); one that straddles it keeps its
    // later packets
    drop_segments_below(drop);
    wsize_ -= removed;
    base_ = cut;
    size_t gone = 0;  // time runs that end at or below the window start
    while (gone + 1 < times_.size() && (int32_t)(times_[gone + 1].first - base_) <= 0) ++gone;
    if (gone) times_.erase(times_.begin(), times_.begin() + gone);
    count_ -= removed;
    column_start_ = to_column(removed);
    first_unremoved_ -= removed;

    // longest packet of the unacknowledged elements, overall and per lane (segment by segment)
    uint32_t longest = 0, lane_longest[kLanes] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (first_unremoved_ < count_) {
        const uint32_t lo = base_ + first_unremoved_, hi = base_ + count_;
        for (size_t i = seg_index_at(lo); i < segs_.size(); ++i) {
            const Segment& sg = segs_[i];
            if (sg.first >= hi) break;
            const uint32_t a = sg.first > lo ? sg.first : lo, b = sg.end() < hi ? sg.end() : hi;
            if (a >= b || !sg.bytes) continue;
            if (longest < sg.bytes) longest = sg.bytes;
            for (uint32_t x = a; x < b && x < a + kLanes; ++x) {
                const uint32_t l = (x - base_) % kLanes;
                if (lane_longest[l] < sg.bytes) lane_longest[l] = sg.bytes;
            }
        }
    }
    longest_ = longest;
    lanes_longest_min_ = ~0u;
    for (unsigned l = 0; l < kLanes; ++l) {
        lanes_[l].longest = lane_longest[l];
        if (lanes_longest_min_ > lane_longest[l]) lanes_longest_min_ = lane_longest[l];
    }

    if (sum_end_ <= sum_start_) reset_sums(first_unremoved_);
}

// EncoderPacketWindow::GetSum (SiameseEncoder.cpp:359-418), for the lane's three sums at once.
// The lane's packets in a segment are every kLanes-th of it: one strided run per segment.  The
// lane may start before the window (segments kept for the sums, remove_elements).
LaneSums& Encoder::get_lane(uint32_t lane_index, uint32_t element_end) {
    Lane& lane = lanes_[lane_index];
    LaneSums& sums = lane.sums;
    uint32_t a = lane.next_abs;
    const uint32_t end = base_ + element_end;
    if ((int32_t)(end - a) > 0) {
        if (lane.longest > 0) sums.grow(lane.longest);
        size_t si = seg_index_at(a);
        do {
            const Segment& sg = segs_[si];
            const uint32_t j = a - sg.first;
            const uint32_t stop = (int32_t)(sg.end() - end) < 0 ? sg.end() : end;
            const uint32_t n = (stop - 1 - a) / kLanes + 1;  // lane packets in [a, stop)
            if (sg.bytes) {
                sums.grow(sg.bytes);
                sums.accumulate_run_level0(sg.row(j), sg.off(j), sg.bytes, col_add(sg.column0, j), n,
                                           sg.stride * kLanes);
            }
            a += n * kLanes;
            while (si + 1 < segs_.size() && (int32_t)(segs_[si].end() - a) <= 0) ++si;
        } while ((int32_t)(end - a) > 0);
        lane.next_abs = a;
    }
    return sums;
}

// ---- acknowledgements (SiameseEncoder.cpp:514-800) ----

bool Encoder::on_ack_data(const uint8_t* data, uint32_t bytes) {
    unsigned next = 0;
    const int hb = get_pnum_header(data, (int)bytes, next);
    if (hb < 1) return false;
    data += hb;
    bytes -= (uint32_t)hb;

    if (col_delta_negative(col_sub(next, ack_.next_expected))) return true;  // out of order

    if (ack_.next_expected == next && ack_.have_data && bytes == ack_.data_bytes &&
        (bytes == 0 || memcmp(data, ack_.data.data(), bytes) == 0))
        return true;  // duplicate

    ack_.next_expected = next;
    ack_.offset = 0;
    ack_.loss_column = next;
    ack_.loss_count = 0;
    ack_.data_bytes = bytes;
    if (bytes > 0) {
        ack_.data.assign(data, data + bytes);
        ack_.data.resize((size_t)bytes + 8, 0);
        ack_.have_data = true;
        if (!decode_next_range()) return false;
    }
    update_rto();
    remove_before(ack_.next_expected);
    return true;
}

// WindowedMinMax<.., WindowedMaxCompare>::Update (SiameseTools.h:184-235)
void Encoder::rtt_update(uint32_t value, uint64_t now, uint64_t window) {
    auto* s = ack_.max_rtt;
    auto expired = [&](int i, uint64_t w) { return (uint64_t)(now - s[i].ts) > w; };
    if (s[0].value == 0 || value >= s[0].value || expired(2, window)) {
        s[0].value = s[1].value = s[2].value = value;
        s[0].ts = s[1].ts = s[2].ts = now;
        return;
    }
    if (value >= s[1].value) { s[1].value = s[2].value = value; s[1].ts = s[2].ts = now; }
    else if (value >= s[2].value) { s[2].value = value; s[2].ts = now; }
    if (expired(0, window)) {
        if (expired(1, window)) { s[0] = s[2]; s[1].value = value; s[1].ts = now; }
        else { s[0] = s[1]; s[1] = s[2]; }
        s[2].value = value;
        s[2].ts = now;
        return;
    }
    if (s[1].value == s[0].value && expired(1, window / 4)) {
        s[1].value = s[2].value = value;
        s[1].ts = s[2].ts = now;
        return;
    }
    if (s[2].value == s[1].value && expired(2, window / 2)) { s[2].value = value; s[2].ts = now; }
}

// EncoderAcknowledgementState::UpdateRTO (SiameseEncoder.cpp:584-723)
void Encoder::update_rto() {
    const uint32_t window_count = count_;
    uint32_t first_loss = to_element(ack_.next_expected);
    if (first_loss >= window_count) return;

    const uint64_t now64 = now_msec();
    const uint32_t now = (uint32_t)now64;
    uint32_t longest = 0;

    uint32_t element = to_element(ack_.next_rto_column);
    if (element >= window_count) element = first_unremoved_;

    // (the oldest send time of a range: one look per time run it overlaps)
    if (element < first_loss) {
        longest = longest_age(element, first_loss, now, longest);
        element = first_loss;
    }

    uint32_t remaining = ack_.data_bytes;
    const uint8_t* data = ack_.data.data();
    while (remaining > 0) {
        unsigned rel = 0, lossM1 = 0;
        const int n = get_nack_range(data, remaining + 8, rel, lossM1);
        if (n < 0 || n > (int)remaining) return;
        data += n;
        remaining -= (uint32_t)n;
        if (element + 1 < first_loss) element = first_loss - 1;
        first_loss += rel;
        if (element < first_loss) {
            if (first_loss > window_count) return;  // (the range leaves the window)
            longest = longest_age(element, first_loss, now, longest);
            element = first_loss;
        }
        first_loss += lossM1 + 2;
    }
    ack_.next_rto_column = to_column(element);
    if (longest <= 0) return;

    uint64_t window = (uint64_t)ack_.rto_msec * 2;
    if (window < 100) window = 100;
    else if (window > 4000) window = 4000;
    rtt_update(longest, now64, window);
    ack_.rto_msec = (ack_.max_rtt[0].value * 3) / 2;
    if (ack_.rto_msec < 20) ack_.rto_msec = 20;
}

// EncoderAcknowledgementState::DecodeNextRange (SiameseEncoder.cpp:725-755)
bool Encoder::decode_next_range() {
    if (ack_.offset >= ack_.data_bytes) return false;
    unsigned rel = 0, lossM1 = 0;
    const int n = get_nack_range(ack_.data.data() + ack_.offset, ack_.data_bytes + 8 - ack_.offset, rel, lossM1);
    if (n < 0) return false;
    ack_.offset += (uint32_t)n;
    if (ack_.offset > ack_.data_bytes) return false;
    ack_.loss_column = col_add(ack_.loss_column, rel);
    ack_.loss_count = lossM1 + 1;
    return true;
}

// GetNextLossColumn (SiameseEncoder.cpp:757-777)
bool Encoder::next_loss_column(uint32_t& column) {
    if (ack_.loss_count <= 0) {
        ack_.loss_column = col_inc(ack_.loss_column);
        if (!decode_next_range()) return false;
    }
    column = ack_.loss_column;
    ack_.loss_column = col_inc(ack_.loss_column);
    --ack_.loss_count;
    return true;
}

// RestartLossIterator (SiameseEncoder.cpp:779-788)
void Encoder::restart_loss_iterator() {
    ack_.offset = 0;
    ack_.loss_column = ack_.next_expected;
    ack_.loss_count = 0;
    decode_next_range();
}

// Encoder::Acknowledge (SiameseEncoder.cpp:814-833)
Result Encoder::acknowledge(const uint8_t* data, uint32_t bytes, uint32_t* next_expected) {
    if (disabled_) return kDisabled;
    if (!on_ack_data(data, bytes)) return kInvalidInput;
    *next_expected = ack_.next_expected;
    stats_[6]++;
    stats_[7] += bytes;
    return kSuccess;
}

Result Encoder::attempt_retransmit(uint32_t e, StoredOriginal* out) {
    const StoredOriginal o = view(e);
    if (o.header_bytes == 0 || o.bytes <= o.header_bytes) { disabled_ = true; return kDisabled; }
    *out = o;
    stats_[4]++;
    stats_[5] += o.bytes - o.header_bytes;
    return kSuccess;
}

// Encoder::Retransmit (SiameseEncoder.cpp:877-1044)
Result Encoder::retransmit(StoredOriginal* out) {
    if (disabled_) return kDisabled;
    if (unacked() == 0) {
        ack_.found_oldest = false;
        return kNeedMoreData;
    }
    const uint32_t first = col_sub(ack_.next_expected, column_start_);
    const uint32_t count = count_;
    if (col_delta_negative(first) || first < first_unremoved_ || first >= count) return kNeedMoreData;

    const uint32_t now = (uint32_t)now_msec();
    const uint32_t rto = ack_.rto_msec;

    if (ack_.found_oldest) {
        const uint32_t e = col_sub(ack_.oldest_column, column_start_);
        if (!col_delta_negative(e) && e >= first && e < count) {
            if ((uint32_t)(now - msec_of(e)) < rto) return kNeedMoreData;
            set_msec(e, now);
            ack_.found_oldest = false;
            return attempt_retransmit(e, out);
        }
        ack_.found_oldest = false;
    }

    uint32_t nack_element = first;
    uint32_t oldest = nack_element;
    uint32_t oldest_msec = msec_of(oldest);
    if ((uint32_t)(now - oldest_msec) >= rto) {
        set_msec(oldest, now);
        return attempt_retransmit(oldest, out);
    }

    if (ack_.data_bytes > 0) {
        restart_loss_iterator();
        uint32_t column = 0;
        while (next_loss_column(column)) {
            nack_element = to_element(column);
            if (nack_element >= count) break;
            const uint32_t last = msec_of(nack_element);
            if ((uint32_t)(now - last) >= rto) {
                set_msec(nack_element, now);
                return attempt_retransmit(nack_element, out);
            }
            if ((int32_t)(oldest_msec - last) > 0) { oldest = nack_element; oldest_msec = last; }
        }
    }

    for (uint32_t e = nack_element + 1; e < count; ++e) {
        const uint32_t last = msec_of(e);
        if ((uint32_t)(now - last) >= rto) {
            set_msec(e, now);
            return attempt_retransmit(e, out);
        }
        if ((int32_t)(oldest_msec - last) > 0) { oldest = e; oldest_msec = last; }
    }
    ack_.found_oldest = true;
    ack_.oldest_column = to_column(oldest);
    return kNeedMoreData;
}

// Encoder::Get (SiameseEncoder.cpp:1256-1294)
Result Encoder::get(uint32_t packet_num, StoredOriginal* out) {
    if (disabled_) return kDisabled;
    const uint32_t e = to_element(packet_num);
    if (e >= count_) return kNeedMoreData;
    const StoredOriginal o = view(e);
    if (o.bytes == 0) return kNeedMoreData;
    if (o.header_bytes == 0 || o.bytes <= o.header_bytes) { disabled_ = true; return kDisabled; }
    *out = o;
    return kSuccess;
}

// ---- recovery generation ----

// `terms` is consumed.  Parity and Cauchy rows name each original once (`distinct`); Siamese
// rows can repeat a row (LDPC pairs) and are merged first.
Result Encoder::emit(Sym& terms, uint32_t len, const RecoveryMeta& meta, RecoveryOut& out, bool distinct) {
    TAMD_PROF_SCOPE(kEncEmit);
    if (!distinct) sym_merge(terms);
    out.meta = meta;
    out.footer_len = put_recovery_footer(meta, out.footer);
    out.data_len = len;
    out.row = ctx_->alloc(len + out.footer_len);
    if (out.row == kNoRow) { disabled_ = true; return kDisabled; }
    ctx_->pb.combine(out.row, terms.data(), terms.size(), len, out.footer, out.footer_len);
    stats_[2]++;
    stats_[3] += out.total();
    return kSuccess;
}

// Encoder::GenerateSinglePacket (SiameseEncoder.cpp:1296-1329)
Result Encoder::generate_single(RecoveryOut& out) {
    const StoredOriginal o = view(first_unremoved_);
    RecoveryMeta m;
    m.SumCount = 1;
    m.LDPCCount = 1;
    m.ColumnStart = o.column;
    m.Row = 0;
    Sym& t = scratch_;
    t.clear();
    t.push_back(Term{o.row, o.bytes, 1});
    return emit(t, o.bytes, m, out, true);
}

// Encoder::GenerateCauchyPacket (SiameseEncoder.cpp:1334-1441)
Result Encoder::generate_cauchy(RecoveryOut& out) {
    TAMD_PROF_SCOPE(kEncCauchy);
    const uint32_t first = first_unremoved_;
    RecoveryMeta m;
    m.SumCount = unacked();
    m.LDPCCount = m.SumCount;
    m.ColumnStart = to_column(first);
    uint32_t mode, crow = 0;
    const uint32_t next_parity = to_element(next_parity_column_);
    if (next_parity <= first || col_delta_negative(next_parity)) {
        next_parity_column_ = col_add(m.ColumnStart, m.SumCount);
        m.Row = 0;
        mode = TAMD_R_CONST;  // parity row: every coefficient 1
    } else {
        crow = next_cauchy_row_;
        m.Row = crow + 1;
        if (++next_cauchy_row_ >= kCauchyMaxRows) next_cauchy_row_ = 0;
        mode = TAMD_R_CAUCHY;  // CauchyElement(crow, column mod 64)
    }

    // The window's originals (level-0 rows): one ACCR per segment (a run of equally long packets
    // at a fixed row stride), clipped to the unacknowledged range.
    std::vector<Run>& runs = runs_;
    runs.clear();
    uint32_t used = 0;
    {
        const uint32_t lo = base_ + first, hi = base_ + count_;
        for (size_t i = seg_index_at(lo); i < segs_.size(); ++i) {
            const Segment& sg = segs_[i];
            if (sg.first >= hi) break;
            const uint32_t a = sg.first > lo ? sg.first : lo, b = sg.end() < hi ? sg.end() : hi;
            if (a >= b || !sg.bytes) continue;
            const uint32_t j = a - sg.first;
            if (used < sg.bytes) used = sg.bytes;
            runs.push_back(Run{sg.row(j), sg.off(j), sg.stride, b - a, sg.bytes, col_add(sg.column0, j)});
        }
    }

    out.meta = m;
    out.footer_len = put_recovery_footer(m, out.footer);
    out.data_len = used;
    out.row = ctx_->alloc(used + out.footer_len);
    if (out.row == kNoRow) { disabled_ = true; return kDisabled; }
    // The row's op is emitted with the group (at the latest by pre_flush, so within this
    // program); its readers must already see the level it will be written at.
    ctx_->rows.set_level(out.row, 1);
    const uint32_t max_group = 3;  // (grp_)
    // (at most 2047: the run indices of a TARGETS word are 11-bit)
    const uint32_t span = kGroupSpan;
    const uint32_t end_col = to_column(count_);
    // A row over a long window stays a pure combine of its own (the executor shares those across
    // a workgroup); a group is one wave's chain, and a long one would set the launch's tail.
    // (and rows over windows of short runs -- the C ABI's one-packet segments -- stay alone too:
    // a MULTI run per packet is an unbatched load each, a lone row's single packets are batched)
    const bool alone = count_ - first >= span || runs.size() * 4 > count_ - first;
    if (grp_n_ && (alone || grp_n_ >= max_group || grp_gen_ != window_gen_ ||
                   col_sub(end_col, grp_[0].first_col) >= span))
        emit_cauchy_group();
    grp_gen_ = window_gen_;
    CauchyTarget& t = grp_[grp_n_++];
    t.row = out.row;
    t.used = used;
    t.first_col = m.ColumnStart;
    t.end_col = end_col;
    t.kind = mode;
    t.param = mode == TAMD_R_CONST ? 1 : crow;
    t.flen = out.footer_len;
    memcpy(t.footer, out.footer, sizeof(t.footer));
    t.runs.swap(runs);
    if (alone) emit_cauchy_group();
    stats_[2]++;
    stats_[3] += out.total();
    return kSuccess;
}

void Encoder::emit_cauchy_group() {
    const uint32_t n = grp_n_;
    if (!n) return;
    grp_n_ = 0;
    ProgramBuilder& pb = ctx_->pb;
    pb.begin_op();
    if (n == 1) {  // a lone row: a pure combine (the executor may share it across a workgroup)
        const CauchyTarget& t = grp_[0];
        for (const Run& r : t.runs) {
            if (r.count == 1) {
                const uint8_t c = t.kind == TAMD_R_CONST ? 1 : cauchy_element(t.param, r.col % kCauchyMaxColumns);
                pb.op_acc(r.row, c, r.len);
            } else {
                pb.op_accr(t.kind, t.param, r.off, r.stride, r.count, r.len, r.col, 1);
            }
        }
        pb.finish_combine(t.row, t.used, t.footer, t.flen);
        return;
    }
    // The union of the windows in runs: row a's runs below the next row's first column.
    const uint32_t base = grp_[0].first_col;
    std::vector<Run>& u = grp_union_;
    u.clear();
    for (uint32_t a = 0; a < n; ++a) {
        const uint32_t stop = a + 1 < n ? col_sub(grp_[a + 1].first_col, base) : ~0u;
        for (const Run& r : grp_[a].runs) {
            const uint32_t at = col_sub(r.col, base);
            if (at >= stop) continue;
            Run c = r;
            if (at + c.count > stop) c.count = stop - at;
            u.push_back(c);
        }
    }
    for (const Run& r : u) {
        const uint32_t at = col_sub(r.col, base);
        uint32_t tw[3] = {0, 0, 0};
        for (uint32_t a = 0; a < n; ++a) {
            const uint32_t f = col_sub(grp_[a].first_col, base), e = col_sub(grp_[a].end_col, base);
            const uint32_t lo = f > at ? f - at : 0u;
            const uint32_t hi = e - at < r.count ? e - at : r.count;  // (e > at: within the union)
            if (e > at && lo < hi) tw[a] = grp_[a].kind | grp_[a].param << 2 | lo << 10 | hi << 21;
        }
        if (tw[0] | tw[1] | tw[2]) pb.op_accr_multi(r.off, r.stride, r.count, r.len, r.col, 1, tw);
    }
    for (uint32_t a = 0; a < n; ++a) pb.op_store(grp_[a].row, grp_[a].used, a, grp_[a].footer, grp_[a].flen);
    pb.end_op(1);
}

// Encoder::AddDenseColumns (SiameseEncoder.cpp:1046-1098)
// The product half (opcode bits 3..5) is folded in with its RX factor right here: both halves
// are clipped to the same length, so rec + RX * prod reads each lane once.
void Encoder::add_dense(uint32_t row, uint32_t recovery_bytes, Sym& rec) {
    const uint8_t rx = row_value(row);
    for (unsigned l = 0; l < kLanes; ++l) {
        const unsigned op = row_opcode(l, row);
        if (!op) continue;
        LaneSums& c = get_lane(l, count_);
        const uint32_t n = c.bytes < recovery_bytes ? c.bytes : recovery_bytes;
        if (!n) continue;
        uint8_t k[3];
        opcode_coefs(op, rx, k);
        c.read(ctx_->rows, ctx_->ex, rec, k, n, nullptr, ctx_->short_scans);
    }
    sum_end_ = count_;
}

// AddDenseColumns straight from the packets: the lane sums a Siamese row reads are sums over the
// packets of its sum range, so the row's dense part is one DENSE run per segment of that range
// (program.h), each packet weighted by its lane's opcode combination -- no lane walk, snapshot
// or carried sum.  Bytes are the same: a lane sum is its packets zero-padded to the longest, and
// each packet is clipped to the recovery length as the sum would be.  The row's LDPC pair
// columns (draw_dense_pairs) are folded into the runs' coefficients (ADJ words); a pair column no run
// covers is read as a row of its own.
//
// Rows are queued (dgrp_) and emitted by emit_dense_group: rows of one sum range share its
// packets, so up to three of them are one op per chunk, each packet loaded once for all.
bool Encoder::defer_dense(uint32_t row, uint32_t recovery_bytes, const RecoveryOut& out) {
    const uint32_t max_group = 3;  // (dgrp_)
    // A group's op is one work item per slice (one wave, or one workgroup in small launches), so
    // its products per item are bounded as a lone row's are: packets per chunk x targets
    const uint32_t max_work = kDenseGroupWork;
    const uint32_t lo = sum_abs_start(), hi = base_ + count_;
    const uint32_t split = ctx_->dense_split;
    const uint32_t rows = split && hi - lo > split ? split : hi - lo;
    if (dgrp_n_ && (lo != dgrp_lo_ || recovery_bytes != dgrp_len_ || window_gen_ != dgrp_gen_ ||
                    rows * (dgrp_n_ + 1) > max_work))
        emit_dense_group();
    // The range's runs (a superset of the queued rows' ranges: they share `lo` and end earlier)
    std::vector<DenseRun>& runs = dgrp_runs_;
    runs.clear();
    for (size_t i = seg_index_at(lo); i < segs_.size(); ++i) {
        const Segment& sg = segs_[i];
        if ((int32_t)(sg.first - hi) >= 0) break;
        const uint32_t a = (int32_t)(sg.first - lo) > 0 ? sg.first : lo;
        const uint32_t b = (int32_t)(sg.end() - hi) < 0 ? sg.end() : hi;
        if ((int32_t)(b - a) <= 0 || !sg.bytes) continue;
        const uint32_t j = a - sg.first;
        runs.push_back(DenseRun{sg.off(j), sg.stride, b - a, sg.bytes < recovery_bytes ? sg.bytes : recovery_bytes,
                                col_add(sg.column0, j), a - lo});
    }
    if (!dgrp_n_) {
        dgrp_lo_ = lo;
        dgrp_len_ = recovery_bytes;
        dgrp_gen_ = window_gen_;
    }
    DenseTarget& t = dgrp_[dgrp_n_];
    t.row = out.row;
    t.ops = g_gf.row_ops[row];
    t.rx = row_value(row);
    t.hi = hi - lo;
    t.flen = out.footer_len;
    memcpy(t.footer, out.footer, sizeof(t.footer));
    // The LDPC pair columns (AddLightColumns over the unacknowledged window): those on a run's
    // packet stay entries of the row (ADJ words), the others -- placeholders, elements outside
    // the range -- are resolved to their rows now (the window may have moved on by emission)
    {
        TAMD_PROF_SCOPE(kEncLight);
        const uint32_t start = base_ + first_unremoved_;
        draw_dense_pairs(row, sum_end_ - first_unremoved_, t.rx, start - lo, lo, runs.data(), runs.size(), t.pairs,
                         pairs_);
        sort_pair_keys(pairs_);
        t.loose.clear();
        for (uint64_t pr : pairs_) {
            const uint32_t e = (uint32_t)(pr >> 8);
            const Segment& sg = seg_of(e - base_);
            t.loose.push_back(Term{sg.row(e - sg.first), sg.bytes, (uint8_t)(pr & 0xffu)});
        }
    }
    // partial sums: one per chunk of the range (none when it fits one)
    const uint32_t chunks = split && t.hi > split ? (t.hi + split - 1) / split : 1u;
    t.parts.clear();
    for (uint32_t c = 1; chunks > 1 && c <= chunks; ++c) {
        const RowId pr = ctx_->alloc_temp(recovery_bytes);
        if (pr == kNoRow) return false;
        t.parts.push_back(pr);
    }
    // the readers of the row see the level it will be written at (emission is within this program)
    ctx_->rows.set_level(out.row, chunks > 1 ? 2 : 1);
    if (++dgrp_n_ >= max_group) emit_dense_group();
    return true;
}

void Encoder::emit_dense_group() {
    const uint32_t n = dgrp_n_;
    if (!n) return;
    dgrp_n_ = 0;
    ProgramBuilder::DenseTarget tg[3];
    for (uint32_t a = 0; a < n; ++a) {
        const DenseTarget& d = dgrp_[a];
        tg[a] = ProgramBuilder::DenseTarget{d.ops, d.rx, d.hi, d.pairs.data(), (uint32_t)d.pairs.size(), d.row,
                                            d.parts.empty() ? nullptr : d.parts.data(), (uint32_t)d.parts.size(),
                                            d.loose.data(), (uint32_t)d.loose.size(), d.footer, d.flen};
    }
    ctx_->pb.emit_dense_range(dgrp_runs_.data(), dgrp_runs_.size(), tg, n, ctx_->dense_split, dgrp_len_, false);
}

// Encoder::AddLightColumns (SiameseEncoder.cpp:1100-1144).  The product half goes straight into
// the row with its RX factor (the reference multiplies the product buffer by RX and adds it,
// :1236-1240; both are clipped to the same length, and every window packet is at most
// longest_ bytes, so no clipping is needed).
void Encoder::add_light(uint32_t row, Sym& rec) {
    const uint32_t start = first_unremoved_;
    const uint32_t count = sum_end_ - start;
    const uint8_t rx = row_value(row);
    Pcg32 prng;
    prng.seed(row, count);
    const uint32_t pairs = (count + kPairRate - 1) / kPairRate;
    const size_t at = rec.size();
    rec.resize(at + 2 * (size_t)pairs);
    Term* t = rec.data() + at;
    const FastMod mod(count);
    for (uint32_t i = 0; i < pairs; ++i) {
        const uint32_t e1 = start + mod(prng.next());
        const uint32_t erx = start + mod(prng.next());
        const Segment& s1 = seg_of(e1);
        const Segment& srx = seg_of(erx);
        t[2 * i] = Term{s1.row(e1 + base_ - s1.first), s1.bytes, 1};
        t[2 * i + 1] = Term{srx.row(erx + base_ - srx.first), srx.bytes, rx};
    }
}

// Short sum ranges (the usual case with acknowledgements: each Siamese row follows a sum reset)
// are read straight from the packets; long ones through the running lane sums.
bool Encoder::direct_sums() const {
    const uint32_t range = count_ + sum_erased_ - sum_start_;
    // Direct reads pay per run (a DENSE run's coefficient setup and first row loads); packets
    // added one by one with host copies (the C ABI) are runs of one, where the lane sums' batched
    // single-row reads are far cheaper: direct only while the range's runs average kDirectMinRun.
    bool direct = range <= kDirectMax;
    if (direct && range) direct = (segs_.size() - seg_index_at(sum_abs_start())) * kDirectMinRun <= range;
    return direct;
}

// encode()'s branches without running them: the single packet and Cauchy / parity rows change
// only row counters (and the sum end); a Siamese row also its sum end, unless its lane reads would
// accumulate packets or snapshot a pending scan.
bool Encoder::encode_is_quiet() const {
    if (disabled_ || count_ <= 0 || first_unremoved_ >= kRemoveThreshold) return false;
    const uint32_t un = unacked();
    if (un == 1) return true;
    const uint32_t ub = count_ - sum_start_ + sum_erased_;
    if (sum_end_ <= sum_start_ || ub >= kMaxPackets) return un <= kCauchyThreshold;  // (else a sum reset)
    if (un <= kSumResetThreshold || ub <= kCauchyThreshold) return true;
    if (direct_sums()) return true;
    for (unsigned l = 0; l < kLanes; ++l)
        if ((int32_t)(base_ + count_ - lanes_[l].next_abs) > 0 || !lanes_[l].sums.idle()) return false;
    return true;
}

// Encoder::Encode (SiameseEncoder.cpp:1146-1254)
Result Encoder::encode(RecoveryOut& out) {
    out = RecoveryOut();
    if (disabled_) return kDisabled;
    if (count_ <= 0) return kNeedMoreData;
    if (first_unremoved_ >= kRemoveThreshold) remove_elements();

    const uint32_t un = unacked();
    if (un == 1) return generate_single(out);

    const uint32_t ub = count_ - sum_start_ + sum_erased_;
    if (sum_end_ <= sum_start_ || ub >= kMaxPackets) {
        if (un <= kCauchyThreshold) return generate_cauchy(out);
        reset_sums(first_unremoved_);
    } else if (un <= kSumResetThreshold || ub <= kCauchyThreshold) {
        sum_end_ = sum_start_;
        return generate_cauchy(out);
    }

    const uint32_t row = next_row_;
    if (++next_row_ >= kRowPeriod) next_row_ = 0;

    const uint32_t recovery_bytes = longest_;
    Sym& rec = rec_;
    rec.clear();
    const bool direct = direct_sums();
    if (!direct) {
        TAMD_PROF_SCOPE(kEncDense);
        add_dense(row, recovery_bytes, rec);
    } else {
        sum_end_ = count_;
    }
    if (!direct) {  // (a direct row's pairs are drawn by defer_dense, into its runs' coefficients)
        TAMD_PROF_SCOPE(kEncLight);
        add_light(row, rec);
    }

    RecoveryMeta m;
    m.SumCount = sum_end_ - sum_start_ + sum_erased_;
    m.LDPCCount = un;
    m.ColumnStart = sum_column_start_;
    m.Row = row;
    if (direct) {
        // one op: the dense runs, the LDPC pairs, the store
        out.meta = m;
        out.footer_len = put_recovery_footer(m, out.footer);
        out.data_len = recovery_bytes;
        out.row = ctx_->alloc(recovery_bytes + out.footer_len);
        if (out.row == kNoRow) { disabled_ = true; return kDisabled; }
        if (!defer_dense(row, recovery_bytes, out)) {  // no arena room for its partial sums
            disabled_ = true;
            ctx_->rows.free_deferred(out.row);
            out = RecoveryOut();
            return kDisabled;
        }
        stats_[2]++;
        stats_[3] += out.total();
        return kSuccess;
    }
    // Every term is within recovery_bytes already (lane reads clip to it, packets are at most
    // longest_).  Terms are not merged: the lane snapshots are distinct rows, and a packet the
    // LDPC pairs name twice just becomes two reads (GF(2^8) sums are linear), which costs the
    // device less than a merge costs the host.
    return emit(rec, recovery_bytes, m, out, true);
}

// Encoder::GetStatistics (SiameseEncoder.cpp:1445-1457)
void Encoder::stats(uint64_t* out, unsigned n) {
    if (n > 9) n = 9;
    stats_[8] = ctx_->rows.bytes_in_use();
    for (unsigned i = 0; i < n; ++i) out[i] = stats_[i];
}

} // namespace tamd
