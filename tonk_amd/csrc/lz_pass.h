// lz_pass.h -- how a call's messages of many streams are split into passes over the streams'
// history rings (tonk_compress_batch.h, cbatch.cpp; host only, also compiled into
// tests/native/cbatch_check.cpp).
//
// A pass is a placement launch followed by a compression launch: all of a pass's messages are in
// their rings before any of them is compressed, each as a job of its own over its stream's ring
// (lz.h RingTrack gives its linear position and the start of its window).  A message at linear
// positions [pos, pos + n) lands on the ring bytes of positions TAMD_LZ_RING lower, so a stream's
// later message of the same pass must not reach TAMD_LZ_RING bytes past the window start of an
// earlier one: within a pass, a stream's placed bytes and the oldest window before them stay
// within the ring.  A message that would break this opens the stream's next pass.  Passes are
// counted per stream from the call's first: a stream with one message is in pass 0 whatever the
// others need, its items are never out of order, and the call launches as many passes as its
// busiest stream needs.
//
// `per_pass` caps a stream's messages in one pass below what the ring allows.  At 1 the bytes
// behind a message's end are, while it is compressed, what the stream's ring held before -- as
// in the per-message interface, whose kernel lets up to four of them into the hash keys of the
// message's last positions (lz.hip: "bytes past the message end may enter a key").  With more
// than one they are the head of the stream's next message.
#pragma once
#include "lz.h"

#include <vector>

namespace tamd {

struct LzPlaced {
    uint64_t pos, win;  // RingTrack::place
    uint32_t pass;
};

struct LzPassPlan {
    struct Open {            // a stream's pass that is still taking messages
        uint64_t call = 0;   // the call it belongs to (an older one: the stream has no item yet)
        uint64_t lo_win = 0; // the oldest window start of its messages
        uint32_t pass = 0, count = 0;
    };
    std::vector<Open> open;  // by stream
    uint64_t call = 0;

    // Places item i (bytes[i] bytes, the next message of stream[i] < open.size()) on
    // tracks[stream[i]] for i = 0 .. n-1 and gives each its pass; per_pass 0: no cap but the
    // ring's.  Returns the number of passes.
    uint32_t plan(uint32_t n, const uint32_t* stream, const uint32_t* bytes, RingTrack* tracks, uint32_t per_pass,
                  LzPlaced* out) {
        ++call;
        uint32_t passes = 0;
        for (uint32_t i = 0; i < n; ++i) {
            Open& o = open[stream[i]];
            LzPlaced p{0, 0, 0};
            tracks[stream[i]].place(bytes[i], &p.pos, &p.win);
            if (o.call != call) {
                o = Open();
                o.call = call;
                o.lo_win = p.win;
            } else {
                const uint64_t lo = p.win < o.lo_win ? p.win : o.lo_win;
                if ((per_pass && o.count >= per_pass) || p.pos + bytes[i] - lo > TAMD_LZ_RING) {
                    ++o.pass;
                    o.count = 0;
                    o.lo_win = p.win;
                } else {
                    o.lo_win = lo;
                }
            }
            ++o.count;
            p.pass = o.pass;
            out[i] = p;
            if (o.pass + 1 > passes) passes = o.pass + 1;
        }
        return passes;
    }
};

}  // namespace tamd
