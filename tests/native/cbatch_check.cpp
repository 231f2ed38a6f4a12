// cbatch_check -- the host-side logic of the stateful batched compressor (tonk_compress_batch.h) as
// a stand-alone program: the placement kernel's byte logic (tonk_amd/csrc/lz_place.h) run by one
// lane and by the kernel's sixteen one after the other, and the pass planner
// (tonk_amd/csrc/lz_pass.h).  Test-only; built plain and under the address and undefined-behaviour
// sanitizers (cbatch.mk) and run by tests/test_cbatch.py.
//
//   cbatch_check place   three abutting messages of one stream (37 bytes, the message, 21 bytes),
//                        each from a source of its own that ends with the granule of its last
//                        byte, placed by different groups in either order: 16 source
//                        misalignments x 16 ring slot phases x lengths 1, 2, 15, 16, 17, 31, 33,
//                        1299, 1300, 24000 x slots inside the ring, across its end and inside its
//                        first 64 bytes; ring and mirror against a memcpy model between guards
//   cbatch_check plan    seeded random calls, 1..40 streams, 0..200 items per stream, maxima
//                        1300, 4000 and 24000, with and without the cap of one message per stream
//                        and pass: positions against RingTracks stepped one by one, order, and a
//                        replay of the passes on rings of linear positions (no placed byte lies on
//                        a window byte of the same pass)
// Prints "ok <cases>" or the first failure.
#include "../../tonk_amd/csrc/lz_pass.h"
#include "../../tonk_amd/csrc/lz_place.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

const uint32_t kGuard = 64, kLanes = 16, kMask = TAMD_LZ_RING - 1u;
const size_t kRingBytes = TAMD_LZ_RING + TAMD_LZ_MIRROR;

int fail(const char* what, long a = 0, long b = 0, long c = 0, long d = 0) {
    printf("FAIL %s (%ld, %ld, %ld, %ld)\n", what, a, b, c, d);
    return 1;
}

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)(s >> 32);
    }
    uint32_t below(uint32_t n) { return next() % n; }  // 0 .. n-1
};

// A message in a source of its own, `mis` bytes into a 16-byte aligned allocation that ends with
// the aligned granule of the message's last byte: a read past that granule is the sanitizer's.
struct Source {
    uint8_t* base;
    uint8_t* msg;
    uint32_t len;
    Source(uint32_t mis, uint32_t n, Rng& r) : len(n) {
        base = (uint8_t*)aligned_alloc(16, (mis + n + 15u) & ~(size_t)15);
        memset(base, 0xEE, (mis + n + 15u) & ~(size_t)15);
        msg = base + mis;
        for (uint32_t i = 0; i < n; ++i) msg[i] = (uint8_t)(r.next() | 1u);  // (never 0: the scrub's fill)
    }
    ~Source() { free(base); }
};

void model_place(uint8_t* ring, uint32_t slot, const uint8_t* src, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t p = (slot + i) & kMask;
        memcpy(ring + p, src + i, 1);
        if (p < TAMD_LZ_MIRROR) memcpy(ring + TAMD_LZ_RING + p, src + i, 1);
    }
}

void lanes_place(uint8_t* ring, uint32_t slot, const Source& s, uint32_t nl) {
    for (uint32_t lane = 0; lane < nl; ++lane) tamd_lz_place(ring, slot, s.msg, s.len, lane, nl);
}

int check_place() {
    const uint32_t lengths[10] = {1, 2, 15, 16, 17, 31, 33, 1299, 1300, 24000};
    const uint32_t kPrev = 37, kNext = 21;
    uint8_t* got_all = (uint8_t*)aligned_alloc(64, kRingBytes + 2 * kGuard);
    uint8_t* want_all = (uint8_t*)aligned_alloc(64, kRingBytes + 2 * kGuard);
    memset(got_all, 0xA5, kRingBytes + 2 * kGuard);
    memset(want_all, 0xA5, kRingBytes + 2 * kGuard);
    uint8_t *got = got_all + kGuard, *want = want_all + kGuard;
    memset(got, 0, kRingBytes);
    memset(want, 0, kRingBytes);
    Rng r(7);
    const std::vector<uint8_t> zeros(24000, 0);
    long cases = 0;
    int rc = 0;
    for (uint32_t li = 0; li < 10 && !rc; ++li) {
        const uint32_t len = lengths[li];
        // slot bases (the phase is added): inside the ring; the message ends at the ring's end;
        // it wraps after one byte, in its middle, before its last byte; inside the mirrored first
        // 64 bytes at each of their granules
        const uint32_t bases[9] = {4096u, TAMD_LZ_RING - len - 16u, TAMD_LZ_RING - 16u, TAMD_LZ_RING - len / 2u - 16u,
                                   TAMD_LZ_RING - (len > 1u ? len - 1u : 1u) - 8u, 0u, 16u, 32u, 48u};
        for (uint32_t bi = 0; bi < 9 && !rc; ++bi)
            for (uint32_t phase = 0; phase < 16 && !rc; ++phase)
                for (uint32_t mis = 0; mis < 16 && !rc; ++mis) {
                    const uint32_t slot = (bases[bi] + phase) & kMask;
                    Source prev((mis + 5u) & 15u, kPrev, r), msg(mis, len, r), next((mis + 11u) & 15u, kNext, r);
                    const uint32_t s_prev = (slot - kPrev) & kMask, s_next = (slot + len) & kMask;
                    // lanes 1 / 16, forwards / backwards: all four for every case; the three messages'
                    // bytes are zeroed in between
                    const Source* o[3] = {&prev, &msg, &next};
                    const uint32_t at[3] = {s_prev, slot, s_next};
                    for (uint32_t v = 0; v < 4; ++v) {
                        const uint32_t nl = v & 1u ? kLanes : 1u;
                        for (uint32_t k = 0; k < 3; ++k) {
                            model_place(got, at[k], zeros.data(), o[k]->len);
                            model_place(want, at[k], o[k]->msg, o[k]->len);
                        }
                        for (uint32_t k = 0; k < 3; ++k) lanes_place(got, at[v & 2u ? 2 - k : k], *o[v & 2u ? 2 - k : k], nl);
                        if (memcmp(got_all, want_all, kRingBytes + 2 * kGuard) != 0) break;
                    }
                    if (memcmp(got_all, want_all, kRingBytes + 2 * kGuard) != 0) {
                        size_t at = 0;
                        while (got_all[at] == want_all[at]) ++at;
                        rc = fail("ring differs from the model: length, slot, source offset, first byte", (long)len, (long)slot, (long)mis,
                                  (long)at - (long)kGuard);
                    }
                    ++cases;
                }
    }
    free(got_all);
    free(want_all);
    if (!rc) printf("ok %ld\n", cases);
    return rc;
}

// ---- the pass planner ----

int check_plan() {
    const uint32_t maxima[3] = {1300, 4000, 24000};
    long cases = 0;
    for (uint32_t mi = 0; mi < 3; ++mi)
        for (uint32_t per_pass = 0; per_pass < 2; ++per_pass)
            for (uint32_t round = 0; round < 8; ++round) {
                const uint32_t maxb = maxima[mi];
                Rng r(1000u * mi + 100u * per_pass + round + 1u);
                const uint32_t ns = 1u + r.below(40);
                tamd::LzPassPlan plan;
                plan.open.resize(ns);
                std::vector<RingTrack> tracks(ns), ref(ns);
                for (uint32_t s = 0; s < ns; ++s) tracks[s].max = ref[s].max = maxb;
                // what each stream's ring holds: the linear position + 1 of the byte in every slot
                std::vector<std::vector<uint64_t>> held(ns, std::vector<uint64_t>(TAMD_LZ_RING, 0));
                for (uint32_t call = 0; call < 3; ++call) {
                    // items: every stream's count, then a random interleaving that keeps each stream's order
                    std::vector<uint32_t> left(ns), stream, bytes;
                    uint32_t total = 0;
                    for (uint32_t s = 0; s < ns; ++s) {
                        const uint32_t kind = r.below(4);
                        left[s] = kind == 0 ? 0u : kind == 1 ? 1u : r.below(201u);
                        total += left[s];
                    }
                    std::vector<uint32_t> live;
                    for (uint32_t s = 0; s < ns; ++s)
                        if (left[s]) live.push_back(s);
                    while (!live.empty()) {
                        const uint32_t k = r.below((uint32_t)live.size()), s = live[k];
                        stream.push_back(s);
                        const uint32_t kind = r.below(8);
                        bytes.push_back(kind == 0 ? maxb : kind == 1 ? 1u + r.below(16) : 1u + r.below(maxb));
                        if (--left[s] == 0) {
                            live[k] = live.back();
                            live.pop_back();
                        }
                    }
                    const uint32_t n = (uint32_t)stream.size();
                    if (n != total) return fail("item count");
                    std::vector<tamd::LzPlaced> out(n ? n : 1);
                    const uint32_t passes = plan.plan(n, stream.data(), bytes.data(), tracks.data(), per_pass, out.data());
                    // positions: RingTracks fed the same lengths one by one; order; pass numbers
                    std::vector<int64_t> last_pass(ns, -1);
                    std::vector<uint32_t> in_pass(ns, 0);
                    uint32_t most = 0;
                    for (uint32_t i = 0; i < n; ++i) {
                        const uint32_t s = stream[i];
                        uint64_t pos = 0, win = 0;
                        ref[s].place(bytes[i], &pos, &win);
                        if (out[i].pos != pos || out[i].win != win) return fail("position differs from RingTrack's", (long)i, (long)s);
                        if (out[i].pass >= passes) return fail("pass out of range", (long)i);
                        if (last_pass[s] < 0 && out[i].pass != 0) return fail("a stream's first item is held back", (long)i, (long)s);
                        if ((int64_t)out[i].pass < last_pass[s] || (int64_t)out[i].pass > last_pass[s] + 1)
                            return fail("a stream's passes are out of order or skip one", (long)i, (long)s);
                        in_pass[s] = (int64_t)out[i].pass == last_pass[s] ? in_pass[s] + 1u : 1u;
                        if (per_pass && in_pass[s] > per_pass) return fail("more messages of a stream in a pass than the cap", (long)i, (long)s);
                        last_pass[s] = out[i].pass;
                        if (out[i].pass + 1u > most) most = out[i].pass + 1u;
                    }
                    if (most != passes) return fail("pass count", (long)passes, (long)most);
                    // the replay: a pass places all its messages, then every one of them must find
                    // its window and itself in the ring (sampled: both ends and every 251st byte)
                    for (uint32_t p = 0; p < passes; ++p) {
                        for (uint32_t i = 0; i < n; ++i)
                            if (out[i].pass == p)
                                for (uint32_t k = 0; k < bytes[i]; ++k) held[stream[i]][(out[i].pos + k) & kMask] = out[i].pos + k + 1;
                        for (uint32_t i = 0; i < n; ++i) {
                            if (out[i].pass != p) continue;
                            const uint64_t lo = out[i].win, hi = out[i].pos + bytes[i];
                            if (hi - lo > TAMD_LZ_RING) return fail("window and message exceed the ring", (long)i);
                            for (uint64_t q = lo; q < hi; q = (q + 251 < hi || q == hi - 1) ? q + 251 : hi - 1)
                                if (held[stream[i]][q & kMask] != q + 1)
                                    return fail("a window byte was overwritten in its pass: item, stream, pass", (long)i, (long)stream[i], (long)p);
                        }
                    }
                    // greedy: a message opens a pass only when it could not join the open one
                    if (!per_pass) {
                        std::vector<uint64_t> lo_win(ns, 0);
                        std::vector<int64_t> cur(ns, -1);
                        for (uint32_t i = 0; i < n; ++i) {
                            const uint32_t s = stream[i];
                            if (cur[s] == (int64_t)out[i].pass) {
                                if (out[i].win < lo_win[s]) lo_win[s] = out[i].win;
                            } else {
                                if (cur[s] >= 0) {
                                    const uint64_t lo = out[i].win < lo_win[s] ? out[i].win : lo_win[s];
                                    if (out[i].pos + bytes[i] - lo <= TAMD_LZ_RING) return fail("a message that fits was held back", (long)i, (long)s);
                                }
                                cur[s] = out[i].pass;
                                lo_win[s] = out[i].win;
                            }
                        }
                    }
                    ++cases;
                }
            }
    printf("ok %ld\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "place")) return check_place();
    if (argc == 2 && !strcmp(argv[1], "plan")) return check_plan();
    fprintf(stderr, "usage: cbatch_check place | plan\n");
    return 2;
}
