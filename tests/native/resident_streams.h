// resident_streams.h -- TEST ONLY.  The streams of a bench session with no device, for cp_bench
// and prog_digest: per stream one Context, the codecs on the step clock, the resident backend
// over a 65536-row input pool per side (device rows are just handles) and the Runner; and the
// key=value arguments the two tools share.
#pragma once
#include "../../tonk_amd/csrc/resident_backend.h"

#include <stdio.h>
#include <stdlib.h>
#include <string>

namespace tamd {

struct NoTranscript {
    template <class R> void on_encode(int, const R&) {}
    template <class D> void on_decode(int, const std::vector<uint32_t>&, const D&) {}
    void on_ack(int, const uint8_t*, uint32_t, int, uint32_t) {}
    void on_event(char, int, uint32_t, uint32_t) {}
    void on_stats(const uint64_t*, const uint64_t*) {}
    void on_retransmit(int, uint32_t, uint32_t, uint64_t) {}
};

// What the tools set per run.  A session of more than 4 streams sets its contexts the same way
// (tamd_session_create); one of at most 4 also sets expand_limit = 16, backsub_rows = 2 and
// short_scans, which the tools leave at the engine's defaults.
struct ResidentArgs {
    wl::Params p;
    uint32_t streams = 8, step = 4096;
    uint32_t expand = ~0u, backsub = ~0u;
    int dense_split = -1;  // -1: by stream count, as the session
    bool pipeline = true;
    bool nobatch = false;  // nobatch=1: single adds only (the runner's fallback path)
    bool contig = true;    // contig=0: the codecs check run contiguity themselves
    ResidentArgs() {
        p.loss_thresh = 42949673;
        p.fec_rate_q16 = 1311;
        p.ack_every = 64;
        p.n_originals = 4096 * 6;
    }
    // One key=value argument: the shared keys and the workload's (wl::parse_param).  False for
    // a key that is neither.
    bool parse(const std::string& k, unsigned long long v) {
        if (k == "streams") streams = (uint32_t)v;
        else if (k == "step") step = (uint32_t)v;
        else if (k == "nobatch") nobatch = v != 0;
        else if (k == "contig") contig = v != 0;
        else return wl::parse_param(p, k, v);
        return true;
    }
};

static uint64_t g_step_clock = 1000;  // the session reads the clock once per step

template <class Backend>
struct ResidentStreams {
    std::vector<std::unique_ptr<Context>> ctxs;
    std::vector<std::unique_ptr<Backend>> be;
    std::vector<wl::Params> ps;
    NoTranscript tr;
    std::vector<std::unique_ptr<wl::Runner<Backend, NoTranscript>>> run;

    explicit ResidentStreams(const ResidentArgs& a) : ctxs(a.streams), be(a.streams), ps(a.streams, a.p), run(a.streams) {
        // (a pool of 65536 rows per side, as the bench's sessions: long runs fit in memory)
        const uint32_t pool = std::min<uint32_t>(a.p.n_originals, 65536);
        for (uint32_t s = 0; s < a.streams; ++s) {
            ps[s].seed_data = 1000 + s;
            ps[s].seed_loss = 2000 + s;
            ctxs[s].reset(new Context());
            Context& ctx = *ctxs[s];
            ctx.ex.expand_limit = a.expand;
            ctx.backsub_rows = a.backsub;
            ctx.dense_split = a.dense_split >= 0 ? (uint32_t)a.dense_split : (a.streams > 4 ? Encoder::kDenseSplit : 0u);
            ctx.pipeline = a.pipeline;
            ctx.rows.init(4ull * pool * 1344 + (256u << 20));
            be[s].reset(new Backend());
            be[s]->ctx = &ctx;
            be[s]->enc.reset(new Encoder(&ctx, 1344));
            be[s]->enc->set_clock(&g_step_clock);
            be[s]->dec.reset(new Decoder(&ctx, 1344));
            be[s]->nobatch = a.nobatch;
            be[s]->contig = a.contig;
            if (!be[s]->alloc_inputs(a.p.n_originals, pool, 1302)) {
                fprintf(stderr, "arena too small for the inputs\n");
                exit(3);
            }
            run[s].reset(new wl::Runner<Backend, NoTranscript>(ps[s], *be[s], tr));
            run[s]->pregenerate();
        }
    }
};

}  // namespace tamd
