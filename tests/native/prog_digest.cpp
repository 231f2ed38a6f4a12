// prog_digest.cpp -- TEST ONLY.  Digests of the device programs the host control plane emits for a
// seeded workload, with no device: the session's backend (resident_backend.h) over the streams
// and the loop of cp_bench.cpp (resident_streams.h; device rows are just handles; programs are
// built, digested and dropped).  The contexts are set as a session of more than 4 streams sets
// them; a session of at most 4 streams also sets expand_limit = 16, backsub_rows = 2 and
// short_scans (tamd_session_create), which neither tool does, so the streams <= 4 cases
// (unchunked, burst_arq, column_wrap) pin the control plane but are not a session's programs.
// After every prepare_flush() the pending
// program's instrs(), ops() and op_levels() and its acc_bytes() / store_bytes() are folded into
// one FNV-1a value per (stream, program); a change of the control plane that is meant to leave
// the emitted programs alone must leave every value alone (tests/test_program_identity.py).
//
// usage: prog_digest streams=S n=N step=K [cp_bench's workload keys] [list=0]
// Prints one JSON line: the per-program digests in (program, stream) order ("programs"; with list=0
// only their count), one digest over all of them ("digest"), and what the run exercised: DENSE
// runs, DENSE runs with 2-3 targets, ADJ words, and Siamese rows summed from two or more chunk
// partials (ops that read at least two rows stored by single-target DENSE ops of the same program).
#include "resident_streams.h"

#include <string.h>
#include <unordered_set>

using namespace tamd;

static const uint64_t kFnvBasis = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
static uint64_t fnv(uint64_t h, const void* data, size_t n) {
    const uint8_t* p = (const uint8_t*)data;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * kFnvPrime;
    return h;
}
static uint64_t fnv_u64(uint64_t h, uint64_t v) { return fnv(h, &v, sizeof(v)); }

struct Reach { uint64_t dense_runs = 0, dense_multi = 0, adj_words = 0, chunked_rows = 0; };

static uint64_t digest_program(const ProgramBuilder& pb, Reach& reach) {
    const auto& ins = pb.instrs();
    const auto& ops = pb.ops();
    const auto& lv = pb.op_levels();
    uint64_t h = kFnvBasis;
    h = fnv_u64(h, ins.size());
    h = fnv(h, ins.data(), ins.size() * sizeof(tamd_instr));
    h = fnv_u64(h, ops.size());
    h = fnv(h, ops.data(), ops.size() * sizeof(tamd_op));
    h = fnv_u64(h, lv.size());
    h = fnv(h, lv.data(), lv.size() * sizeof(uint32_t));
    h = fnv_u64(h, pb.acc_bytes());
    h = fnv_u64(h, pb.store_bytes());
    // what the program exercised
    std::unordered_set<uint32_t> partials;  // rows stored by ops that are single-target DENSE runs only
    for (const tamd_op& o : ops) {
        bool dense = false, other = false;
        for (uint32_t k = o.first; k < o.first + o.count; ++k) {
            const uint32_t w = ins[k].w0, kind = w & 0xff;
            if (kind == TAMD_I_ADJ) ++reach.adj_words;
            if (kind == TAMD_I_ACC || kind == TAMD_I_ACC3 || kind == TAMD_I_STOREC) other = true;
            if (kind != TAMD_I_ACCR) continue;
            if (((w >> 8) & 0xff) != TAMD_R_DENSE) { other = true; continue; }
            ++reach.dense_runs;
            if (((w >> 16) & 0xff) >= 2) { ++reach.dense_multi; other = true; }
            else dense = true;
        }
        if (dense && !other)
            for (uint32_t k = o.first; k < o.first + o.count; ++k)
                if ((ins[k].w0 & 0xff) == TAMD_I_STORE) partials.insert(ins[k].row);
    }
    if (!partials.empty())
        for (const tamd_op& o : ops) {
            uint32_t n = 0;
            for (uint32_t k = o.first; k < o.first + o.count; ++k)
                if ((ins[k].w0 & 0xff) == TAMD_I_ACC && partials.count(ins[k].row)) ++n;
            if (n >= 2) ++reach.chunked_rows;
        }
    return h;
}

int main(int argc, char** argv) {
    gf_init();
    ResidentArgs args;
    uint32_t list = 1;
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        const std::string k(argv[i], eq ? eq - argv[i] : 0);
        const unsigned long long v = eq ? strtoull(eq + 1, nullptr, 0) : 0;
        if (k == "list") list = (uint32_t)v;
        else if (!args.parse(k, v)) {
            fprintf(stderr, "prog_digest: unknown key %s\n", argv[i]);
            return 2;
        }
    }
    const wl::Params& p = args.p;
    const uint32_t streams = args.streams, step = args.step;
    if (!streams || !step || !p.n_originals) return 2;
    ResidentStreams<ResidentBackend> rs(args);
    auto& ctxs = rs.ctxs;
    auto& run = rs.run;
    Reach reach;
    uint64_t all = kFnvBasis, nprog = 0, instrs = 0, nops = 0;
    std::string progs;
    for (uint32_t done = 0; done < p.n_originals; done += step) {
        for (uint32_t s = 0; s < streams; ++s) {
            Context& ctx = *ctxs[s];
            run[s]->advance(step);
            const uint64_t e = ctx.epoch;
            ctx.prepare_flush();
            const uint64_t h = digest_program(ctx.pb, reach);
            instrs += ctx.pb.instrs().size();
            nops += ctx.pb.ops().size();
            all = fnv_u64(all, h);
            ++nprog;
            if (list) {
                char buf[32];
                snprintf(buf, sizeof(buf), "%s\"%016llx\"", progs.empty() ? "" : ", ", (unsigned long long)h);
                progs += buf;
            }
            ctx.finish_flush();
            ctx.rows.release_up_to(e);
        }
    }
    printf("{\"digest\": \"%016llx\", \"n_programs\": %llu, \"instrs\": %llu, \"ops\": %llu, \"dense_runs\": %llu, "
           "\"dense_multi_runs\": %llu, \"adj_words\": %llu, \"chunked_rows\": %llu",
           (unsigned long long)all, (unsigned long long)nprog, (unsigned long long)instrs, (unsigned long long)nops,
           (unsigned long long)reach.dense_runs, (unsigned long long)reach.dense_multi,
           (unsigned long long)reach.adj_words, (unsigned long long)reach.chunked_rows);
    if (list) printf(", \"programs\": [%s]", progs.c_str());
    printf("}\n");
    return 0;
}
