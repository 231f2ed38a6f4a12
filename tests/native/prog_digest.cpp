// prog_digest.cpp -- TEST ONLY.  Digests of the device programs the host control plane emits for a
// seeded workload, with no device: the backend and the loop of cp_bench.cpp (device rows are just
// handles; programs are built, digested and dropped).  After every prepare_flush() the pending
// program's instrs(), ops() and op_levels() and its acc_bytes() / store_bytes() are folded into
// one FNV-1a value per (stream, program); a change of the control plane that is meant to leave
// the emitted programs alone must leave every value alone (tests/test_program_identity.py).
//
// usage: prog_digest streams=S n=N step=K [cp_bench's workload keys] [list=0]
// Prints one JSON line: the per-program digests in (program, stream) order ("programs"; with list=0
// only their count), one digest over all of them ("digest"), and what the run exercised: DENSE
// runs, DENSE runs with 2-3 targets, ADJ words, and Siamese rows summed from two or more chunk
// partials (ops that read at least two rows stored by single-target DENSE ops of the same program).
#include "../../tonk_amd/csrc/decoder.h"
#include "../../tonk_amd/csrc/workload.h"
#include "../../tonk_amd/csrc/prof.h"

#include <memory>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <unordered_set>

using namespace tamd;

static int g_nobatch = 0;
static bool g_contig = true;
static uint64_t g_step_clock = 1000;
struct Null {
    struct RecRef { RecoveryOut out; };
    struct DecRef {};
    Context* ctx;
    Encoder* enc;
    Decoder* dec;
    std::vector<RowId> enc_rows, dec_rows;
    uint32_t pool = 0;  // rows per side; original i uses row i mod pool
    uint64_t layout(const std::vector<RowId>& rows, uint32_t index, uint32_t k) const {
        if (index % pool + k > pool) return 0;
        const uint32_t o0 = ctx->rows.offset(rows[0]), stride = ctx->rows.offset(rows[1]) - o0;
        return (uint64_t)(o0 + (index % pool) * stride) << 32 | stride;
    }
    int enc_add(uint32_t index, uint32_t len, uint32_t* col) {
        const uint32_t hb = length_header_bytes(len);
        return enc->add(enc_rows[index], hb + len, hb, len, nullptr, col, true);
    }
    bool enc_add_run(uint32_t index, uint32_t k, uint32_t len, uint32_t* col0) {
        if (g_nobatch) return false;
        const uint32_t hb = length_header_bytes(len);
        return enc->add_run(&enc_rows[index], k, hb + len, hb, len, true, col0, g_contig ? layout(enc_rows, index, k) : 0);
    }
    bool dec_add_run(uint32_t col0, uint32_t index, uint32_t k, uint32_t len) {
        if (g_nobatch) return false;
        const uint32_t hb = length_header_bytes(len);
        return dec->add_run_inorder(col0, &dec_rows[index], k, hb + len, hb, len, true, g_contig ? layout(dec_rows, index, k) : 0);
    }
    int enc_encode(RecRef& r) { return enc->encode(r.out); }
    int enc_ack(const uint8_t* b, uint32_t n, uint32_t* next) { return enc->acknowledge(b, n, next); }
    int enc_is_ready() { return enc->remaining_slots() <= 2 ? (int)kMaxPacketsReached : 0; }
    int dec_add_original(uint32_t col, uint32_t index, uint32_t len) {
        const uint32_t hb = length_header_bytes(len);
        bool took = false;
        return dec->add_original(col, dec_rows[index], hb + len, hb, len, nullptr, &took, true);
    }
    void recovery_lost(const RecRef& r) { ctx->rows.free_deferred(r.out.row); }
    int dec_add_recovery(const RecRef& r) {
        uint8_t tail[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t tl = r.out.total() < 8 ? r.out.total() : 8;
        memcpy(tail + tl - r.out.footer_len, r.out.footer, r.out.footer_len);
        bool took = false;
        const int rc = dec->add_recovery(r.out.row, r.out.total(), tail, nullptr, &took);
        if (!took) ctx->rows.free_deferred(r.out.row);
        return rc;
    }
    int dec_is_ready() { return dec->is_ready(); }
    std::vector<RecoveredPacket*> got;
    int dec_decode(std::vector<uint32_t>& nums, DecRef&) {
        got.clear();
        const int rc = dec->decode(got);
        if (rc == 0) for (auto* p : got) nums.push_back(p->packet_num);
        return rc;
    }
    int dec_ack(uint8_t* b, uint32_t l, uint32_t* u) { return dec->ack(b, l, u); }
    void stats(uint64_t e[9], uint64_t d[11]) { enc->stats(e, 9); dec->stats(d, 11); }
    void set_time(uint64_t) {}
    int enc_retransmit(uint32_t*, uint32_t*, const uint8_t**) { return 2; }
};

struct NoTr {
    void on_encode(int, const Null::RecRef&) {}
    void on_decode(int, const std::vector<uint32_t>&, const Null::DecRef&) {}
    void on_ack(int, const uint8_t*, uint32_t, int, uint32_t) {}
    void on_event(char, int, uint32_t, uint32_t) {}
    void on_stats(const uint64_t*, const uint64_t*) {}
    void on_retransmit(int, uint32_t, uint32_t, uint64_t) {}
};

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
    wl::Params p;
    p.loss_thresh = 42949673;
    p.fec_rate_q16 = 1311;
    p.ack_every = 64;
    uint32_t streams = 8, step = 4096, list = 1;
    p.n_originals = 4096 * 6;
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) continue;
        std::string k(argv[i], eq - argv[i]);
        const unsigned long long v = strtoull(eq + 1, nullptr, 0);
        if (k == "nobatch") g_nobatch = (int)v;
        else if (k == "contig") g_contig = v != 0;
        else if (k == "list") list = (uint32_t)v;
        else if (k == "streams") streams = (uint32_t)v;
        else if (k == "n") p.n_originals = (uint32_t)v;
        else if (k == "step") step = (uint32_t)v;
        else if (k == "loss") p.loss_thresh = (uint32_t)v;
        else if (k == "fec") p.fec_rate_q16 = (uint32_t)v;
        else if (k == "ack") p.ack_every = (uint32_t)v;
        else if (k == "ge") p.ge_enable = (uint32_t)v;
        else if (k == "gb") p.gb_thresh = (uint32_t)v;
        else if (k == "bg") p.bg_thresh = (uint32_t)v;
        else if (k == "arq") p.arq_lag = (uint32_t)v;
        else {
            fprintf(stderr, "prog_digest: unknown key %s\n", k.c_str());
            return 2;
        }
    }
    if (!streams || !step || !p.n_originals) return 2;
    // One Context per stream with each side's input rows contiguous, as cp_bench lays them out.
    std::vector<std::unique_ptr<Context>> ctxs(streams);
    std::vector<std::unique_ptr<Null>> be(streams);
    std::vector<std::unique_ptr<Encoder>> encs(streams);
    std::vector<std::unique_ptr<Decoder>> decs(streams);
    std::vector<wl::Params> ps(streams, p);
    NoTr tr;
    std::vector<std::unique_ptr<wl::Runner<Null, NoTr>>> run(streams);
    for (uint32_t s = 0; s < streams; ++s) {
        ps[s].seed_data = 1000 + s;
        ps[s].seed_loss = 2000 + s;
        ctxs[s].reset(new Context());
        Context& ctx = *ctxs[s];
        ctx.dense_split = streams > 4 ? Encoder::kDenseSplit : 0u;
        ctx.pipeline = true;
        ctx.rows.init(4ull * std::min<uint32_t>(p.n_originals, 65536) * 1344 + (256u << 20));
        encs[s].reset(new Encoder(&ctx, 1344));
        encs[s]->set_clock(&g_step_clock);
        decs[s].reset(new Decoder(&ctx, 1344));
        be[s].reset(new Null());
        be[s]->ctx = &ctx;
        be[s]->enc = encs[s].get();
        be[s]->dec = decs[s].get();
        const uint32_t pool = std::min<uint32_t>(p.n_originals, 65536);
        be[s]->pool = pool;
        for (uint32_t i = 0; i < pool; ++i) be[s]->enc_rows.push_back(ctx.rows.alloc(1302));
        for (uint32_t i = 0; i < pool; ++i) be[s]->dec_rows.push_back(ctx.rows.alloc(1302));
        for (uint32_t i = pool; i < p.n_originals; ++i) be[s]->enc_rows.push_back(be[s]->enc_rows[i - pool]);
        for (uint32_t i = pool; i < p.n_originals; ++i) be[s]->dec_rows.push_back(be[s]->dec_rows[i - pool]);
        run[s].reset(new wl::Runner<Null, NoTr>(ps[s], *be[s], tr));
        run[s]->pregenerate();
    }
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
