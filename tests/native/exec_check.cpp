// exec_check.cpp -- TEST ONLY.  Differential test of the program executor (kernels.hip run_item /
// run_accr / exec_level) against the CPU interpreter of the program format
// (oracle/siamese_oracle.c oracle_run_program).
//
// A case is a small arena image (seeded random bytes, guard rows between and after the rows in
// use) and one program built through ProgramBuilder's public op API, so span, full, level, cost
// class and op_pure are what the product computes.  The interpreter's image is the expected
// result; the device image after the run is compared with it bit for bit over the WHOLE arena,
// guards and unused space included.
//
// usage: exec_check <mode> [only=<substring of the case name>]
//   list    one JSON line per case: name, group, contexts, multi-target DENSE (no device)
//   cpu     build + validate + interpret every case; one JSON line with digest and reach record
//   mutate  per case and claimed feature: semantic mutations must change the interpreter's image
//   reject  validate_program must refuse a hand-made violation of each precondition
//   launch  every case on the GPU through Device::run (tamd_exec24, or tamd_exec16 with
//           TONK_AMD_SLICE=1024)
//   serve   every one-context case through Server::build / post / wait (tamd_serve)
// GPU modes print {name, ok, first_bad_offset, row, byte_in_row, want, got} per case, stop at the
// first HIP error (exit 3, the case named on stderr) and go on after a mere mismatch (exit 1 at
// the end).
//
// Adding a case: append a Spec in add_cases() (fixed seed, a builder over Case's helpers).  Every
// new instruction kind or run mode needs cases here, a decoder arm in parse_run()/validate, its
// reach facts in tests/test_exec_kernel.py and, where it has a parameter, a mutation.
#include "../../tonk_amd/csrc/server.h"
#include "../../oracle/siamese_oracle.h"

#include <algorithm>
#include <functional>
#include <memory>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <unistd.h>
#include <vector>

using namespace tamd;

static const uint64_t kArena = 2ull << 20;  // the whole device arena of a case
static const uint32_t kL[] = {1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1300, 1302,
                              1535, 1536, 1537, 2047, 2048, 2049, 3071, 3072, 3073, 9008};
static const uint32_t kC[] = {1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 19, 20, 21, 24, 25, 63, 64, 65, 127, 128, 129};
static const size_t kNL = sizeof(kL) / sizeof(kL[0]), kNC = sizeof(kC) / sizeof(kC[0]);

struct Rng {  // splitmix64
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t u(uint32_t n) { return (uint32_t)(next() % n); }
    uint32_t in(uint32_t lo, uint32_t hi) { return lo + u(hi - lo + 1); }
    uint8_t nz() { return (uint8_t)(1 + u(255)); }         // a nonzero byte
    uint8_t coef() { return (uint8_t)(2 + u(254)); }       // neither 0 nor 1
};

static void die(const std::string& m) {
    fprintf(stderr, "exec_check: %s\n", m.c_str());
    exit(2);
}

// ---------------------------------------------------------------------------------------------
// A program as plain vectors (what the interpreter, the validator and the mutations work on)
// ---------------------------------------------------------------------------------------------
struct Prog {
    std::vector<tamd_op> ops;
    std::vector<tamd_instr> in;
    std::vector<uint32_t> bucket;  // TAMD_COST_CLASSES * level + class, per op
    std::vector<uint8_t> pure;
};
static Prog prog_of(const ProgramBuilder& pb) {
    Prog p;
    p.ops = pb.ops();
    p.in.assign(pb.instrs().begin(), pb.instrs().end());
    p.bucket = pb.op_levels();
    p.pure = pb.op_pure();
    return p;
}
static uint32_t kind_of(const tamd_instr& w) { return w.w0 & 0xffu; }

// One ACCR with its payload words.
struct Run {
    uint32_t at = 0, words = 0;  // index of the ACCR word, words in all
    uint32_t mode = 0, p = 0, scale = 0, row0 = 0, len = 0, count = 0, stride = 0, col0 = 0, cstep = 0;
    uint32_t nt = 0;             // DENSE targets (1..3); MULTI: 3 target words
    uint32_t coefs[3] = {0, 0, 0}, nadj[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // COEFS index, ADJ words, range end
    uint32_t targets = 0;        // MULTI: index of the TARGETS word
};
// Decode the run at `at` (an ACCR word) of an op ending at `end`; "" or what is malformed.
static std::string parse_run(const std::vector<tamd_instr>& in, uint32_t at, uint32_t end, Run& r) {
    r = Run();
    r.at = at;
    if (at + 1 >= end || kind_of(in[at + 1]) != TAMD_I_RANGE) return "ACCR without RANGE";
    const tamd_instr &a = in[at], &g = in[at + 1];
    r.mode = (a.w0 >> 8) & 0xffu, r.p = (a.w0 >> 16) & 0xffu, r.scale = a.w0 >> 24;
    r.row0 = a.row, r.len = a.len, r.count = a.cap, r.stride = g.row, r.col0 = g.len, r.cstep = g.cap;
    r.words = 2;
    if (r.mode == TAMD_R_MULTI) {
        if (at + 2 >= end || kind_of(in[at + 2]) != TAMD_I_TARGETS) return "MULTI without TARGETS";
        r.targets = at + 2;
        r.words = 3;
    } else if (r.mode == TAMD_R_DENSE) {
        r.nt = r.p > 1 ? r.p : 1;
        if (r.nt > 3) return "DENSE with more than three targets";
        uint32_t k = at + 2;
        for (uint32_t t = 0; t < r.nt; ++t) {
            if (k >= end || kind_of(in[k]) != TAMD_I_COEFS) return "DENSE without COEFS";
            r.coefs[t] = k;
            r.nadj[t] = r.nt > 1 ? in[k].cap & 0xffffu : in[k].cap;
            r.hi[t] = r.nt > 1 ? in[k].cap >> 16 : r.count;
            if (r.nadj[t] > end - k - 1) return "ADJ words past the op";
            for (uint32_t q = 0; q < r.nadj[t]; ++q)
                if (kind_of(in[k + 1 + q]) != TAMD_I_ADJ) return "COEFS.cap counts a word that is no ADJ";
            k += 1 + r.nadj[t];
        }
        r.words = k - at;
    } else if (r.mode != TAMD_R_LANE3 && r.mode != TAMD_R_CAUCHY && r.mode != TAMD_R_CONST) {
        return "unknown run mode";
    }
    return "";
}
static uint32_t adj_entry(const std::vector<tamd_instr>& in, uint32_t first_word, uint32_t q) {
    const uint32_t* w = &in[first_word + q / 4].w0;
    const uint32_t d = w[q & 3u];
    return (q & 3u) == 0 ? d & ~0xffu : d;  // (dword 0 carries the word's kind)
}

// ---------------------------------------------------------------------------------------------
// Preconditions (program.h "Preconditions"): no program that fails them may reach a GPU.
// ---------------------------------------------------------------------------------------------
struct RowInfo { uint32_t off, units; bool guard; };
struct Span { uint64_t lo, hi; };  // bytes [lo, hi)
struct Access { uint32_t level; std::vector<Span> rd, wr; };

static const RowInfo* row_at(const std::vector<RowInfo>& rows, uint64_t byte) {  // rows sorted by off
    size_t lo = 0, hi = rows.size();
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if ((uint64_t)rows[mid].off * 64 <= byte) lo = mid + 1; else hi = mid;
    }
    if (!lo) return nullptr;
    const RowInfo& r = rows[lo - 1];
    return byte < ((uint64_t)r.off + r.units) * 64 ? &r : nullptr;
}
static bool inside_row(const std::vector<RowInfo>& rows, uint64_t lo, uint64_t hi) {
    if (hi <= lo) return true;
    const RowInfo* r = row_at(rows, lo);
    return r && !r->guard && hi <= ((uint64_t)r->off + r->units) * 64;
}

// Format and address rules of one program; fills `acc` with what each op reads and writes.  The
// executor's loads are 16 (or 8) bytes per lane at offsets below `len`, rows are whole 64-byte
// units, and a run's loads past its end are clamped to its last row: a read of [row, row + len)
// inside one allocated row therefore keeps every load of the executor inside that row.
static std::string validate_format(const Prog& p, const std::vector<RowInfo>& rows, std::vector<Access>& acc) {
    char buf[160];
    for (size_t o = 0; o < p.ops.size(); ++o) {
        const tamd_op& op = p.ops[o];
        auto err = [&](const std::string& m) {
            snprintf(buf, sizeof buf, "op %zu: %s", o, m.c_str());
            return std::string(buf);
        };
        if ((uint64_t)op.first + op.count > p.in.size()) return err("instructions past the program");
        if (op.span & 7u) return err("span is no multiple of 8");
        if (op.full > op.span) return err("full > span");
        Access a;
        a.level = p.bucket[o] / TAMD_COST_CLASSES;
        if (!a.level) return err("level 0");
        const uint32_t end = op.first + op.count;
        uint32_t stores = 0, after_store = 0;
        bool impure = false;
        auto use_len = [&](uint32_t len) -> const char* {
            if (len > op.span) return "length > span";
            if (len < op.full) return "length < full";
            return nullptr;
        };
        for (uint32_t k = op.first; k < end;) {
            const tamd_instr& w = p.in[k];
            const uint32_t kind = kind_of(w);
            if (kind == TAMD_I_ACC || kind == TAMD_I_ACC3) {
                if (kind == TAMD_I_ACC && ((w.w0 >> 16) & 0xffu) > 2) return err("ACC accumulator > 2");
                if (kind == TAMD_I_ACC3 || ((w.w0 >> 16) & 0xffu)) impure = true;
                if (!w.len) return err("ACC of no bytes");
                if (const char* e = use_len(w.len)) return err(e);
                const uint64_t b = (uint64_t)w.row * 64;
                if (!inside_row(rows, b, b + w.len)) return err("ACC reads outside an allocated row");
                a.rd.push_back(Span{b, b + w.len});
                after_store += stores ? 1 : 0;
                ++k;
            } else if (kind == TAMD_I_CLEAR) {
                impure = true;
                after_store += stores ? 1 : 0;
                ++k;
            } else if (kind == TAMD_I_STORE || kind == TAMD_I_STOREC) {
                const bool st = kind == TAMD_I_STORE;
                uint32_t flen = 0;
                if (st) {
                    if (k + 1 >= end || kind_of(p.in[k + 1]) != TAMD_I_FOOTER) return err("STORE without FOOTER");
                    flen = (w.w0 >> 8) & 0xffu;
                    if (flen > 8) return err("footer > 8 bytes");
                    if (((w.w0 >> 16) & 0xffu) > 2) return err("STORE accumulator > 2");
                    ++stores;
                } else {
                    impure = true;
                }
                if (const char* e = use_len(w.len)) return err(e);
                if ((uint64_t)w.len + flen > w.cap) return err("len + footer > cap");
                if (w.cap & 7u) return err("cap is no multiple of 8");
                if (w.cap > op.span) return err("cap > span");
                const uint64_t b = (uint64_t)w.row * 64;
                if (!inside_row(rows, b, b + w.cap)) return err("store writes outside an allocated row");
                a.wr.push_back(Span{b, b + w.cap});
                k += st ? 2 : 1;
            } else if (kind == TAMD_I_ACCR) {
                Run r;
                const std::string e = parse_run(p.in, k, end, r);
                if (!e.empty()) return err(e);
                after_store += stores ? 1 : 0;
                if (!r.count) return err("run of no rows");
                if (!r.len) return err("run of no bytes");
                if (const char* e2 = use_len(r.len)) return err(e2);
                if (r.col0 >= TAMD_COLUMN_PERIOD) return err("col0 past the column period");
                if (r.mode == TAMD_R_LANE3) {
                    impure = true;
                    if ((uint64_t)r.col0 + (uint64_t)(r.count - 1) * r.cstep >= TAMD_COLUMN_PERIOD)
                        return err("LANE3 run crosses the column wrap");
                }
                if (r.scale && r.mode != TAMD_R_CAUCHY && !(r.mode == TAMD_R_DENSE && r.nt == 1))
                    return err("scale on a run that has none");
                if (r.mode == TAMD_R_CAUCHY && r.p >= kCauchyMaxRows) return err("CAUCHY row >= 192");
                if (r.mode == TAMD_R_MULTI) {
                    impure = true;
                    const uint32_t* t = &p.in[r.targets].row;
                    for (unsigned q = 0; q < 3; ++q) {
                        const uint32_t kd = t[q] & 3u, lo = (t[q] >> 10) & 0x7ffu, hi = t[q] >> 21;
                        if (kd == 0) {
                            if (t[q]) return err("unused MULTI target with a window");
                            continue;
                        }
                        if (kd != TAMD_R_CAUCHY && kd != TAMD_R_CONST) return err("MULTI target kind");
                        if (kd == TAMD_R_CAUCHY && ((t[q] >> 2) & 0xffu) >= kCauchyMaxRows) return err("CAUCHY row >= 192");
                        if (hi > r.count) return err("MULTI hi > count");
                        if (lo > hi) return err("MULTI lo > hi");
                    }
                    // (lo and hi are 11-bit fields: hi <= count keeps count within them when hi = count)
                }
                if (r.mode == TAMD_R_DENSE) {
                    for (uint32_t t = 0; t < r.nt; ++t) {
                        if (r.hi[t] > r.count) return err("DENSE target range past the run");
                        if (t && r.hi[t] < r.hi[t - 1]) return err("DENSE target ranges are not nested");
                        bool empty_seen = false;
                        uint32_t last = 0;
                        for (uint32_t q = 0; q < 4 * r.nadj[t]; ++q) {
                            const uint32_t d = adj_entry(p.in, r.coefs[t] + 1, q);
                            if (!(d & 0xff00u)) {  // delta 0: an empty entry
                                if (d) return err("empty ADJ entry with an index");
                                empty_seen = true;
                                continue;
                            }
                            if (empty_seen) return err("ADJ entry after an empty one");
                            if ((d >> 16) < last) return err("ADJ entries not ascending");
                            last = d >> 16;
                        }
                    }
                }
                for (uint32_t e2 = 0; e2 < r.count; ++e2) {
                    const uint64_t b = ((uint64_t)r.row0 + (uint64_t)e2 * r.stride) * 64;
                    if (!inside_row(rows, b, b + r.len)) return err("run reads outside an allocated row");
                    a.rd.push_back(Span{b, b + r.len});
                }
                k += r.words;
            } else {
                return err("unknown or stray instruction word");
            }
        }
        // Ops flagged pure may be split over waves: acc_0 only (1) or plain sums into up to three
        // accumulators (2), and nothing after the first STORE but more STOREs (at most three).
        if (p.pure[o]) {
            if (impure) return err("pure op with ACC3 / CLEAR / STOREC / LANE3 / MULTI / acc_1,2");
            if (!stores || stores > 3 || after_store) return err("pure op whose stores are not its last words");
            if (p.pure[o] == 1 && stores != 1) return err("pure op with several stores");
        }
        acc.push_back(a);
    }
    return "";
}
static bool overlap(const std::vector<Span>& a, const std::vector<Span>& b) {
    for (const Span& x : a)
        for (const Span& y : b)
            if (x.lo < y.hi && y.lo < x.hi) return true;
    return false;
}
// Ops of one level run concurrently (and an op's loads of a batch are issued before its stores):
// no op reads what an op of its level -- itself included -- writes, and no two write one place.
static std::string validate_hazards(const std::vector<Access>& acc) {
    char buf[96];
    for (size_t i = 0; i < acc.size(); ++i)
        for (size_t j = 0; j < acc.size(); ++j) {
            if (acc[i].level != acc[j].level) continue;
            if (overlap(acc[i].rd, acc[j].wr)) {
                snprintf(buf, sizeof buf, "op %zu reads a row op %zu of its level writes", i, j);
                return buf;
            }
            if (i < j && overlap(acc[i].wr, acc[j].wr)) {
                snprintf(buf, sizeof buf, "ops %zu and %zu of one level write one row", i, j);
                return buf;
            }
        }
    return "";
}
static std::string validate_program(const Prog* progs, size_t n, std::vector<RowInfo> rows) {
    std::sort(rows.begin(), rows.end(), [](const RowInfo& a, const RowInfo& b) { return a.off < b.off; });
    std::vector<Access> acc;
    for (size_t i = 0; i < n; ++i) {
        const std::string e = validate_format(progs[i], rows, acc);
        if (!e.empty()) return e;
    }
    return validate_hazards(acc);
}

// ---------------------------------------------------------------------------------------------
// Cases
// ---------------------------------------------------------------------------------------------
struct Case {
    std::string name, group;
    uint64_t seed = 0;
    int nctx = 1;
    uint32_t unclaim = 0;  // mutation features the case does not claim (F_* bits)
    std::unique_ptr<Context> ctx[2];
    std::vector<RowInfo> rows;
    std::vector<uint8_t> image;
    Rng rng{0};
    std::vector<std::unique_ptr<std::vector<uint32_t>>> keep_u32;  // storage the builders point into
    std::vector<std::unique_ptr<std::vector<RowId>>> keep_rows;

    void init(int n) {
        nctx = n;
        for (int i = 0; i < n; ++i) {
            ctx[i].reset(new Context());
            ctx[i]->rows.init(kArena / n, (kArena / n / 64) * i);
        }
    }
    ProgramBuilder& pb(int ci = 0) { return ctx[ci]->pb; }
    RowId alloc(uint32_t bytes, int ci = 0) {
        const RowId r = ctx[ci]->rows.alloc(bytes);
        const RowId g = ctx[ci]->rows.alloc(64);  // a guard behind every row
        if (r == kNoRow || g == kNoRow) die("case " + name + ": arena too small");
        rows.push_back(RowInfo{ctx[ci]->rows.offset(r), ctx[ci]->rows.units(r), false});
        rows.push_back(RowInfo{ctx[ci]->rows.offset(g), 1, true});
        return r;
    }
    uint32_t off(RowId r, int ci = 0) { return ctx[ci]->rows.offset(r); }
    // `count` rows of `len` bytes at `stride` units, inside one allocation; the first row's offset
    uint32_t region(uint32_t count, uint32_t stride, uint32_t len, int ci = 0) {
        return off(alloc((count - 1) * stride * 64 + len, ci), ci);
    }
    const uint8_t* footer() {  // eight nonzero bytes that live as long as the case
        keep_u32.emplace_back(new std::vector<uint32_t>(2));
        uint8_t* f = (uint8_t*)keep_u32.back()->data();
        for (int i = 0; i < 8; ++i) f[i] = rng.nz();
        return f;
    }
    void finish() {
        image.resize(kArena);
        Rng fill(seed * 0x100000001B3ull + 0x5EED);
        for (size_t i = 0; i < kArena; i += 8) {
            const uint64_t v = fill.next() | 0x0101010101010101ull;  // (no zero bytes: zero fill shows)
            memcpy(&image[i], &v, 8);
        }
        for (size_t i = 0; i < rows.size(); ++i)
            if (rows[i].guard)
                for (uint32_t b = 0; b < 64; ++b) image[(size_t)rows[i].off * 64 + b] = (uint8_t)(0xC3u ^ (i * 7u) ^ b);
    }
    std::vector<Prog> progs() {
        std::vector<Prog> v;
        for (int i = 0; i < nctx; ++i) v.push_back(prog_of(ctx[i]->pb));
        return v;
    }
};

struct Spec {
    std::string name, group;
    uint64_t seed;
    std::function<void(Case&)> fn;
};
static std::unique_ptr<Case> build_case(const Spec& s) {
    std::unique_ptr<Case> c(new Case());
    c->name = s.name, c->group = s.group, c->seed = s.seed;
    c->rng = Rng(s.seed);
    s.fn(*c);
    if (!c->ctx[0]) die("case " + s.name + " built nothing");
    c->finish();
    return c;
}

static uint32_t tword(uint32_t kind, uint32_t p, uint32_t lo, uint32_t hi) { return kind | p << 2 | lo << 10 | hi << 21; }
static uint64_t rnd_ops(Rng& r) { return r.next() & 0xffffffffffffull; }
static uint32_t units_of(uint32_t len) { return (len + 63) / 64; }

// A CLEAR word: no emitter of the product writes one, the executor and the interpreter both know it.
static void op_clear(ProgramBuilder& pb) {
    tamd_instr* w = pb.reserve(1);
    w->w0 = TAMD_I_CLEAR, w->row = 0, w->len = 0, w->cap = 0;
    pb.commit(w + 1);
}

// A multi-target DENSE range through emit_dense_range: `total` packets of `len` bytes in `nruns`
// runs, targets with range ends hi[0..n) (nested), each with pair entries of its own; split > 0
// cuts the range into partial sums summed one level up.
static void dense_range(Case& c, uint32_t n, const uint32_t* hi, uint32_t len, uint32_t nruns, uint32_t split,
                        uint32_t col0, uint32_t pairs_each, int ci = 0) {
    Rng& g = c.rng;
    const uint32_t total = hi[n - 1];
    std::vector<DenseRun> runs;
    uint32_t e0 = 0;
    for (uint32_t r = 0; r < nruns; ++r) {
        const uint32_t cnt = r + 1 == nruns ? total - e0 : std::max(1u, total / nruns);
        const uint32_t stride = units_of(len) + (r & 1u);
        runs.push_back(DenseRun{c.region(cnt, stride, len, ci), stride, cnt, len, (col0 + e0) & (TAMD_COLUMN_PERIOD - 1), e0});
        e0 += cnt;
    }
    const uint32_t chunks = split && total > split ? (total + split - 1) / split : 1u;
    std::vector<ProgramBuilder::DenseTarget> tg(n);
    for (uint32_t t = 0; t < n; ++t) {
        ProgramBuilder::DenseTarget& d = tg[t];
        memset(&d, 0, sizeof d);
        d.ops = t == 1 ? 0xffffffffffffull : rnd_ops(g);
        d.rx = t == 2 ? 1 : g.coef();
        d.hi = hi[t];
        c.keep_u32.emplace_back(new std::vector<uint32_t>());
        std::vector<uint32_t>& pr = *c.keep_u32.back();
        // pair entries on packets of the range: its first and last, block edges, a doubled one
        std::vector<uint32_t> rel;
        const uint32_t cand[] = {0, hi[t] - 1, 63, 64, 65, hi[t] / 2, hi[t] / 2};
        for (uint32_t q = 0; q < pairs_each && q < 7; ++q)
            if (cand[q] < hi[t]) rel.push_back(cand[q]);
        for (uint32_t q = 7; q < pairs_each; ++q) rel.push_back(g.u(hi[t]));
        std::sort(rel.begin(), rel.end());
        for (uint32_t x : rel) pr.push_back(x << 8 | g.nz());
        d.pairs = pr.data();
        d.npairs = (uint32_t)pr.size();
        d.dst = c.alloc(len + 8, ci);
        const uint32_t mine = split && hi[t] > split ? (hi[t] + split - 1) / split : 1u;
        if (chunks > 1 && mine > 1) {
            c.keep_rows.emplace_back(new std::vector<RowId>());
            std::vector<RowId>& parts = *c.keep_rows.back();
            for (uint32_t q = 0; q < mine; ++q) parts.push_back(c.alloc(len, ci));
            d.parts = parts.data();
            d.nparts = mine;
        }
        d.footer = c.footer();
        d.flen = 1 + t;
    }
    c.pb(ci).emit_dense_range(runs.data(), runs.size(), tg.data(), n, split, len, false);
}

static void add_cases(std::vector<Spec>& out) {
    uint64_t seed = 1000;
    auto add = [&](const std::string& group, const std::string& name, std::function<void(Case&)> fn) {
        out.push_back(Spec{group + "/" + name, group, ++seed, std::move(fn)});
    };
    static const uint8_t kCoefs[3] = {1, 2, 0xff};

    // ---- acc_store: one ACC + STORE per op; footers 0..8; caps L + F, the next 64, slices larger
    for (size_t li = 0; li < kNL; ++li) {
        const uint32_t L = kL[li];
        add("acc_store", "L" + std::to_string(L), [L](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            for (uint32_t F = 0; F <= 8; ++F)
                for (uint32_t v = 0; v < 3; ++v) {
                    const uint32_t i = F * 3 + v;
                    const uint32_t bytes = v == 0 ? L + F : v == 1 ? L + F + 64 : L + F + 3 * 1536 + 200;
                    const RowId src = c.alloc(L), dst = c.alloc(bytes);
                    const uint8_t coef = (i & 3u) < 3 ? kCoefs[i & 3u] : c.rng.coef();
                    if (i & 1u) {
                        pb.begin_op();
                        pb.op_acc(src, coef, L);
                        pb.op_store(dst, L, 0, c.footer(), F);
                        pb.end_op();
                    } else {
                        const Term t{src, L, coef};
                        pb.combine(dst, &t, 1, L, c.footer(), F);
                    }
                }
            // mixed source lengths: full < span, slices FULL / masked / partial in one op
            const uint32_t l2 = L > 1600 ? 1600 : (L + 1) / 2, l3 = L > 16 ? L - 9 : L;
            const RowId a = c.alloc(L), b = c.alloc(l2), d = c.alloc(l3), dst = c.alloc(L + 5 + 2 * 1536);
            pb.begin_op();
            pb.op_acc(a, 1, L);
            pb.op_acc(b, c.rng.coef(), l2);
            pb.op_acc(d, c.rng.coef(), l3);
            pb.op_store(dst, L, 0, c.footer(), 5);
            pb.end_op();
        });
    }

    // ---- batching: instruction batches of 5 (exec24, serve) and 6 (exec16)
    for (uint32_t N = 1; N <= 14; ++N)
        add("batching", "plain" + std::to_string(N), [N](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            const uint32_t L = 1300;
            pb.begin_op();
            for (uint32_t a = 0; a < 3; ++a)  // every accumulator gets a row whatever N is
                pb.op_acc(c.alloc(L), c.rng.coef(), L, a);
            for (uint32_t i = 0; i < N; ++i)
                pb.op_acc(c.alloc(L), i & 1u ? 1 : c.rng.coef(), L, i % 5 == 3 ? 1 : i % 7 == 5 ? 2 : 0);
            for (uint32_t a = 0; a < 3; ++a) pb.op_store(c.alloc(L + 8), L, a, c.footer(), 5 - a);
            pb.end_op();
            // the same count ending in one STORE (N + 2 words)
            pb.begin_op();
            for (uint32_t i = 0; i < N; ++i) pb.op_acc(c.alloc(L), c.rng.coef(), L);
            pb.op_store(c.alloc(L + 8), L, 0, c.footer(), 8);
            pb.end_op();
        });
    for (uint32_t P = 0; P <= 6; ++P)
        add("batching", "accr_at" + std::to_string(P), [P](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            const uint32_t L = 1300, st = units_of(L);
            pb.begin_op();
            for (uint32_t i = 0; i < P; ++i) pb.op_acc(c.alloc(L), c.rng.coef(), L);
            pb.op_accr(TAMD_R_CAUCHY, c.rng.u(192), c.region(7, st, L), st, 7, L, c.rng.u(1000), 1);
            for (uint32_t i = 0; i < 3; ++i) pb.op_acc(c.alloc(L), c.rng.coef(), L);
            pb.op_accr(TAMD_R_CONST, c.rng.coef(), c.region(3, st, L), st, 3, L, 5, 1);
            pb.op_store(c.alloc(L + 8), L, 0, c.footer(), 4);
            pb.end_op();
        });
    add("batching", "clear", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        const uint32_t L = 1300;
        pb.begin_op();
        for (uint32_t i = 0; i < 3; ++i) pb.op_acc(c.alloc(L), c.rng.coef(), L, i);
        for (uint32_t i = 0; i < 3; ++i) pb.op_store(c.alloc(L + 8), L, i, c.footer(), 3 + i);
        op_clear(pb);
        pb.op_acc(c.alloc(L), c.rng.coef(), L, 0);
        pb.op_acc(c.alloc(L), 1, L, 1);
        pb.op_store(c.alloc(L + 8), L, 0, c.footer(), 2);
        pb.op_store(c.alloc(L + 8), L, 1, c.footer(), 0);
        pb.op_store(c.alloc(L + 8), L, 2, c.footer(), 1);  // acc_2 after the CLEAR: zeros
        pb.end_op();
    });

    // ---- acc3_storec: ACC3 chains, LANE3 runs, STOREC combinations
    for (size_t ci = 0; ci < kNC; ++ci) {
        const uint32_t C = kC[ci];
        add("acc3_storec", "C" + std::to_string(C), [C, ci](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            for (uint32_t v = 0; v < 2; ++v) {
                const uint32_t L = kL[(2 * ci + v + 3) % (kNL - 1)], st = units_of(L) + v, cstep = v ? 8 : 1;
                // v = 1: the run ends on the last column before the 22-bit wrap
                const uint32_t col0 = v ? TAMD_COLUMN_PERIOD - 1 - (C - 1) * cstep : c.rng.u(1u << 20);
                pb.begin_op();
                pb.op_acc3_off(c.off(c.alloc(L)), c.rng.coef(), c.rng.coef(), L);
                pb.op_accr(TAMD_R_LANE3, 0, c.region(C, st, L), st, C, L, col0, cstep);
                pb.op_acc3_off(c.off(c.alloc(L)), 1, c.rng.coef(), L);
                for (uint32_t s = 0; s < 3; ++s) {
                    const uint32_t k = (uint32_t)(ci * 6 + v * 3 + s) % 27u;  // c0, c1, c2 in {0, 1, other}
                    uint8_t cc[3];
                    for (uint32_t a = 0, q = k; a < 3; ++a, q /= 3) cc[a] = q % 3 == 0 ? 0 : q % 3 == 1 ? 1 : c.rng.coef();
                    if (!cc[s]) cc[s] = s == 1 ? c.rng.coef() : 1;  // (every accumulator reaches a store of the op)
                    pb.op_storec(c.alloc(L + (s ? 64 * s : 0)), L, cc);
                }
                pb.end_op();
            }
        });
    }
    add("acc3_storec", "parts", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        const uint32_t L = 1302, wunits = units_of(L), wcap = wunits * 64;
        pb.begin_op();
        for (uint32_t i = 0; i < 7; ++i) pb.op_acc3_off(c.off(c.alloc(L)), c.rng.coef(), c.rng.coef(), L);
        const RowId d = c.alloc(3 * wcap);
        static const uint8_t unit[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (uint32_t s = 0; s < 3; ++s) pb.op_storec_part(d, s * wunits, L, wcap, unit[s], s == 0);
        pb.end_op();
        // and read back by parts one level up
        pb.begin_op();
        for (uint32_t s = 0; s < 3; ++s) pb.op_acc_part(d, s * wunits, c.rng.coef(), wcap, s);
        uint8_t cc[3] = {1, 1, 1};
        pb.op_storec(c.alloc(wcap), L, cc);
        pb.end_op();
    });

    // ---- runs: CONST, CAUCHY, scaled CAUCHY
    for (size_t ci = 0; ci < kNC; ++ci) {
        const uint32_t C = kC[ci];
        add("runs", "C" + std::to_string(C), [C, ci](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            for (uint32_t v = 0; v < 5; ++v) {
                const uint32_t L = kL[(5 * ci + v) % (kNL - 1)];
                const uint32_t st = units_of(L) + (v == 1 ? 1 : v == 3 ? 37 : v == 4 ? units_of(L) : 0);
                // columns: col mod 64 crossing 63 -> 0 inside the run; v = 2, 4: crossing the 22-bit wrap
                const uint32_t col0 = v == 2 || v == 4 ? TAMD_COLUMN_PERIOD - (C + 1) / 2
                                                         : 64 * c.rng.u(1000) + 63 - (C > 1 ? c.rng.u(std::min(C - 1, 63u)) : 0);
                const uint32_t row0 = c.region(C, st, L);
                const RowId dst = c.alloc(L + 8);
                if (v == 0) {  // parity: CONST p = 1, a pure combine
                    pb.begin_op();
                    pb.op_accr(TAMD_R_CONST, 1, row0, st, C, L, col0, 1);
                    pb.finish_combine(dst, L, c.footer(), 2);
                } else if (v == 1) {
                    pb.begin_op();
                    pb.op_accr(TAMD_R_CONST, c.rng.coef(), row0, st, C, L, col0, 1);
                    pb.op_store(dst, L, 0, c.footer(), 8);
                    pb.end_op();
                } else if (v == 2) {
                    pb.begin_op();
                    pb.op_accr(TAMD_R_CAUCHY, c.rng.u(192), row0, st, C, L, col0, 1);
                    pb.finish_combine(dst, L, c.footer(), 0);
                } else {  // CAUCHY with a scale (2, 255) as combine() emits a scaled run term
                    const Term t = pb.run_term(TAMD_R_CAUCHY, v == 3 ? 191 : c.rng.u(192), row0, st, C, col0, L);
                    Term s = t;
                    s.coef = v == 3 ? 2 : 255;
                    pb.combine(dst, &s, 1, L, c.footer(), 7);
                }
            }
        });
    }

    // ---- multi: ACCR MULTI with 1..3 targets
    for (size_t ci = 0; ci < kNC; ++ci) {
        const uint32_t C = kC[ci];
        add("multi", "C" + std::to_string(C), [C, ci](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            for (uint32_t v = 0; v < 6; ++v) {
                const uint32_t L = kL[(6 * ci + v + 1) % (kNL - 1)], st = units_of(L) + (v & 1u);
                // the odd variants: a column step other than 1 (the format allows any)
                const uint32_t cstep = v == 3 ? 3 : v & 1u ? 8 : 1;
                const uint32_t K = TAMD_R_CAUCHY, X = TAMD_R_CONST;
                auto P = [&]() { return c.rng.u(192); };
                uint32_t t[3] = {0, 0, 0};
                switch (v) {
                case 0: t[0] = tword(K, P(), 0, C / 3), t[1] = tword(X, 0, C / 3, 2 * C / 3), t[2] = tword(K, P(), 2 * C / 3, C); break;
                case 1: t[0] = tword(X, 0, 0, std::min(C, 2 * C / 3 + 1)), t[1] = tword(K, P(), C / 3, C), t[2] = tword(K, P(), 0, C); break;
                case 2: t[0] = tword(K, P(), 0, C), t[1] = tword(K, P(), 0, C), t[2] = tword(X, 0, 0, C); break;
                case 3: t[0] = tword(K, P(), C / 2, C / 2), t[1] = tword(K, P(), 0, C); break;  // an empty window
                case 4: t[0] = tword(K, P(), 0, C); break;
                default: t[0] = tword(X, 0, 0, (C + 1) / 2), t[1] = tword(K, P(), C / 2, C); break;
                }
                pb.begin_op();
                pb.op_accr_multi(c.region(C, st, L), st, C, L, c.rng.u(1u << 22), cstep, t);
                for (uint32_t a = 0; a < 3; ++a) pb.op_store(c.alloc(L + a + 1), L, a, c.footer(), a + 1);
                pb.end_op();
            }
        });
    }

    // ---- dense1: single-target DENSE runs
    for (size_t ci = 0; ci < kNC; ++ci) {
        const uint32_t C = kC[ci];
        add("dense1", "C" + std::to_string(C), [C, ci](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            for (uint32_t v = 0; v < 4; ++v) {
                const uint32_t L = kL[(4 * ci + v + 2) % (kNL - 1)], st = units_of(L) + (v == 2 ? 3 : 0);
                const uint64_t ops = v == 1 ? 0 : v == 2 ? 0xffffffffffffull : rnd_ops(c.rng);
                const uint8_t rx = v == 0 ? c.rng.coef() : v == 1 ? 0 : v == 2 ? 1 : c.rng.coef();
                const uint8_t scale = v == 0 ? 1 : v == 1 ? 2 : v == 2 ? 255 : 1;
                // v = 3: the run crosses the column wrap
                const uint32_t col0 = v == 3 ? TAMD_COLUMN_PERIOD - (C + 1) / 2 : c.rng.u(1u << 22);
                // ADJ entries: none (v = 0 on even cases), one, many; on 0, 63, 64, 65, count - 1; a doubled index
                std::vector<uint32_t> idx;
                if (v == 0 && (ci & 1u)) idx.push_back(C - 1);
                if (v == 1) {  // (all-zero opcodes: the additions are all the run does)
                    const uint32_t cand[] = {0, 63, 64, 65, C - 1, C / 2, C / 2};
                    for (uint32_t x : cand)
                        if (x < C) idx.push_back(x);
                }
                if (v == 2) idx.push_back(0), idx.push_back(C - 1);
                if (v == 3)
                    for (uint32_t q = 0; q < 5 + ci % 4; ++q) idx.push_back(c.rng.u(C));  // (5..8: padded last words)
                std::sort(idx.begin(), idx.end());
                std::vector<uint32_t> adj;
                for (uint32_t x : idx) adj.push_back(x << 16 | (uint32_t)c.rng.nz() << 8);
                pb.begin_op();
                pb.op_accr_dense(c.region(C, st, L), st, C, L, col0, ops, rx, adj.data(), (uint32_t)adj.size(), scale);
                if (v & 1u) pb.op_store(c.alloc(L + 8), L, 0, c.footer(), 6);
                else pb.finish_combine(c.alloc(L + 8), L, c.footer(), 1);
                if (v & 1u) pb.end_op();
            }
        });
    }
    add("dense1", "scale0_and_terms", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        const uint32_t L = 1302, st = units_of(L), C = 70;
        // scale 0 emits nothing; the op's other run still counts
        pb.begin_op();
        pb.op_accr_dense(c.region(C, st, L), st, C, L, 77, rnd_ops(c.rng), 9, nullptr, 0, 0);
        pb.op_accr_dense(c.region(C, st, L), st, C, L, 99, rnd_ops(c.rng), c.rng.coef(), nullptr, 0, 1);
        pb.finish_combine(c.alloc(L + 8), L, c.footer(), 3);
        // as the decoder emits an elimination: a dense run term scaled by the term's coefficient
        const uint32_t keys[3] = {(100u + 0) << 8 | 1, (100u + 64) << 8 | 0x35, (100u + C - 1) << 8 | 1};
        Term t = pb.dense_run_term(c.region(C, st, L), st, C, 4000, rnd_ops(c.rng), c.rng.coef(), keys, 3, 100, L);
        t.coef = 0x8e;
        Term u{c.alloc(L), L, 3};
        Term both[2] = {u, t};
        pb.combine(c.alloc(L + 8), both, 2, L, c.footer(), 4);
    });

    // ---- dense_multi: nested targets (the launch path only: Server::build declines them)
    add("dense_multi", "p2", [](Case& c) {
        c.init(1);
        const uint32_t hi[2] = {40, 100};
        dense_range(c, 2, hi, 300, 2, 0, 12345, 6);
    });
    add("dense_multi", "p3", [](Case& c) {
        c.init(1);
        const uint32_t hi[3] = {40, 70, 129};
        dense_range(c, 3, hi, 1302, 3, 0, TAMD_COLUMN_PERIOD - 50, 7);
    });
    add("dense_multi", "p3_equal_hi", [](Case& c) {
        c.init(1);
        const uint32_t hi[3] = {65, 65, 65};
        dense_range(c, 3, hi, 513, 1, 0, 7, 5);
    });
    add("dense_multi", "p2_split", [](Case& c) {
        c.init(1);
        const uint32_t hi[2] = {30, 100};
        dense_range(c, 2, hi, 300, 2, 48, 999, 9);
    });
    add("dense_multi", "p3_split", [](Case& c) {
        c.init(1);
        const uint32_t hi[3] = {64, 100, 129};
        dense_range(c, 3, hi, 1025, 2, 64, 4242, 8);
    });

    // ---- shared: class-0 pure combines (>= 48 KB of ACC bytes), run by a whole workgroup
    add("shared", "acc_list", [](Case& c) {
        c.init(1);
        std::vector<Term> t;
        for (uint32_t i = 0; i < 61; ++i) t.push_back(Term{c.alloc(1300), 1300, i % 3 ? c.rng.coef() : (uint8_t)1});
        c.pb().combine(c.alloc(1308), t.data(), t.size(), 1300, c.footer(), 8);
    });
    add("shared", "runs_mixed", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        const uint32_t L = 2000, st = units_of(L);  // two 1536-byte slices, the last partial
        std::vector<Term> t;
        t.push_back(pb.run_term(TAMD_R_CONST, 1, c.region(21, st, L), st, 21, 0, L));
        t.push_back(pb.run_term(TAMD_R_CAUCHY, 17, c.region(25, st + 1, L), st + 1, 25, 50, L));
        t.back().coef = 0x1d;
        const uint32_t keys[2] = {3u << 8 | 1, 18u << 8 | 0x77};
        t.push_back(pb.dense_run_term(c.region(19, st, L), st, 19, 1000, rnd_ops(c.rng), c.rng.coef(), keys, 2, 0, L));
        t.push_back(pb.run_term(TAMD_R_CONST, 1, c.region(7, st, L), st, 7, 0, L));
        t.back().coef = 0xa0;
        for (uint32_t i = 0; i < 7; ++i) t.push_back(Term{c.alloc(L), i == 3 ? 1500u : L, c.rng.coef()});
        pb.combine(c.alloc(L + 8), t.data(), t.size(), L, c.footer(), 5);
    });
    add("shared", "dense_p2", [](Case& c) {
        c.init(1);
        const uint32_t hi[2] = {50, 129};
        dense_range(c, 2, hi, 1302, 2, 0, 31337, 7);
    });
    add("shared", "dense_p3", [](Case& c) {
        c.init(1);
        const uint32_t hi[3] = {33, 64, 100};
        dense_range(c, 3, hi, 1700, 1, 0, TAMD_COLUMN_PERIOD - 40, 8);
    });
    add("shared", "store_shared", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        const uint32_t L = 1300, st = units_of(L);
        pb.begin_op();
        for (uint32_t i = 0; i < 9; ++i) pb.op_acc(c.alloc(L), c.rng.coef(), L);
        pb.op_accr(TAMD_R_CAUCHY, 5, c.region(41, st, L), st, 41, L, 60, 1);
        pb.op_accr_dense(c.region(13, st, L), st, 13, L, 9, rnd_ops(c.rng), c.rng.coef());
        pb.op_store_shared(c.alloc(L + 8), L, 0, c.footer(), 7);
        pb.end_op();
    });
    add("shared", "apart", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        // one shared item, nine single-wave items beside it: more workgroups than shared items
        const uint32_t L = 1300, st = units_of(L);
        const Term r = pb.run_term(TAMD_R_CONST, 1, c.region(50, st, L), st, 50, 0, L);
        pb.combine(c.alloc(L + 8), &r, 1, L, c.footer(), 2);
        for (uint32_t i = 0; i < 9; ++i) {
            pb.begin_op();
            pb.op_acc(c.alloc(700), c.rng.coef(), 700, i & 1u);
            pb.op_acc(c.alloc(700), 1, 700, i & 1u);
            pb.op_store(c.alloc(708), 700, i & 1u, c.footer(), 3);
            pb.end_op();
        }
    });
    add("shared", "two_shared_only", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        for (uint32_t i = 0; i < 2; ++i) {
            const uint32_t L = i ? 3073 : 1025, st = units_of(L), C = i ? 23 : 53;
            const Term r = pb.run_term(TAMD_R_CAUCHY, 100 + i, c.region(C, st, L), st, C, 7, L);
            pb.combine(c.alloc(L + 8), &r, 1, L, c.footer(), 1);
        }
    });

    // ---- serve_groups: levels of 1, 2, 3, 4, 5, 8, 9 items (groups of 16, 8, 4, 2 waves, the claim loop)
    static const uint32_t kItems[] = {1, 2, 3, 4, 5, 8, 9};
    for (uint32_t N : kItems)
        add("serve_groups", "n" + std::to_string(N), [N](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            const uint32_t L = 1000, st = units_of(L);
            for (uint32_t i = 0; i < N; ++i) {
                const uint32_t C = 13 + 11 * i;
                if (i & 1u) {  // a non-pure op: the group's first wave alone
                    pb.begin_op();
                    pb.op_accr(TAMD_R_CAUCHY, c.rng.u(192), c.region(C, st, L), st, C, L, 3 * i, 1);
                    pb.op_acc(c.alloc(L), c.rng.coef(), L, 1);
                    pb.op_store(c.alloc(L + 8), L, 0, c.footer(), 4);
                    pb.op_store(c.alloc(L + 8), L, 1, c.footer(), 1);
                    pb.end_op();
                } else {  // a pure combine: its row batches split over the group
                    std::vector<Term> t;
                    t.push_back(pb.run_term(TAMD_R_CAUCHY, c.rng.u(192), c.region(C, st, L), st, C, 61, L));
                    t.back().coef = i & 2u ? 1 : 0x42;
                    for (uint32_t q = 0; q < 6 + i; ++q) t.push_back(Term{c.alloc(L), L, c.rng.coef()});
                    const uint32_t keys[1] = {5u << 8 | 9};
                    t.push_back(pb.dense_run_term(c.region(17, st, L), st, 17, 300, rnd_ops(c.rng), c.rng.coef(), keys, 1, 0, L));
                    pb.combine(c.alloc(L + 8), t.data(), t.size(), L, c.footer(), 6);
                }
            }
        });
    add("serve_groups", "levels_2_1_3", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        const uint32_t L = 1302;
        RowId l1[2], l2;
        for (uint32_t i = 0; i < 2; ++i) {
            std::vector<Term> t;
            for (uint32_t q = 0; q < 12; ++q) t.push_back(Term{c.alloc(L), L, c.rng.coef()});
            pb.combine(l1[i] = c.alloc(L), t.data(), t.size(), L);
        }
        const Term t2[3] = {Term{l1[0], L, 1}, Term{l1[1], L, 0x33}, Term{c.alloc(L), L, 5}};
        pb.combine(l2 = c.alloc(L + 8), t2, 3, L, c.footer(), 2);
        for (uint32_t i = 0; i < 3; ++i) {
            const Term t3[3] = {Term{l2, L - i, c.rng.coef()}, Term{l1[i & 1u], L, 1}, Term{c.alloc(L), L, 7}};
            pb.combine(c.alloc(L + 8), t3, 3, L, c.footer(), 3 + i);
        }
    });

    // ---- levels: level n reads what level n - 1 wrote; a row written twice across levels
    add("levels", "chain3_rewrite", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        const uint32_t L = 2049;
        const RowId x = c.alloc(L + 8), y = c.alloc(L + 16), a = c.alloc(L), b = c.alloc(L);
        const Term t1[2] = {Term{a, L, 2}, Term{b, L, 3}};
        pb.combine(x, t1, 2, L, c.footer(), 8);  // level 1 writes x
        pb.begin_op();
        pb.op_acc(x, c.rng.coef(), L + 8);  // (the footer too)
        pb.op_acc(a, 1, L);
        pb.op_store(y, L + 8, 0, c.footer(), 1);
        pb.end_op();                             // level 2 reads x, writes y
        const Term t3[2] = {Term{y, L + 9, 0x10}, Term{b, 700, 1}};
        pb.combine(x, t3, 2, L + 8, c.footer(), 0);  // level 3 reads y, writes x again
    });
    add("levels", "two_levels_lanes", [](Case& c) {
        c.init(1);
        ProgramBuilder& pb = c.pb();
        const uint32_t L = 513, st = units_of(L);
        pb.begin_op();
        pb.op_accr(TAMD_R_LANE3, 0, c.region(9, st, L), st, 9, L, 1000, 8);
        uint8_t c0[3] = {1, 0, 0}, c1[3] = {0, 1, 0}, c2[3] = {0, 0, 1};
        const RowId s0 = c.alloc(L), s1 = c.alloc(L), s2 = c.alloc(L);
        pb.op_storec(s0, L, c0), pb.op_storec(s1, L, c1), pb.op_storec(s2, L, c2);
        pb.end_op();
        pb.begin_op();
        pb.op_acc(s0, 1, L, 0), pb.op_acc(s1, 1, L, 1), pb.op_acc(s2, 1, L, 2);
        pb.op_accr(TAMD_R_LANE3, 0, c.region(4, st, L), st, 4, L, 1072, 8);
        uint8_t cc[3] = {c.rng.coef(), 1, c.rng.coef()};
        pb.op_storec(c.alloc(L), L, cc);
        pb.end_op();
    });

    // ---- merged: two contexts in one program (Device::run(ctxs, 2))
    for (uint32_t m = 0; m < 3; ++m)
        add("merged", "m" + std::to_string(m), [m](Case& c) {
            c.init(2);
            for (int ci = 0; ci < 2; ++ci) {
                ProgramBuilder& pb = c.pb(ci);
                const uint32_t L = ci ? 1537 : 1023, st = units_of(L);
                const uint32_t nops = 2 + m + ci;
                RowId prev = kNoRow;
                for (uint32_t i = 0; i < nops; ++i) {
                    std::vector<Term> t;
                    t.push_back(pb.run_term(i & 1u ? TAMD_R_CAUCHY : TAMD_R_CONST, i & 1u ? 7 + i : 1, c.region(9 + 20 * i * m, st, L, ci),
                                            st, 9 + 20 * i * m, 30, L));
                    t.push_back(Term{c.alloc(L, ci), L, c.rng.coef()});
                    if (prev != kNoRow && (i & 1u)) t.push_back(Term{prev, L, c.rng.coef()});  // a second level
                    pb.combine(prev = c.alloc(L + 8, ci), t.data(), t.size(), L, c.footer(), i);
                }
                if (m == 2) {
                    const uint32_t hi[2] = {20, 70};
                    dense_range(c, 2, hi, L, 1, 0, 555, 4, ci);
                }
            }
        });

    // ---- fuzz: 64 seeded random programs within the preconditions
    for (uint32_t f = 0; f < 64; ++f)
        add("fuzz", "f" + std::to_string(f), [](Case& c) {
            c.init(1);
            ProgramBuilder& pb = c.pb();
            Rng& g = c.rng;
            auto len = [&]() { return g.u(4) == 0 ? kL[g.u(kNL - 1)] : g.in(1, 3073); };
            auto cnt = [&]() { return g.u(3) == 0 ? kC[g.u(kNC)] : g.in(1, 129); };
            struct Made { RowId row; uint32_t len, level; };
            std::vector<Made> made;  // rows earlier ops wrote
            const uint32_t nops = g.in(2, 12);
            while (pb.ops().size() < nops) {
                const uint32_t L = len(), st = units_of(L) + (g.u(3) == 0 ? g.u(5) : 0);
                // sources of an earlier level (at most level 2, so the program stays within 3 levels)
                std::vector<Made> from;
                if (!made.empty() && g.u(2))
                    for (uint32_t q = 0; q < 2; ++q) {
                        const Made& m = made[g.u((uint32_t)made.size())];
                        if (m.level <= 2) from.push_back(m);
                    }
                auto old_terms = [&](uint32_t maxacc) {
                    for (const Made& m : from) pb.op_acc(m.row, g.coef(), std::min(m.len, L), g.u(maxacc + 1));
                };
                const RowId dst = c.alloc(L + 8 + (g.u(4) == 0 ? 64 * g.u(40) : 0));
                const uint32_t flen = g.u(9);
                uint32_t level = 0;
                uint32_t what = g.u(7);
                if (what == 5 && pb.ops().size() + 8 > 12) what = 6;  // (a split range is up to 5 + 3 ops)
                switch (what) {
                case 0: {  // plain: ACCs into the three accumulators, stores, maybe a CLEAR
                    pb.begin_op();
                    const uint32_t n = g.in(1, 13);
                    bool used[3] = {true, false, false};
                    pb.op_acc(c.alloc(L), g.coef(), L, 0);
                    for (uint32_t i = 0; i < n; ++i) {
                        const uint32_t l = g.u(3) ? L : g.in(1, L), a = g.u(3);
                        pb.op_acc(c.alloc(l), g.u(3) ? g.coef() : 1, l, a);
                        used[a] = true;
                    }
                    old_terms(0);
                    if (g.u(3) == 0) {  // every accumulator in use is stored, then all restart from zero
                        for (uint32_t a = 0; a < 3; ++a)
                            if (used[a]) pb.op_store(c.alloc(L + 8), L, a, c.footer(), g.u(9));
                        op_clear(pb);
                        used[1] = used[2] = false;
                        pb.op_acc(c.alloc(L), g.coef(), L, 0);
                    }
                    for (uint32_t a = 1; a < 3; ++a)
                        if (used[a]) pb.op_store(c.alloc(L + 8), L, a, c.footer(), g.u(9));
                    pb.op_store(dst, L, 0, c.footer(), flen);
                    level = pb.end_op();
                    break;
                }
                case 1: {  // a pure combine of rows and runs
                    std::vector<Term> t;
                    for (uint32_t i = g.u(6); i > 0; --i) t.push_back(Term{c.alloc(L), g.u(4) ? L : g.in(1, L), g.coef()});
                    for (const Made& m : from) t.push_back(Term{m.row, std::min(m.len, L), g.coef()});
                    for (uint32_t i = g.in(1, 3); i > 0; --i) {
                        const uint32_t C = cnt(), mode = g.u(3);
                        if (mode == 2) {
                            std::vector<uint32_t> keys;
                            for (uint32_t q = g.u(6); q > 0; --q) keys.push_back((50 + g.u(C)) << 8 | g.nz());
                            std::sort(keys.begin(), keys.end());
                            t.push_back(pb.dense_run_term(c.region(C, st, L), st, C, g.u(1u << 22), rnd_ops(g), (uint8_t)g.u(256),
                                                          keys.data(), (uint32_t)keys.size(), 50, L));
                        } else {
                            t.push_back(pb.run_term(mode ? TAMD_R_CAUCHY : TAMD_R_CONST, mode ? g.u(192) : g.nz(), c.region(C, st, L), st, C,
                                                    g.u(1u << 22), L));
                        }
                        t.back().coef = g.u(2) ? 1 : g.coef();
                    }
                    level = pb.combine(dst, t.data(), t.size(), L, c.footer(), flen);
                    break;
                }
                case 2: {  // lanes: ACC3 / LANE3, STORECs
                    pb.begin_op();
                    for (uint32_t i = g.u(4); i > 0; --i) pb.op_acc3_off(c.off(c.alloc(L)), g.coef(), g.coef(), L);
                    const uint32_t C = cnt(), cstep = g.u(2) ? 8 : 1;
                    pb.op_accr(TAMD_R_LANE3, 0, c.region(C, st, L), st, C, L, g.u(TAMD_COLUMN_PERIOD - 129 * 8), cstep);
                    old_terms(2);
                    for (uint32_t i = g.in(1, 3); i > 1; --i) {
                        uint8_t cc[3] = {(uint8_t)(g.u(3) ? g.coef() : 1), (uint8_t)(g.u(3) ? g.coef() : 0), (uint8_t)g.u(256)};
                        pb.op_storec(c.alloc(L), L, cc);
                    }
                    uint8_t cc[3] = {g.coef(), g.coef(), 1};
                    pb.op_storec(dst, L, cc);
                    level = pb.end_op();
                    break;
                }
                case 3: {  // MULTI
                    pb.begin_op();
                    const uint32_t C = cnt();
                    uint32_t t[3] = {0, 0, 0};
                    for (uint32_t a = 0, n = g.in(1, 3); a < n; ++a) {
                        const uint32_t lo = g.u(C), hi = g.in(lo + 1, C);
                        t[a] = tword(g.u(2) ? TAMD_R_CAUCHY : TAMD_R_CONST, g.u(192), lo, hi);
                    }
                    pb.op_accr_multi(c.region(C, st, L), st, C, L, g.u(1u << 22), 1, t);
                    old_terms(0);
                    for (uint32_t a = 1; a < 3; ++a)
                        if (t[a]) pb.op_store(c.alloc(L + 8), L, a, c.footer(), g.u(9));
                    pb.op_store(dst, L, 0, c.footer(), flen);
                    level = pb.end_op();
                    break;
                }
                case 4: {  // single-target DENSE with ADJ words and a scale
                    pb.begin_op();
                    const uint32_t C = cnt();
                    std::vector<uint32_t> adj;
                    for (uint32_t q = g.u(10); q > 0; --q) adj.push_back(g.u(C) << 16 | (uint32_t)g.nz() << 8);
                    std::sort(adj.begin(), adj.end());
                    pb.op_accr_dense(c.region(C, st, L), st, C, L, g.u(1u << 22), rnd_ops(g), (uint8_t)g.u(256), adj.data(),
                                     (uint32_t)adj.size(), g.u(2) ? 1 : g.coef());
                    old_terms(0);
                    pb.op_store(dst, L, 0, c.footer(), flen);
                    level = pb.end_op();
                    break;
                }
                case 5: {  // multi-target DENSE range
                    uint32_t hi[3];
                    const uint32_t n = g.in(2, 3);
                    hi[0] = g.in(1, 60);
                    for (uint32_t a = 1; a < n; ++a) hi[a] = std::min(129u, hi[a - 1] + g.u(50));
                    dense_range(c, n, hi, L, g.in(1, 2), g.u(3) ? 0 : g.in(32, 64), g.u(1u << 22), g.u(9));
                    level = 1;
                    continue;  // (its rows are not read again: their level depends on the split)
                }
                default: {  // CONST / CAUCHY runs raw, ending in op_store
                    pb.begin_op();
                    const uint32_t C = cnt();
                    if (g.u(2)) pb.op_accr(TAMD_R_CONST, g.nz(), c.region(C, st, L), st, C, L, g.u(1u << 22), 1);
                    else pb.op_accr(TAMD_R_CAUCHY, g.u(192), c.region(C, st, L), st, C, L, g.u(1u << 22), 1);
                    old_terms(0);
                    pb.op_store(dst, L, 0, c.footer(), flen);
                    level = pb.end_op();
                    break;
                }
                }
                made.push_back(Made{dst, L, level});
            }
        });
}

// ---------------------------------------------------------------------------------------------
// The interpreter over a case's image: level by level, contexts in order within a level (the
// merged launch runs one level of every context at a time).
// ---------------------------------------------------------------------------------------------
static int interpret(const std::vector<Prog>& progs, std::vector<uint8_t>& img) {
    uint32_t maxl = 0;
    for (const Prog& p : progs)
        for (uint32_t b : p.bucket) maxl = std::max(maxl, b / TAMD_COST_CLASSES);
    for (uint32_t l = 1; l <= maxl; ++l)
        for (const Prog& p : progs) {
            std::vector<uint32_t> sorted;
            for (size_t i = 0; i < p.ops.size(); ++i)
                if (p.bucket[i] / TAMD_COST_CLASSES == l) {
                    const tamd_op& o = p.ops[i];
                    sorted.push_back(o.first), sorted.push_back(o.count), sorted.push_back(o.span), sorted.push_back(o.full);
                }
            if (sorted.empty()) continue;
            const int rc = oracle_run_program(img.data(), img.size(), sorted.data(), (unsigned)(sorted.size() / 4),
                                              (const uint32_t*)p.in.data(), (unsigned)p.in.size());
            if (rc) return rc;
        }
    return 0;
}
static uint64_t digest(const std::vector<uint8_t>& v) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i + 8 <= v.size(); i += 8) {
        uint64_t w;
        memcpy(&w, &v[i], 8);
        h = (h ^ w) * 1099511628211ull;
        h ^= h >> 29;
    }
    return h;
}
static bool has_multi_dense(const std::vector<Prog>& progs) {
    for (const Prog& p : progs)
        for (const tamd_instr& w : p.in)
            if (kind_of(w) == TAMD_I_ACCR && ((w.w0 >> 8) & 0xffu) == TAMD_R_DENSE && ((w.w0 >> 16) & 0xffu) > 1) return true;
    return false;
}

// Which in-batch positions an ACCR cuts a batch at, and how many STOREs are a batch's last word
// with their FOOTER in the next one, for instruction batches of B words (run_item's walk).
static void batch_walk(const Prog& p, uint32_t B, uint32_t& cut, uint32_t& split) {
    for (const tamd_op& op : p.ops) {
        const uint32_t end = op.first + op.count;
        for (uint32_t k = op.first; k < end;) {
            uint32_t nb = std::min(B, end - k);
            for (uint32_t j = B; j-- > 0;)
                if (j < nb && kind_of(p.in[k + j]) == TAMD_I_ACCR) nb = j;
            cut |= nb < std::min(B, end - k) ? 1u << nb : 0u;
            if (nb == 0) {
                Run r;
                if (!parse_run(p.in, k, end, r).empty()) return;
                k += r.words;
                continue;
            }
            if (nb == B && kind_of(p.in[k + nb - 1]) == TAMD_I_STORE) ++split;
            k += nb;
        }
    }
}

static void print_reach(Case& c, const std::vector<Prog>& progs, uint64_t dig) {
    printf("{\"name\":\"%s\",\"group\":\"%s\",\"seed\":%llu,\"nctx\":%d,\"slice\":%u,\"digest\":\"%016llx\",\"multi_dense\":%s,",
           c.name.c_str(), c.group.c_str(), (unsigned long long)c.seed, c.nctx, slice_bytes(), (unsigned long long)dig,
           has_multi_dense(progs) ? "true" : "false");
    uint32_t adj = 0, targets = 0, stores = 0, kinds[16] = {0}, cut5 = 0, cut6 = 0, split5 = 0, split6 = 0;
    std::vector<uint32_t> level_items;
    std::string ops = "[", runs = "[";
    char buf[160];
    for (const Prog& p : progs) {
        batch_walk(p, 5, cut5, split5);
        batch_walk(p, 6, cut6, split6);
        for (size_t o = 0; o < p.ops.size(); ++o) {
            const tamd_op& op = p.ops[o];
            const uint32_t lvl = p.bucket[o] / TAMD_COST_CLASSES, sl = op_slices(op.span);
            if (level_items.size() <= lvl) level_items.resize(lvl + 1, 0);
            level_items[lvl] += sl;
            snprintf(buf, sizeof buf, "%s{\"span\":%u,\"full\":%u,\"slices\":%u,\"level\":%u,\"cls\":%u,\"pure\":%u,\"words\":%u}",
                     ops.size() > 1 ? "," : "", op.span, op.full, sl, lvl, p.bucket[o] % TAMD_COST_CLASSES, p.pure[o], op.count);
            ops += buf;
            for (uint32_t k = op.first; k < op.first + op.count;) {
                const uint32_t kind = kind_of(p.in[k]);
                kinds[kind & 15u]++;
                if (kind == TAMD_I_STORE || kind == TAMD_I_STOREC) ++stores;
                if (kind != TAMD_I_ACCR) {
                    ++k;
                    continue;
                }
                Run r;
                parse_run(p.in, k, op.first + op.count, r);
                uint32_t nt = r.nt, words = r.nadj[0] + r.nadj[1] + r.nadj[2];
                if (r.mode == TAMD_R_MULTI) {
                    nt = 0;
                    for (unsigned q = 0; q < 3; ++q) nt += (&p.in[r.targets].row)[q] != 0;
                }
                adj += words;
                targets += nt;
                snprintf(buf, sizeof buf, "%s{\"mode\":%u,\"p\":%u,\"scale\":%u,\"count\":%u,\"len\":%u,\"stride\":%u,\"cstep\":%u,\"targets\":%u,\"adj\":%u}",
                         runs.size() > 1 ? "," : "", r.mode, r.p, r.scale, r.count, r.len, r.stride, r.cstep, nt, words);
                runs += buf;
                k += r.words;
            }
        }
    }
    printf("\"ops\":%s],\"runs\":%s],\"adj_words\":%u,\"targets\":%u,\"stores\":%u,", ops.c_str(), runs.c_str(), adj, targets, stores);
    printf("\"acc3\":%u,\"storec\":%u,\"clear\":%u,\"cut5\":%u,\"cut6\":%u,\"split5\":%u,\"split6\":%u,\"level_items\":[",
           kinds[TAMD_I_ACC3], kinds[TAMD_I_STOREC], kinds[TAMD_I_CLEAR], cut5, cut6, split5, split6);
    for (size_t l = 1; l < level_items.size(); ++l) printf("%s%u", l > 1 ? "," : "", level_items[l]);
    printf("]}\n");
}

// ---------------------------------------------------------------------------------------------
// Mutations: one semantic change at a time; the interpreter's image must change
// ---------------------------------------------------------------------------------------------
enum { F_STORE_LEN = 1, F_FOOTER = 2, F_COEF = 4, F_COUNT = 8, F_HI = 16, F_ADJ = 32, F_RX = 64, F_SCALE = 128 };
static const char* const kFeat[] = {"store_len", "footer", "coef", "count", "hi", "adj", "rx", "scale"};
struct Site { uint32_t feat, prog, word, field, xorv, sub; };  // field: 0 w0, 1 row, 2 len, 3 cap; sub: subtract 1 from bits at shift
// Row e's coefficient for target t of a DENSE run (program.h), scale apart: a row whose coefficient
// is zero adds nothing, so dropping it (count - 1, hi - 1) is no semantic change.
static uint8_t dense_coef(const Prog& p, const Run& r, uint32_t t, uint32_t e, bool* uses_rx = nullptr) {
    const tamd_instr& cw = p.in[r.coefs[t]];
    const uint64_t ow = (uint64_t)cw.row | ((uint64_t)(cw.len & 0xffffu) << 32);
    const uint32_t col = (uint32_t)(((uint64_t)r.col0 + (uint64_t)e * r.cstep) % TAMD_COLUMN_PERIOD);
    const uint32_t b = (uint32_t)(ow >> (6u * (col % 8u))) & 63u;
    const uint8_t cx = oracle_column_value(col), cx2 = oracle_gf_sqr(cx), rx = (uint8_t)(cw.len >> 16);
    const uint8_t sd = (uint8_t)((b & 1u) ^ ((b & 2u) ? cx : 0u) ^ ((b & 4u) ? cx2 : 0u));
    const uint8_t tp = (uint8_t)(((b >> 3) & 1u) ^ ((b & 16u) ? cx : 0u) ^ ((b & 32u) ? cx2 : 0u));
    if (uses_rx) *uses_rx = tp != 0;
    uint8_t g = (uint8_t)(sd ^ oracle_gf_mul(rx, tp));
    for (uint32_t q = 0; q < 4 * r.nadj[t]; ++q) {
        const uint32_t d = adj_entry(p.in, r.coefs[t] + 1, q);
        if ((d >> 16) == e) g ^= (uint8_t)(d >> 8);
    }
    return g;
}

// (`done`: the interpreter's image of the unchanged program.  A store without a footer that loses
// its last byte writes a zero there instead: a change only where that byte is not zero already.)
static void sites_of(const std::vector<Prog>& progs, const std::vector<uint8_t>& done, std::vector<Site>& out) {
    for (uint32_t pi = 0; pi < progs.size(); ++pi) {
        const Prog& p = progs[pi];
        for (const tamd_op& op : p.ops) {
            const uint32_t end = op.first + op.count;
            for (uint32_t k = op.first; k < end;) {
                const tamd_instr& w = p.in[k];
                const uint32_t kind = kind_of(w);
                if (kind == TAMD_I_STORE) {
                    if (w.len && (((w.w0 >> 8) & 0xffu) || done[(size_t)w.row * 64 + w.len - 1]))
                        out.push_back(Site{F_STORE_LEN, pi, k, 2, 0, 1});
                    if ((w.w0 >> 8) & 0xffu) out.push_back(Site{F_FOOTER, pi, k + 1, 1, 0x40, 0});  // footer byte 0
                    k += 2;
                } else if (kind == TAMD_I_STOREC) {
                    if (w.len && done[(size_t)w.row * 64 + w.len - 1]) out.push_back(Site{F_STORE_LEN, pi, k, 2, 0, 1});
                    out.push_back(Site{F_COEF, pi, k, 0, 1u << 8, 0});
                    ++k;
                } else if (kind == TAMD_I_ACC || kind == TAMD_I_ACC3) {
                    out.push_back(Site{F_COEF, pi, k, 0, 1u << 8, 0});
                    ++k;
                } else if (kind == TAMD_I_ACCR) {
                    Run r;
                    parse_run(p.in, k, end, r);
                    // the run's last row counts unless nothing takes it: no MULTI window ends there, or
                    // its DENSE coefficient is zero
                    bool last_counts = true;
                    if (r.mode == TAMD_R_MULTI) {
                        last_counts = false;
                        for (uint32_t q = 0; q < 3; ++q) {
                            const uint32_t t = (&p.in[r.targets].row)[q];
                            if ((t >> 21) == r.count && ((t >> 10) & 0x7ffu) < r.count) last_counts = true;
                        }
                    }
                    if (r.mode == TAMD_R_DENSE) {
                        last_counts = false;
                        for (uint32_t t = 0; t < r.nt; ++t)
                            if (r.hi[t] == r.count && dense_coef(p, r, t, r.count - 1)) last_counts = true;
                    }
                    if (last_counts) out.push_back(Site{F_COUNT, pi, k, 3, 0, 1});
                    if (r.mode == TAMD_R_CONST || r.mode == TAMD_R_CAUCHY) out.push_back(Site{F_COEF, pi, k, 0, 1u << 16, 0});
                    if (r.scale > 1) out.push_back(Site{F_SCALE, pi, k, 0, 1u << 24, 0});
                    if (r.mode == TAMD_R_MULTI)
                        for (uint32_t q = 0; q < 3; ++q) {
                            const uint32_t t = (&p.in[r.targets].row)[q];
                            if ((t >> 21) > ((t >> 10) & 0x7ffu)) out.push_back(Site{F_HI, pi, r.targets, 1 + q, 0, 1u << 21});
                            if ((t & 3u) == TAMD_R_CAUCHY && (t >> 21) > ((t >> 10) & 0x7ffu))
                                out.push_back(Site{F_COEF, pi, r.targets, 1 + q, 1u << 2, 0});
                        }
                    if (r.mode == TAMD_R_DENSE)
                        for (uint32_t t = 0; t < r.nt; ++t) {
                            bool rx_used = false;  // (some row of the range takes the rx product)
                            for (uint32_t e = 0; e < r.hi[t] && !rx_used; ++e) dense_coef(p, r, t, e, &rx_used);
                            if (rx_used) out.push_back(Site{F_RX, pi, r.coefs[t], 2, 1u << 16, 0});
                            if (r.nt > 1 && r.hi[t] && dense_coef(p, r, t, r.hi[t] - 1))
                                out.push_back(Site{F_HI, pi, r.coefs[t], 3, 0, 1u << 16});
                            for (uint32_t q = 0; q < 4 * r.nadj[t]; ++q) {
                                const uint32_t d = adj_entry(p.in, r.coefs[t] + 1, q);
                                if ((d & 0xff00u) && (d >> 16) < r.hi[t])
                                    out.push_back(Site{F_ADJ, pi, r.coefs[t] + 1 + q / 4, q & 3u, 1u << 8, 0});
                            }
                        }
                    k += r.words;
                } else {
                    ++k;
                }
            }
        }
    }
}
static void apply(std::vector<Prog>& progs, const Site& s) {
    uint32_t* f = &progs[s.prog].in[s.word].w0 + s.field;
    if (s.sub) *f -= s.sub;
    else *f ^= s.xorv;
}

// ---------------------------------------------------------------------------------------------
// Modes
// ---------------------------------------------------------------------------------------------
static bool pick(const Spec& s, const std::string& only) { return only.empty() || s.name.find(only) != std::string::npos; }

static int mode_cpu(const std::vector<Spec>& specs, const std::string& only, bool list) {
    int bad = 0;
    for (const Spec& s : specs) {
        if (!pick(s, only)) continue;
        std::unique_ptr<Case> c = build_case(s);
        std::vector<Prog> progs = c->progs();
        if (list) {
            printf("{\"name\":\"%s\",\"group\":\"%s\",\"nctx\":%d,\"multi_dense\":%s}\n", c->name.c_str(), c->group.c_str(), c->nctx,
                   has_multi_dense(progs) ? "true" : "false");
            continue;
        }
        const std::string e = validate_program(progs.data(), progs.size(), c->rows);
        std::vector<uint8_t> img = c->image;
        const int rc = e.empty() ? interpret(progs, img) : -100;
        if (!e.empty() || rc) {
            printf("{\"name\":\"%s\",\"group\":\"%s\",\"error\":\"%s\",\"rc\":%d}\n", c->name.c_str(), c->group.c_str(), e.c_str(), rc);
            ++bad;
            continue;
        }
        // guards stay as they were in the expected image too (an interpreter that strays is a bug)
        for (const RowInfo& r : c->rows)
            if (r.guard && memcmp(&img[(size_t)r.off * 64], &c->image[(size_t)r.off * 64], 64)) {
                printf("{\"name\":\"%s\",\"group\":\"%s\",\"error\":\"the interpreter wrote a guard row\",\"rc\":0}\n", c->name.c_str(),
                       c->group.c_str());
                ++bad;
            }
        print_reach(*c, progs, digest(img));
    }
    return bad ? 1 : 0;
}

static int mode_mutate(const std::vector<Spec>& specs, const std::string& only) {
    int bad = 0;
    for (const Spec& s : specs) {
        if (!pick(s, only)) continue;
        std::unique_ptr<Case> c = build_case(s);
        const std::vector<Prog> progs = c->progs();
        std::vector<uint8_t> base = c->image;
        if (interpret(progs, base)) die("case " + c->name + " does not run");
        const uint64_t want = digest(base);
        std::vector<Site> sites;
        sites_of(progs, base, sites);
        uint32_t tried[8] = {0}, dead[8] = {0};
        std::string first_dead;
        for (unsigned f = 0; f < 8; ++f) {
            if (c->unclaim & (1u << f)) continue;
            std::vector<const Site*> mine;
            for (const Site& st : sites)
                if (st.feat == (1u << f)) mine.push_back(&st);
            // (the first and the last four sites of a feature: long cases stay quick)
            for (size_t i = 0; i < mine.size(); ++i) {
                if (i >= 4 && i + 4 < mine.size()) continue;
                std::vector<Prog> m = progs;
                apply(m, *mine[i]);
                std::vector<uint8_t> img = c->image;
                const int rc = interpret(m, img);
                ++tried[f];
                if (rc || digest(img) == want) {
                    ++dead[f];
                    if (first_dead.empty())
                        first_dead = std::string(kFeat[f]) + " at word " + std::to_string(mine[i]->word) + (rc ? " (rc)" : "");
                }
            }
        }
        bool ok = true;
        printf("{\"name\":\"%s\",\"group\":\"%s\",\"tried\":{", c->name.c_str(), c->group.c_str());
        for (unsigned f = 0; f < 8; ++f) {
            printf("%s\"%s\":%u", f ? "," : "", kFeat[f], tried[f]);
            if (dead[f]) ok = false;
        }
        printf("},\"ok\":%s,\"insensitive\":\"%s\"}\n", ok ? "true" : "false", first_dead.c_str());
        bad += !ok;
    }
    return bad ? 1 : 0;
}

// validate_program must refuse one hand-made violation of every precondition.
static int mode_reject() {
    Case c;
    c.name = "reject", c.seed = 7, c.rng = Rng(7);
    c.init(1);
    ProgramBuilder& pb = c.pb();
    const uint32_t L = 300, st = units_of(L), C = 10;
    // op 0: a LANE3 run, op 1: MULTI, op 2: DENSE with ADJ, op 3: ACC + STORE, op 4 (level 2) reads op 3's row
    pb.begin_op();
    pb.op_accr(TAMD_R_LANE3, 0, c.region(C, st, L), st, C, L, TAMD_COLUMN_PERIOD - C, 1);
    uint8_t one[3] = {1, 1, 1};
    pb.op_storec(c.alloc(L), L, one);
    pb.end_op();
    const uint32_t t[3] = {tword(TAMD_R_CAUCHY, 3, 2, C), tword(TAMD_R_CONST, 0, 0, 5), 0};
    pb.begin_op();
    pb.op_accr_multi(c.region(C, st, L), st, C, L, 0, 1, t);
    pb.op_store(c.alloc(L + 8), L, 0, c.footer(), 2);
    pb.end_op();
    const uint32_t adj[5] = {1u << 16 | 5u << 8, 3u << 16 | 6u << 8, 3u << 16 | 7u << 8, 8u << 16 | 9u << 8, 9u << 16 | 1u << 8};
    pb.begin_op();
    pb.op_accr_dense(c.region(C, st, L), st, C, L, 0, 0x123456789abcull, 5, adj, 5, 1);
    pb.op_store(c.alloc(L + 8), L, 0, c.footer(), 2);
    pb.end_op();
    const RowId src = c.alloc(L), mid = c.alloc(L + 8);
    pb.begin_op();
    pb.op_acc(src, 3, L);
    pb.op_store(mid, L, 0, c.footer(), 2);
    pb.end_op();
    pb.begin_op();
    pb.op_acc(mid, 1, L);
    pb.op_store(c.alloc(L + 8), L, 0, c.footer(), 0);
    pb.end_op();
    const uint32_t hi[3] = {4, 7, 10};
    dense_range(c, 3, hi, L, 1, 0, 100, 3);
    c.finish();
    const Prog good = prog_of(pb);
    int bad = 0;
    auto check = [&](const char* rule, const Prog& p, bool want_reject) {
        const std::string e = validate_program(&p, 1, c.rows);
        const bool ok = e.empty() != want_reject;
        printf("{\"rule\":\"%s\",\"rejected\":%s,\"ok\":%s,\"message\":\"%s\"}\n", rule, e.empty() ? "false" : "true",
               ok ? "true" : "false", e.c_str());
        bad += !ok;
    };
    check("unchanged", good, false);
    auto word_of = [&](size_t op, uint32_t kind, uint32_t nth = 0) -> uint32_t {
        for (uint32_t k = good.ops[op].first; k < good.ops[op].first + good.ops[op].count; ++k)
            if (kind_of(good.in[k]) == kind && nth-- == 0) return k;
        die("reject: word not found");
        return 0;
    };
    const size_t dm = good.ops.size() - 1;  // the multi-target DENSE op
    Prog p;
    p = good, p.in[word_of(0, TAMD_I_ACCR)].cap = 0, check("run count >= 1", p, true);
    p = good, p.in[word_of(0, TAMD_I_ACCR)].len = 0, check("run len >= 1", p, true);
    p = good, p.in[word_of(0, TAMD_I_RANGE)].len += 1, check("LANE3 within the column period", p, true);
    p = good, p.in[word_of(1, TAMD_I_TARGETS)].row = tword(TAMD_R_CAUCHY, 3, 2, C + 1), check("MULTI hi <= count", p, true);
    p = good, p.in[word_of(1, TAMD_I_TARGETS)].len = tword(TAMD_R_CONST, 0, 6, 5), check("MULTI lo <= hi", p, true);
    p = good, p.in[word_of(1, TAMD_I_TARGETS)].row = tword(TAMD_R_CAUCHY, 192, 2, C), check("CAUCHY row < 192", p, true);
    p = good, std::swap(p.in[word_of(2, TAMD_I_ADJ)].row, p.in[word_of(2, TAMD_I_ADJ)].cap), check("ADJ ascending", p, true);
    p = good, p.in[word_of(2, TAMD_I_ADJ)].len = 0, check("ADJ empty entries last", p, true);
    p = good, p.in[word_of(dm, TAMD_I_COEFS, 0)].cap += 5u << 16, check("DENSE ranges nested", p, true);
    p = good, p.in[word_of(dm, TAMD_I_COEFS, 2)].cap += 1u << 16, check("DENSE hi <= count", p, true);
    p = good, p.in[word_of(3, TAMD_I_ACC)].len = 64 * units_of(L) + 1, p.ops[3].span = 1024, check("reads inside an allocated row", p, true);
    p = good, p.in[word_of(3, TAMD_I_ACC)].row += units_of(L), check("no read of a guard row", p, true);
    p = good, p.in[word_of(0, TAMD_I_ACCR)].cap = C + 1, check("run rows inside an allocated row", p, true);
    p = good, p.in[word_of(3, TAMD_I_STORE)].cap = 64 * units_of(L + 8) + 64, p.ops[3].span = 1024, check("stores inside an allocated row", p, true);
    p = good, p.in[word_of(3, TAMD_I_STORE)].cap -= 4, check("cap a multiple of 8", p, true);
    p = good, p.bucket[4] = p.bucket[3], check("no read of a row written in the same level", p, true);
    p = good, p.in[word_of(4, TAMD_I_STORE)].row = p.in[word_of(3, TAMD_I_STORE)].row, p.bucket[4] = p.bucket[3],
    p.in[word_of(4, TAMD_I_ACC)].row = p.in[word_of(3, TAMD_I_ACC)].row, check("no two writers of a row in one level", p, true);
    p = good, p.in[word_of(3, TAMD_I_ACC)].len = L - 1, check("full <= every length", p, true);
    return bad ? 1 : 0;
}

struct Diff { bool ok; uint64_t off; long row; uint32_t byte, want, got; };
static Diff compare(const Case& c, const std::vector<uint8_t>& want, const std::vector<uint8_t>& got) {
    Diff d{true, 0, -1, 0, 0, 0};
    for (size_t i = 0; i < want.size(); ++i)
        if (want[i] != got[i]) {
            d.ok = false, d.off = i, d.want = want[i], d.got = got[i];
            for (size_t r = 0; r < c.rows.size(); ++r)
                if (i >= (size_t)c.rows[r].off * 64 && i < ((size_t)c.rows[r].off + c.rows[r].units) * 64)
                    d.row = (long)r, d.byte = (uint32_t)(i - (size_t)c.rows[r].off * 64);
            break;
        }
    return d;
}
static void print_result(const Case& c, const char* state, const Diff& d) {
    printf("{\"name\":\"%s\",\"group\":\"%s\",\"state\":\"%s\",\"ok\":%s,\"first_bad_offset\":%lld,\"row\":%ld,\"byte_in_row\":%u,"
           "\"want\":%u,\"got\":%u}\n",
           c.name.c_str(), c.group.c_str(), state, d.ok ? "true" : "false", d.ok ? -1ll : (long long)d.off, d.row, d.byte, d.want, d.got);
    fflush(stdout);
}

static int mode_gpu(const std::vector<Spec>& specs, const std::string& only, bool serve) {
    Device dev;
    if (!dev.init(0, kArena)) die("no device: " + dev.error());
    Server srv;
    if (serve && !srv.init(dev, 4, 64, 50)) die("the persistent executor did not start");
    int bad = 0;
    auto hip_error = [&](const Case& c, const char* what) {
        fflush(stdout);
        fprintf(stderr, "exec_check: HIP error in case %s (%s): %s\n", c.name.c_str(), what, dev.error().c_str());
        // (no further GPU work: not even the server's stop command)
        _exit(3);
    };
    for (const Spec& s : specs) {
        if (!pick(s, only)) continue;
        std::unique_ptr<Case> c = build_case(s);
        if (serve && c->nctx > 1) continue;
        const std::vector<Prog> progs = c->progs();
        const std::string e = validate_program(progs.data(), progs.size(), c->rows);
        if (!e.empty()) die("case " + c->name + " is malformed (" + e + "): not run");
        std::vector<uint8_t> want = c->image, got(kArena);
        if (interpret(progs, want)) die("case " + c->name + " does not run on the interpreter");
        fprintf(stderr, "case %s\n", c->name.c_str());
        dev.upload(0, c->image.data(), kArena);
        dev.synchronize();
        if (dev.failed()) hip_error(*c, "upload");
        if (serve) {
            CmdBuf b;
            const std::vector<Device::HostCopy> none;
            c->ctx[0]->prepare_flush();
            if (!Server::build(b, none, &c->ctx[0]->pb, none)) {
                c->ctx[0]->finish_flush();
                print_result(*c, "declined", Diff{true, 0, -1, 0, 0, 0});
                continue;
            }
            srv.post(b);
            c->ctx[0]->finish_flush();
            if (!srv.wait(b)) {
                fflush(stdout);
                fprintf(stderr, "exec_check: case %s: the persistent executor did not complete the command\n", c->name.c_str());
                _exit(3);
            }
            dev.download_now(got.data(), 0, kArena);
            b.release();
        } else {
            Context* ctxs[2] = {c->ctx[0].get(), c->nctx > 1 ? c->ctx[1].get() : nullptr};
            for (int i = 0; i < c->nctx; ++i) ctxs[i]->prepare_flush();
            const uint64_t ticket = dev.run(ctxs, (size_t)c->nctx);
            for (int i = 0; i < c->nctx; ++i) ctxs[i]->finish_flush();
            dev.wait(ticket);
            if (dev.failed()) hip_error(*c, "run");
            dev.download(got.data(), 0, kArena);
        }
        if (dev.failed()) hip_error(*c, "download");
        const Diff d = compare(*c, want, got);
        print_result(*c, "run", d);
        bad += !d.ok;
    }
    if (serve) srv.stop();
    dev.synchronize();
    if (dev.failed()) {
        fprintf(stderr, "exec_check: HIP error at the end: %s\n", dev.error().c_str());
        return 3;
    }
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) die("usage: exec_check list|cpu|mutate|reject|launch|serve [only=<name part>]");
    const std::string mode = argv[1];
    std::string only;
    for (int i = 2; i < argc; ++i)
        if (!strncmp(argv[i], "only=", 5)) only = argv[i] + 5;
    if (oracle_gf_init()) die("oracle self test failed");
    if (!gf_init()) die("host field tables failed");  // (combine() folds coefficients with them)
    std::vector<Spec> specs;
    add_cases(specs);
    if (mode == "list") return mode_cpu(specs, only, true);
    if (mode == "cpu") return mode_cpu(specs, only, false);
    if (mode == "mutate") return mode_mutate(specs, only);
    if (mode == "reject") return mode_reject();
    if (mode == "launch") return mode_gpu(specs, only, false);
    if (mode == "serve") return mode_gpu(specs, only, true);
    die("unknown mode " + mode);
    return 2;
}
