// unlz_check.cpp -- TEST ONLY.  The block reader the decompression kernel uses
// (tonk_amd/csrc/unlz.h alone) on the host: as a serial walk (one "lane") and on 64 emulated
// lanes, against the reference's zstd (oracle/_ref/libmsgcodec_ref.so: MessageCompressor /
// MessageDecompressor restated).
//
//   unlz_check check <streams> [<rewrites out>]
//       every message of every stream is compressed by the reference and restored by the walk
//       (uncompressed ones inserted); bytes must equal the message and the reference
//       decompressor's.  Then the Repeat rewrites, the hand-made blocks and the GPU compressor's
//       format (lz.h's host block writer under a greedy parse).  Prints how often each path of
//       the reader ran; all must be nonzero.  <rewrites out>: the rewrite streams as blocks.
//   unlz_check mutants <streams> [<cases out>]
//       malformed blocks: every truncation and 2,000 seeded bit flips of three valid blocks, an
//       offset too far and an output capacity too small; ring, input and output are allocated
//       exactly (run it under -fsanitize=address,undefined).  Whatever the walk accepts the
//       reference must accept with the same bytes.  <cases out>: 64 chosen cases with the
//       walk's verdicts.
//   unlz_check bench <streams> <threads> <reps>
//       the reference decompressor on host threads, over the blocks of the file (or, for a file
//       of raw messages, over the reference compressor's blocks of them): decoding alone is
//       timed, the median repetition is reported.
//   unlz_check tables
//       the decode-table build's phases for 64 lanes against the state-by-state build.
//   unlz_check ring
//       the compressor's form of the history-ring rule (lz.h RingTrack) and the decoder's
//       (tamd_unlz_place) side by side: 10 maximum sizes x 200 seeded streams x 400 lengths.
//   unlz_check directed <cases out>
//       blocks written from chosen parses (lz_host.h lz_host_write), aimed at the boundaries of
//       the reader's lane code: the chunk of 64 sequences, the waits for bytes just written, the
//       lane count as a match's period and length, matches into and across the previous ring
//       segment, block and literal sizes around 256 and 1536.  Every block goes through the walk
//       and the reference decompressor; both must restore the message.  Prints one JSON record
//       per group (the reader's path counters and facts); <cases out>: the corpus with verdicts.
//   unlz_check lanes <streams> [blocks=<file>] [cases=<file>] [skip=<function>:<line>]
//       the reader as the kernel runs it: 64 lanes as fibres, each calling unlz.h with
//       (lane, 64) inside the kernel's message loop restated, TAMD_UNLZ_SYNC() = wait until every
//       lane has arrived.  Between two syncs one lane at a time runs its phase to the end, in
//       three orders (ascending, descending, a seeded shuffle redrawn at every sync).  Restored
//       bytes, status, repeat offsets and ring bookkeeping after every message must equal the
//       walk's (and the reference's bytes).  Inputs: the reference's blocks of <streams>, block
//       files without verdicts (check's rewrites) and case files with them (directed).  skip=:
//       all lanes run through that one sync site without waiting.
//   unlz_check sens <streams> [blocks=<file>] [cases=<file>]
//       for every sync site the lanes reach (over the block files, the case files and the first
//       messages of every stream): does skipping it change any output under any order?
//   unlz_check reach <streams> [blocks=<file>] [cases=<file>]
//       the walk over the same kinds of input; prints how often each path and each outcome of a
//       wait ran (which paths a set of inputs reaches, e.g. the device's).
//
// Stream files: "UNLZ", u32 streams; per stream u32 max, u32 messages; per message u32 is_block,
// u32 bytes, the bytes.  Case files add per message i32 status, u32 restored, the restored bytes.
static unsigned long long g_cnt[64];
#define TAMD_UNLZ_COUNT(what) (++g_cnt[what])
// (a sync knows where it stands; outside the lanes / sens modes it does nothing)
static void emu_sync(const char* func, int line);
#define TAMD_UNLZ_SYNC() emu_sync(__func__, __LINE__)
#include "../../tonk_amd/csrc/unlz.h"
#include "lz_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <ucontext.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

extern "C" {
void* ref_comp_new(unsigned max);
int ref_comp(void* c, const uint8_t* data, unsigned bytes, uint8_t* dest, unsigned* written);
void ref_comp_free(void* c);
void* ref_decomp_new(unsigned max);
void ref_insert(void* d, const uint8_t* data, unsigned bytes);
int ref_decomp(void* d, const uint8_t* src, unsigned bytes, uint8_t* out, unsigned cap);
void ref_decomp_free(void* d);
}

typedef std::vector<uint8_t> Bytes;
struct Msg {
    bool is_block = false;
    Bytes data;
};
struct Stream {
    uint32_t max = 0;
    std::vector<Msg> msgs;
};

static bool read_streams(const char* path, std::vector<Stream>* out, bool verdicts = false) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    char magic[4];
    uint32_t n = 0;
    bool ok = fread(magic, 1, 4, f) == 4 && memcmp(magic, "UNLZ", 4) == 0 && fread(&n, 4, 1, f) == 1;
    for (uint32_t s = 0; ok && s < n; ++s) {
        Stream st;
        uint32_t m = 0;
        ok = fread(&st.max, 4, 1, f) == 1 && fread(&m, 4, 1, f) == 1;
        for (uint32_t k = 0; ok && k < m; ++k) {
            uint32_t isb = 0, len = 0;
            ok = fread(&isb, 4, 1, f) == 1 && fread(&len, 4, 1, f) == 1 && len <= (1u << 20);
            Msg g;
            g.is_block = isb != 0;
            g.data.resize(len);
            if (ok && len) ok = fread(g.data.data(), 1, len, f) == len;
            if (ok && verdicts) {  // (a case file's verdicts are skipped: the walk gives them again)
                int32_t status = 0;
                uint32_t r = 0;
                ok = fread(&status, 4, 1, f) == 1 && fread(&r, 4, 1, f) == 1 && r <= (1u << 20) && fseek(f, (long)r, SEEK_CUR) == 0;
            }
            st.msgs.push_back(g);
        }
        out->push_back(st);
    }
    fclose(f);
    return ok;
}

struct Case {  // a message with the walk's verdict
    Msg msg;
    int32_t status = 0;
    Bytes restored;
};
static void write_cases(FILE* f, uint32_t max, const std::vector<Case>& cs, bool verdicts) {
    const uint32_t m = (uint32_t)cs.size();
    fwrite(&max, 4, 1, f);
    fwrite(&m, 4, 1, f);
    for (const Case& c : cs) {
        const uint32_t isb = c.msg.is_block, len = (uint32_t)c.msg.data.size(), r = (uint32_t)c.restored.size();
        fwrite(&isb, 4, 1, f);
        fwrite(&len, 4, 1, f);
        if (len) fwrite(c.msg.data.data(), 1, len, f);
        if (verdicts) {
            fwrite(&c.status, 4, 1, f);
            fwrite(&r, 4, 1, f);
            if (r) fwrite(c.restored.data(), 1, r, f);
        }
    }
}

// The host walk: one stream's state with buffers of exactly the sizes the reader may touch.
struct Walk {
    uint32_t max;
    tamd_unlz_state* S;
    tamd_unlz_work* W;
    uint8_t *ring, *lit, *out;
    bool failed = false;
    explicit Walk(uint32_t mx) : max(mx) {
        S = (tamd_unlz_state*)malloc(sizeof(tamd_unlz_state));
        W = (tamd_unlz_work*)malloc(sizeof(tamd_unlz_work));
        ring = (uint8_t*)malloc(TAMD_UNLZ_RING);
        lit = (uint8_t*)malloc(mx);
        out = (uint8_t*)malloc(mx);
        memset(W, 0, sizeof(*W));
        memset(ring, 0, TAMD_UNLZ_RING);
        tamd_unlz_reset(S);
    }
    ~Walk() {
        free(S);
        free(W);
        free(ring);
        free(lit);
        free(out);
    }
    Walk(const Walk&) = delete;
    // a compressed block (copied into an exact allocation) or an uncompressed message
    int32_t feed(const Msg& m, Bytes* restored, uint32_t cap = 0) {
        restored->clear();
        if (failed) return TAMD_UNLZ_E_FAILED;
        const uint32_t n = (uint32_t)m.data.size();
        if (n == 0 || n > max) {
            failed = true;
            return TAMD_UNLZ_E_SIZE;
        }
        uint8_t* in = (uint8_t*)malloc(n);
        memcpy(in, m.data.data(), n);
        int32_t rc = 0;
        tamd_unlz_place(S, max);
        if (m.is_block) {
            uint32_t r = 0;
            // (the large literal buffer stands in for the kernel's scratch: same size here)
            rc = tamd_unlz_block(S, W, ring, in, n, cap ? cap : max, out, lit, max < TAMD_LZ_MAX_MESSAGE ? max : TAMD_LZ_MAX_MESSAGE,
                                 lit, max, 0, 1, &r);
            if (rc) failed = true;
            else restored->assign(out, out + r);
        } else {
            tamd_unlz_insert(S, ring, in, n, out, 0, 1);
            restored->assign(out, out + n);
        }
        free(in);
        return rc;
    }
};

struct RefDec {
    void* h;
    uint32_t max;
    Bytes buf;
    explicit RefDec(uint32_t mx) : h(ref_decomp_new(mx)), max(mx), buf(mx + 64) {}
    ~RefDec() { ref_decomp_free(h); }
    RefDec(const RefDec&) = delete;
    int feed(const Msg& m, Bytes* restored) {
        restored->clear();
        if (!m.is_block) {
            ref_insert(h, m.data.data(), (unsigned)m.data.size());
            *restored = m.data;
            return (int)m.data.size();
        }
        const int r = ref_decomp(h, m.data.data(), (unsigned)m.data.size(), buf.data(), max);
        if (r > 0) restored->assign(buf.begin(), buf.begin() + r);
        return r;
    }
};

// The reference compressor over a stream's messages: a block, or the message itself.
static std::vector<Msg> ref_blocks(const Stream& st) {
    std::vector<Msg> out;
    void* c = ref_comp_new(st.max);
    Bytes dest(st.max + 64);
    for (const Msg& m : st.msgs) {
        unsigned w = 0;
        ref_comp(c, m.data.data(), (unsigned)m.data.size(), dest.data(), &w);
        Msg b;
        b.is_block = w != 0;
        if (w) b.data.assign(dest.begin(), dest.begin() + w);
        else b.data = m.data;
        out.push_back(b);
    }
    ref_comp_free(c);
    return out;
}

static int fail(const char* what, size_t s, size_t k, int a = 0, int b = 0) {
    printf("FAIL %s (stream %zu, message %zu: %d / %d)\n", what, s, k, a, b);
    return 1;
}

// ---- Repeat rewrite: the table descriptions of a block's RLE / FSE-described entries removed and
// their modes set to Repeat; the bit stream stays.  False when the block has none.
static bool repeat_rewrite(const Bytes& b, Bytes* out) {
    tamd_unlz_work W;
    memset(&W, 0, sizeof(W));
    if (tamd_unlz_lit_header(b.data(), (uint32_t)b.size(), 1u << 20, &W)) return false;
    uint32_t at = W.seq_at;
    if (at >= b.size()) return false;
    uint32_t ns = b[at++];
    if (!ns) return false;
    if (ns >= 128) at += ns == 255 ? 2 : 1;
    if (at >= b.size()) return false;
    const uint32_t modes_at = at, modes = b[at++];
    uint32_t new_modes = modes;
    const uint32_t shift[3] = {6, 4, 2};  // LL, OF, ML in the order of their descriptions
    const uint32_t max_sym[3] = {35, 31, 52}, max_log[3] = {9, 8, 9};
    Bytes res(b.begin(), b.begin() + at);
    bool any = false;
    for (uint32_t i = 0; i < 3; ++i) {
        const uint32_t mode = (modes >> shift[i]) & 3u;
        if (mode == 1) {
            at += 1;
        } else if (mode == 2) {
            int16_t norm[64];
            uint32_t nsym, lg, used;
            if (tamd_unlz_ncount(b.data() + at, (uint32_t)b.size() - at, max_sym[i], max_log[i], norm, &nsym, &lg, &used)) return false;
            at += used;
        }
        if (mode == 1 || mode == 2) {
            new_modes |= 3u << shift[i];
            any = true;
        }
    }
    if (!any || at > b.size()) return false;
    res.insert(res.end(), b.begin() + at, b.end());
    res[modes_at] = (uint8_t)new_modes;
    *out = res;
    return true;
}

// ---- the GPU compressor's format: the host compressor of lz_host.h (as tests/native/lz_check.cpp
// drives it) over the linear stream, with the guards a stream of any maximum needs.
static std::vector<Msg> gpu_format_blocks(const Stream& st) {
    std::vector<Msg> res;
    uint8_t fse[TAMD_FSE_BYTES];
    tamd_fse_blob(fse);
    Bytes stream;
    for (const Msg& m : st.msgs) stream.insert(stream.end(), m.data.begin(), m.data.end());
    stream.resize(stream.size() + 16);
    RingTrack ring;
    ring.max = st.max;
    LzHostOptions opt;
    opt.floor = 16;
    opt.len_cap = 60000;
    opt.max = st.max;
    std::vector<int64_t> table(1u << 14, -1);
    Bytes out;
    for (const Msg& m : st.msgs) {
        uint64_t pos = 0, win = 0;
        ring.place((uint32_t)m.data.size(), &pos, &win);
        LzHostStats hs;
        const uint32_t w = lz_host_block(stream.data(), pos, (uint32_t)m.data.size(), win, table, fse, opt, &out, &hs);
        Msg b;
        b.is_block = w != 0;
        if (w) b.data.assign(out.begin(), out.begin() + w);
        else b.data = m.data;
        res.push_back(b);
    }
    return res;
}

static const char* kCntName[TAMD_CNT_N] = {
    "lit_raw", "lit_rle", "lit_huffman", "lit_treeless", "huf_1_stream", "huf_4_streams", "weights_direct", "weights_fse",
    "no_sequences", "ll_predefined", "ll_rle", "ll_fse", "ll_repeat", "ml_predefined", "ml_rle", "ml_fse", "ml_repeat",
    "of_predefined", "of_rle", "of_fse", "of_repeat", "offset_new", "rep0", "rep1", "rep2", "rep_ll0_1", "rep_ll0_2",
    "rep_ll0_minus1", "ext_dict_match", "ext_dict_cross", "overlap_match", "ring_restart"};

// Blocks through the walk and the reference side by side; `want`: the original messages (null:
// only the two decoders are compared).
// (`seen`: the walk's bytes and stream state after every message, and what the reader says of the block)
struct Seen {
    Bytes bytes;
    uint32_t rep[3], next, dict_len;
    uint32_t nseq, lit_type, n_streams, lit_sel, nbig;
    int32_t status;
};
// (`rejects`: the stream's last message is a block that the walk and the reference both reject)
static int run_pair(const std::vector<Msg>& blocks, const std::vector<Msg>* want, uint32_t max, size_t s, const char* what,
                    std::vector<Seen>* seen = nullptr, bool rejects = false) {
    Walk wk(max);
    RefDec rd(max);
    Bytes a, b;
    for (size_t k = 0; k < blocks.size(); ++k) {
        const int32_t rc = wk.feed(blocks[k], &a);
        const int r = rd.feed(blocks[k], &b);
        const bool last_rejected = rejects && k + 1 == blocks.size();
        if (last_rejected ? (rc == 0 || r > 0) : (rc || r <= 0)) return fail(what, s, k, rc, r);
        if (a != b) return fail("walk differs from the reference decompressor", s, k);
        if (want && !last_rejected && a != (*want)[k].data) return fail("walk differs from the message", s, k);
        if (seen) {
            Seen e;
            e.bytes = a;
            e.status = rc;
            for (int i = 0; i < 3; ++i) e.rep[i] = wk.S->rep[i];
            e.next = wk.S->next;
            e.dict_len = wk.S->dict_len;
            e.nseq = wk.W->nseq;
            e.lit_type = wk.W->lit_type;
            e.n_streams = wk.W->n_streams;
            e.lit_sel = wk.W->lit_sel;
            e.nbig = wk.W->nbig;
            seen->push_back(e);
        }
    }
    return 0;
}

static int mode_check(const std::vector<Stream>& streams, const char* rewrites_out) {
    FILE* fo = rewrites_out ? fopen(rewrites_out, "wb") : nullptr;
    std::vector<std::pair<uint32_t, std::vector<Case>>> dump;
    unsigned long long n_blocks = 0, n_rewrites = 0, n_gpu_blocks = 0, n_rewrite_streams = 0;
    for (size_t s = 0; s < streams.size(); ++s) {
        const Stream& st = streams[s];
        const std::vector<Msg> blocks = ref_blocks(st);
        for (const Msg& b : blocks) n_blocks += b.is_block;
        if (run_pair(blocks, &st.msgs, st.max, s, "reference block rejected")) return 1;
        // Repeat rewrites: up to 24 probe positions spread over the stream's candidates
        std::vector<size_t> cand;
        std::vector<Bytes> rew;
        for (size_t k = 0; k < blocks.size(); ++k) {
            Bytes r;
            if (blocks[k].is_block && repeat_rewrite(blocks[k].data, &r)) {
                cand.push_back(k);
                rew.push_back(r);
            }
        }
        const size_t probes = cand.size() < 24 ? cand.size() : 24;
        size_t accepted = 0;
        for (size_t j = 0; j < probes; ++j) {
            const size_t ci = j * cand.size() / probes, k = cand[ci];
            Walk wk(st.max);
            RefDec rd(st.max);
            Bytes a, b;
            std::vector<Case> cs;
            for (size_t q = 0; q <= k; ++q) {
                if (wk.feed(blocks[q], &a) || rd.feed(blocks[q], &b) <= 0 || a != b) return fail("rewrite prefix", s, q);
                Case c;
                c.msg = blocks[q];
                cs.push_back(c);
            }
            Msg extra;
            extra.is_block = true;
            extra.data = rew[ci];
            const int32_t rc = wk.feed(extra, &a);
            const int r = rd.feed(extra, &b);
            if (r <= 0) continue;  // (the reference does not take this rewrite: no expectation)
            if (rc) return fail("Repeat rewrite rejected by the walk", s, k, rc, r);
            if (a != b) return fail("Repeat rewrite: bytes differ from the reference's", s, k);
            ++n_rewrites;
            ++accepted;
            Case c;
            c.msg = extra;
            cs.push_back(c);
            if (j < 4) dump.push_back(std::make_pair(st.max, cs));
        }
        printf("stream %zu: repeat rewrites %zu accepted of %zu probed (%zu candidates)\n", s, accepted, probes, cand.size());
        if (cand.size() >= 20 && accepted < 20) return fail("fewer than 20 Repeat rewrites accepted in a stream with 20 candidates", s, accepted);
        n_rewrite_streams += accepted >= 20;
        // the GPU compressor's format
        if (s < 4 || st.max > 1300) {
            const std::vector<Msg> gb = gpu_format_blocks(st);
            for (const Msg& b : gb) n_gpu_blocks += b.is_block;
            if (run_pair(gb, &st.msgs, st.max, s, "block of the GPU compressor's format rejected")) return 1;
        }
    }
    // hand-made blocks on a fresh stream: 20 x 'A' as RLE literals, "hello" as raw literals
    {
        const uint8_t rle[3] = {0xa1, 0x41, 0x00};
        const uint8_t raw[7] = {0x28, 'h', 'e', 'l', 'l', 'o', 0x00};
        std::vector<Msg> hm(2);
        hm[0].is_block = hm[1].is_block = true;
        hm[0].data.assign(rle, rle + 3);
        hm[1].data.assign(raw, raw + 7);
        std::vector<Msg> want(2);
        want[0].data.assign(20, 'A');
        want[1].data.assign(raw + 1, raw + 6);
        if (run_pair(hm, &want, 1300, 9999, "hand-made block rejected")) return 1;
        std::vector<Case> cs(2);
        cs[0].msg = hm[0];
        cs[1].msg = hm[1];
        dump.push_back(std::make_pair(1300u, cs));
    }
    // hand-made: the repeat-offset codes no level-1 compressor writes.  200 bytes of history, then
    // one block: raw literals and sequences (literal length, match length, Offset_Value; the
    // writer of lz.h codes seq_off + 3, so Offset_Value v is passed as v - 3).
    {
        std::vector<Msg> hm(2);
        uint32_t x = 7;
        for (int i = 0; i < 200; ++i) {
            x = x * 1664525u + 1013904223u;
            hm[0].data.push_back((uint8_t)(x >> 24));
        }
        const uint32_t seq[][3] = {
            {4, 8, 50 + 3},  // new offsets: 50, then 70
            {3, 5, 70 + 3},
            {2, 6, 2},       // literals, code 2: the second repeat offset (50)
            {2, 4, 3},       // literals, code 3: the third (1)
            {0, 5, 3},       // no literals, code 3: the first minus one = 0, decoded as 1
            {0, 7, 2},       // no literals, code 2: the third
            {0, 9, 3},       // no literals, code 3: the first minus one
            {1, 3, 1},       // code 1: the first
        };
        const uint32_t ns = sizeof(seq) / sizeof(seq[0]);
        uint32_t lo[ns], off[ns], lits = 5;
        for (uint32_t i = 0; i < ns; ++i) {
            lo[i] = seq[i][0] | (seq[i][1] << 16);
            off[i] = seq[i][2] - 3u;
            lits += seq[i][0];
        }
        uint8_t fse[TAMD_FSE_BYTES];
        tamd_fse_blob(fse);
        Bytes b(128);
        uint32_t w = tamd_lits_header(lits, b.data());
        for (uint32_t i = 0; i < lits; ++i) b[w++] = (uint8_t)('a' + i);
        w += tamd_seq_header(ns, &b[w]);
        const uint32_t nb = tamd_fse_sequences(lo, off, ns, fse, &b[w], 64);
        if (!nb) return fail("hand-made repeat-offset block: writer", 0, 0);
        b.resize(w + nb);
        hm[1].is_block = true;
        hm[1].data = b;
        if (run_pair(hm, nullptr, 1300, 9998, "hand-made repeat-offset block rejected")) return 1;
        std::vector<Case> cs(2);
        cs[0].msg = hm[0];
        cs[1].msg = hm[1];
        dump.push_back(std::make_pair(1300u, cs));
    }
    if (fo) {
        const uint32_t n = (uint32_t)dump.size();
        fwrite("UNLZ", 1, 4, fo);
        fwrite(&n, 4, 1, fo);
        for (auto& d : dump) write_cases(fo, d.first, d.second, false);
        fclose(fo);
    }
    int zero = 0;
    for (int i = 0; i < TAMD_CNT_N; ++i) {
        printf("path %s %llu\n", kCntName[i], g_cnt[i]);
        zero += g_cnt[i] == 0;
    }
    printf("blocks %llu, repeat rewrites %llu, gpu-format blocks %llu\n", n_blocks, n_rewrites, n_gpu_blocks);
    if (zero) {
        printf("FAIL %d reader paths never ran\n", zero);
        return 1;
    }
    printf("streams with at least 20 accepted repeat rewrites: %llu\n", n_rewrite_streams);
    if (n_rewrites < 20 || n_rewrite_streams < 3) {
        printf("FAIL too few Repeat rewrites\n");
        return 1;
    }
    printf("ok\n");
    return 0;
}

// ---- malformed blocks -----------------------------------------------------------------------
struct Subject {
    uint32_t max;
    std::vector<Msg> prefix;
    Msg block;
};

struct MutStats {
    unsigned long long tried = 0, walk_ok = 0, ref_ok = 0, ref_only = 0;
    unsigned long long ref_only_by[16] = {0};  // by the walk's status (its negative)
};

// One mutant after its prefix: the walk's verdict; the reference beside it.  Returns nonzero when
// the walk accepted what the reference rejects or restores differently.
static int try_mutant(const Subject& sj, const Msg& mutant, MutStats* ms, std::vector<Case>* record, uint32_t cap = 0) {
    Walk wk(sj.max);
    RefDec rd(sj.max);
    Bytes a, b;
    std::vector<Case> cs;
    for (const Msg& m : sj.prefix) {
        const int32_t rc = wk.feed(m, &a);
        if (rc || rd.feed(m, &b) <= 0 || a != b) return fail("mutant prefix", 0, 0, rc);
        Case c;
        c.msg = m;
        c.restored = a;
        cs.push_back(c);
    }
    const int32_t rc = wk.feed(mutant, &a, cap);
    ++ms->tried;
    if (cap) {  // (capacity case: the reference has no such parameter here)
        if (rc != TAMD_UNLZ_E_DSTCAP) return fail("capacity too small was not rejected", 0, 0, rc);
        return 0;
    }
    const int r = rd.feed(mutant, &b);
    ms->walk_ok += rc == 0;
    ms->ref_ok += r > 0;
    ms->ref_only += rc != 0 && r > 0;
    if (rc != 0 && r > 0) ++ms->ref_only_by[(-rc) & 15];
    if (rc == 0 && (r <= 0 || a != b)) return fail("the walk accepted a mutant the reference does not restore the same", 0, 0, rc, r);
    if (record) {
        Case c;
        c.msg = mutant;
        c.status = rc;
        c.restored = a;
        cs.push_back(c);
        // a later message of the stream (sent uncompressed): restored only when the mutant was accepted
        Case t;
        t.msg.data.assign(48, (uint8_t)'t');
        t.status = wk.feed(t.msg, &t.restored);
        cs.push_back(t);
        *record = cs;
    }
    return 0;
}

static int mode_mutants(const std::vector<Stream>& streams, const char* cases_out) {
    // three valid blocks of different shapes, early in their streams (short prefixes): raw
    // literals with sequences, Huffman literals with a tree, treeless Huffman literals
    std::vector<Subject> subj;
    bool have[3] = {false, false, false};
    for (const Stream& st : streams) {
        const std::vector<Msg> blocks = ref_blocks(st);
        for (size_t k = 0; k < blocks.size() && k < 16; ++k) {
            if (!blocks[k].is_block) continue;
            const uint32_t type = blocks[k].data[0] & 3u;
            const int shape = type == 0 ? 0 : type == 2 ? 1 : type == 3 ? 2 : -1;
            if (shape < 0 || have[shape]) continue;
            if (shape == 0 && blocks[k].data.size() < 40) continue;
            have[shape] = true;
            Subject sj;
            sj.max = st.max;
            sj.prefix.assign(blocks.begin(), blocks.begin() + k);
            sj.block = blocks[k];
            subj.push_back(sj);
        }
    }
    if (subj.size() != 3) {
        printf("FAIL found %zu of the three block shapes\n", subj.size());
        return 1;
    }
    MutStats ms;
    std::vector<std::pair<uint32_t, std::vector<Case>>> chosen;
    uint32_t rng = 12345;
    auto rnd = [&rng]() {
        rng = rng * 1664525u + 1013904223u;
        return rng >> 8;
    };
    for (size_t j = 0; j < subj.size(); ++j) {
        const Subject& sj = subj[j];
        MutStats one;
        std::vector<Case> rec;
        if (try_mutant(sj, sj.block, &one, &rec) || one.walk_ok != 1) return fail("unmutated block rejected", j, 0);
        chosen.push_back(std::make_pair(sj.max, rec));
        const size_t n = sj.block.data.size();
        for (size_t len = 1; len < n; ++len) {  // every truncation
            Msg m = sj.block;
            m.data.resize(len);
            const bool keep = len % (n / 6 + 1) == 1;
            if (try_mutant(sj, m, &ms, keep ? &rec : nullptr)) return 1;
            if (keep) chosen.push_back(std::make_pair(sj.max, rec));
        }
        for (int t = 0; t < 2000; ++t) {  // seeded single-bit flips
            Msg m = sj.block;
            const uint32_t bit = rnd() % (uint32_t)(8 * n);
            m.data[bit >> 3] ^= (uint8_t)(1u << (bit & 7u));
            const bool keep = t % 143 == 0;
            if (try_mutant(sj, m, &ms, keep ? &rec : nullptr)) return 1;
            if (keep) chosen.push_back(std::make_pair(sj.max, rec));
        }
        // the output capacity one byte short of what the block restores
        Walk wk(sj.max);
        Bytes a;
        for (const Msg& m : sj.prefix) wk.feed(m, &a);
        wk.feed(sj.block, &a);
        if (a.size() > 1 && try_mutant(sj, sj.block, &ms, nullptr, (uint32_t)a.size() - 1)) return 1;
    }
    {  // an offset beyond the history: one sequence, offset 30000, on a fresh stream and after a prefix
        uint8_t fse[TAMD_FSE_BYTES];
        tamd_fse_blob(fse);
        for (int with_prefix = 0; with_prefix < 2; ++with_prefix) {
            Bytes b(64);
            uint32_t w = tamd_lits_header(8, b.data());
            memcpy(&b[w], "abcdefgh", 8);
            w += 8;
            uint8_t h[4];
            const uint32_t hs = tamd_seq_header(1, h);
            memcpy(&b[w], h, hs);
            w += hs;
            const uint32_t lo = 4u | (8u << 16), off = 30000;
            w += tamd_fse_sequences(&lo, &off, 1, fse, &b[w], 32);
            b.resize(w);
            Subject sj;
            sj.max = subj[0].max;
            if (with_prefix) sj.prefix = subj[0].prefix;
            Msg m;
            m.is_block = true;
            m.data = b;
            MutStats one;
            std::vector<Case> rec;
            if (try_mutant(sj, m, &one, &rec)) return 1;
            if (one.walk_ok || one.ref_ok) return fail("offset beyond the history was accepted", 0, 0);
            if (rec[rec.size() - 2].status != TAMD_UNLZ_E_OFFSET) return fail("offset beyond the history: status", 0, 0, rec[rec.size() - 2].status);
            chosen.push_back(std::make_pair(sj.max, rec));
            ms.tried += 1;
        }
    }
    if (cases_out) {
        // 64 cases: a fixed, evenly spread selection
        FILE* fo = fopen(cases_out, "wb");
        if (!fo) return fail("cannot write the cases", 0, 0);
        const uint32_t want = 64, have_n = (uint32_t)chosen.size();
        const uint32_t n = have_n < want ? have_n : want;
        fwrite("UNLZ", 1, 4, fo);
        fwrite(&n, 4, 1, fo);
        for (uint32_t i = 0; i < n; ++i) {
            const auto& c = chosen[(size_t)i * have_n / n];
            write_cases(fo, c.first, c.second, true);
        }
        fclose(fo);
    }
    printf("mutants %llu: walk accepts %llu, reference accepts %llu, reference accepts and walk rejects %llu\n", ms.tried,
           ms.walk_ok, ms.ref_ok, ms.ref_only);
    for (int i = 1; i < 16; ++i)
        if (ms.ref_only_by[i]) printf("  rejected with status -%d though the reference accepts: %llu\n", i, ms.ref_only_by[i]);
    printf("ok\n");
    return 0;
}

// ---- the reference decompressor's rate ------------------------------------------------------
static int mode_bench(const std::vector<Stream>& streams, unsigned threads, unsigned reps) {
    std::vector<std::vector<Msg>> blocks(streams.size());
    {
        std::atomic<size_t> next(0);
        // (a stream given as blocks is timed as it is; a stream of raw messages is compressed by
        // the reference first)
        auto work = [&]() {
            for (size_t s; (s = next++) < streams.size();) {
                bool given = false;
                for (const Msg& m : streams[s].msgs) given = given || m.is_block;
                blocks[s] = given ? streams[s].msgs : ref_blocks(streams[s]);
            }
        };
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < threads; ++t) ts.emplace_back(work);
        for (auto& t : ts) t.join();
    }
    // Timed: the decoding alone.  Each repetition's threads are started, and each creates the
    // decoders (context and ring) of its own streams (s = t, t + threads, ...), before the clock
    // starts; they are freed after it stops.
    std::atomic<unsigned long long> bytes(0);
    std::vector<double> secs;
    for (unsigned rep = 0; rep < reps; ++rep) {
        std::atomic<unsigned> ready(0), finished(0);
        std::atomic<bool> go(false);
        bytes = 0;
        std::chrono::steady_clock::time_point t1;
        auto work = [&](unsigned t) {
            std::vector<RefDec*> decs;
            for (size_t s = t; s < streams.size(); s += threads) decs.push_back(new RefDec(streams[s].max));
            ++ready;
            while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
            unsigned long long b = 0;
            size_t i = 0;
            for (size_t s = t; s < streams.size(); s += threads) {
                RefDec& rd = *decs[i++];
                for (const Msg& m : blocks[s]) {
                    if (m.is_block) {
                        const int r = ref_decomp(rd.h, m.data.data(), (unsigned)m.data.size(), rd.buf.data(), rd.max);
                        b += r > 0 ? (unsigned)r : 0u;
                    } else {
                        ref_insert(rd.h, m.data.data(), (unsigned)m.data.size());
                        b += m.data.size();
                    }
                }
            }
            bytes += b;
            if (++finished == threads) t1 = std::chrono::steady_clock::now();  // (the last thread stops the clock)
            for (RefDec* d : decs) delete d;
        };
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < threads; ++t) ts.emplace_back(work, t);
        while (ready.load() < threads) std::this_thread::yield();
        const auto t0 = std::chrono::steady_clock::now();
        go.store(true, std::memory_order_release);
        for (auto& t : ts) t.join();
        secs.push_back(std::chrono::duration<double>(t1 - t0).count());
    }
    // (the host is shared: the median repetition, with the fastest and the slowest beside it)
    std::sort(secs.begin(), secs.end());
    const double sec = secs[secs.size() / 2];
    const double gib = (double)bytes / (1024.0 * 1024.0 * 1024.0);
    printf("{\"threads\": %u, \"reps\": %u, \"seconds\": %.6f, \"restored_bytes\": %llu, \"gib_per_s\": %.4f, "
           "\"gib_per_s_slowest\": %.4f, \"gib_per_s_fastest\": %.4f}\n",
           threads, reps, sec, (unsigned long long)bytes, gib / sec, gib / secs.back(), gib / secs.front());
    return 0;
}

// ---- the decode-table build over 64 lanes -----------------------------------------------------
// tamd_unlz_fse_table's phases run for 64 lanes one after the other, phase by phase (what the
// kernel's wave does between its synchronisations), against the table built state by state in
// the order FSE_buildDTable defines; also with one lane, the host walk's form.
static void classic_table(const int16_t* norm, uint32_t nsym, uint32_t log, uint32_t* tab) {
    const uint32_t size = 1u << log, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
    std::vector<uint8_t> spread(size);
    std::vector<uint32_t> nxt(nsym);
    uint32_t high = size - 1u;
    for (uint32_t s = 0; s < nsym; ++s) {
        if (norm[s] == -1) {
            spread[high--] = (uint8_t)s;
            nxt[s] = 1;
        } else {
            nxt[s] = (uint32_t)norm[s];
        }
    }
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; ++s)
        for (int32_t i = 0; i < norm[s]; ++i) {
            spread[pos] = (uint8_t)s;
            pos = (pos + step) & mask;
            while (pos > high) pos = (pos + step) & mask;
        }
    for (uint32_t u = 0; u < size; ++u) {
        const uint32_t s = spread[u], ns = nxt[s]++;
        const uint32_t nb = log - (31u - (uint32_t)__builtin_clz(ns));
        tab[u] = s | (nb << 8) | (((ns << nb) - size) << 16);
    }
}

static int mode_tables() {
    uint32_t rng = 2024;
    auto rnd = [&rng]() {
        rng = rng * 1664525u + 1013904223u;
        return rng >> 8;
    };
    const uint32_t NL = 64;
    unsigned long long n_tables = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        const uint32_t log = trial < 3 ? (trial == 2 ? 5u : 6u) : 5u + rnd() % 5u, size = 1u << log;
        const uint32_t max_sym = trial % 7 == 0 ? 256u : 53u;
        int16_t norm[256];
        uint32_t nsym = 0;
        if (trial < 3) {  // the predefined distributions
            uint32_t tab[64], one[64];
            uint8_t spread[512];
            uint16_t nxt[256], cum[256];
            // (built by one lane; compared below through the classic build of the same counts)
            tamd_unlz_predefined((uint32_t)trial, one, norm, spread, nxt, cum, 0, 1);
            nsym = trial == 0 ? 36u : trial == 1 ? 53u : 29u;
            classic_table(norm, nsym, log, tab);
            if (memcmp(tab, one, size * 4u)) return fail("predefined table", (size_t)trial, 0);
        } else {  // random counts that sum to the size: some zero, some "less than one"
            uint32_t left = size;
            while (left && nsym < max_sym) {
                const uint32_t kind = rnd() % 8u;
                uint32_t c;
                if (kind == 0) c = 0;
                else if (kind == 1) c = ~0u;  // -1
                else if (kind == 2) c = 1u + rnd() % left;
                else c = 1u + rnd() % (left < 6u ? left : 6u);
                if (nsym + 1 == max_sym && (c == 0 || c == ~0u)) c = 1;
                norm[nsym++] = c == ~0u ? (int16_t)-1 : (int16_t)c;
                left -= c == ~0u ? 1u : c;
            }
            if (left) {  // (out of symbols: the last one takes the rest)
                const int16_t last = norm[nsym - 1];
                norm[nsym - 1] = (int16_t)((last < 0 ? 1 : (int32_t)last) + (int32_t)left);
            }
        }
        uint32_t sum = 0;
        for (uint32_t s = 0; s < nsym; ++s) sum += norm[s] < 0 ? 1u : (uint32_t)norm[s];
        if (sum != size) return fail("table test: counts do not sum to the size", (size_t)trial, sum);
        uint32_t want[512], got[512], one[512];
        uint8_t spread[512];
        uint16_t nxt[256], cum[256];
        classic_table(norm, nsym, log, want);
        memset(one, 0xee, sizeof(one));
        memset(spread, 0xee, sizeof(spread));
        tamd_unlz_fse_table(norm, nsym, log, one, spread, nxt, cum, 0, 1);
        if (memcmp(want, one, size * 4u)) return fail("table built by one lane differs", (size_t)trial, log);
        memset(got, 0xee, sizeof(got));
        memset(spread, 0xee, sizeof(spread));
        for (uint32_t l = 0; l < NL; ++l) tamd_unlz_fse_symbols(norm, nsym, log, spread, nxt, cum, l, NL);
        for (uint32_t l = 0; l < NL; ++l) tamd_unlz_fse_spread(norm, nsym, log, spread, cum, l, NL);
        for (uint32_t b = 0; b < size; b += NL) {
            uint32_t v[64];
            for (uint32_t l = 0; l < NL; ++l) v[l] = tamd_unlz_fse_number(spread, nxt, log, b, l, NL);
            for (uint32_t l = 0; l < NL; ++l) tamd_unlz_fse_put(v[l], got, nxt, log, b, l);
        }
        if (memcmp(want, got, size * 4u)) return fail("table built by 64 lanes differs", (size_t)trial, log);
        ++n_tables;
    }
    printf("tables %llu: 64 lanes == one lane == state order\nok\n", n_tables);
    return 0;
}

// ---- the two forms of the ring rule ----------------------------------------------------------
// RingTrack (lz.h: the compressor's linear positions and window start) and tamd_unlz_place (the
// decoder's ring offset and dictionary length) stepped side by side over seeded message lengths.
static int mode_ring() {
    const uint32_t sizes[] = {1, 7, 1300, 4000, 8000, 11999, 12000, 12001, 23999, 24000};
    unsigned long long placements = 0, restarts = 0, partial = 0;
    for (uint32_t max : sizes)
        for (uint32_t stream = 0; stream < 200; ++stream) {
            uint32_t rng = max * 1000u + stream;
            auto rnd = [&rng]() {
                rng = rng * 1664525u + 1013904223u;
                return rng >> 8;
            };
            RingTrack rt;
            rt.max = max;
            tamd_unlz_state S;
            tamd_unlz_reset(&S);
            uint64_t lin = 0;
            for (uint32_t k = 0; k < 400; ++k) {
                // uniform in 1..max; a fifth of the lengths forced to max, a seventh to 1
                const uint32_t kind = rnd() % 35u;
                const uint32_t n = kind < 7u ? max : kind < 12u ? 1u : 1u + rnd() % max;
                uint64_t pos = 0, win = 0;
                rt.place(n, &pos, &win);
                const uint32_t before = S.next;
                tamd_unlz_place(&S, max);
                restarts += before != 0 && S.next == 0;
                if (pos != lin) return fail("ring: position is not the running byte count", max, k);
                if (S.next + n > TAMD_UNLZ_RING) return fail("ring: message placed past the ring's end", max, k);
                const uint64_t seg = lin - S.next;
                const uint32_t left = S.dict_len > S.next + n ? S.dict_len - (S.next + n) : 0u;
                if (win != seg - left) return fail("ring: window start differs from the decoder's history", max, k);
                partial += left != 0;
                ++placements;
                S.next += n;
                lin += n;
            }
        }
    printf("placements %llu, restarts %llu, partly overwritten dictionary %llu\nok\n", placements, restarts, partial);
    return 0;
}

static const char* kWaitName[TAMD_CNT_ALL - TAMD_CNT_N] = {"ext_wait", "ext_no_wait", "cross_rest", "cross_none",
                                                            "match_wait", "match_no_wait"};

static void print_counters(const unsigned long long* c, const char* sep) {
    for (int i = 0; i < TAMD_CNT_N; ++i) printf("%s\"%s\": %llu", i ? sep : "", kCntName[i], c[i]);
}

// ---- directed blocks -------------------------------------------------------------------------
// The generator chooses the parse: literals are seeded bytes, every match is copied from the
// history at its offset, and lz_host_write writes the block.  The history is kept as the decoder
// holds it (the ring rule restated: write offset, previous segment), and beside it RingTrack says
// where the compressor's window starts: a match that would start before it is a generator bug,
// except where a case says `outside` (below: the one wait no in-window block can reach).
struct Seq {
    uint32_t ll, ml, off;
};
struct Gen {
    uint32_t max, next = 0, dict_len = 0, rng;
    RingTrack rt;
    Bytes ring;
    const uint8_t* fse;
    std::vector<Msg> blocks;  // what the decoder is given
    std::vector<Msg> want;    // the messages
    std::string err;
    Gen(uint32_t mx, uint32_t seed, const uint8_t* f) : max(mx), rng(seed * 2654435761u + 12345u), ring(TAMD_UNLZ_RING), fse(f) {
        rt.max = mx;
    }
    // alphabet 0: skewed (symbol s with probability 2^-(s+1), s < 20); else uniform below it
    uint8_t byte(uint32_t alphabet) {
        rng = rng * 1664525u + 1013904223u;
        const uint32_t v = rng >> 8;
        if (alphabet) return (uint8_t)(v % alphabet);
        uint32_t s = 0;
        while (s < 19 && ((v >> s) & 1u)) ++s;
        return (uint8_t)s;
    }
    uint64_t place(uint32_t n, uint64_t* win) {
        if (next + max > TAMD_UNLZ_RING) {
            if (next) dict_len = next;
            next = 0;
        }
        uint64_t pos = 0;
        rt.place(n, &pos, win);
        return pos;
    }
    void plain(uint32_t n, uint32_t alphabet) {  // a message sent as it is: history
        uint64_t win = 0;
        place(n, &win);
        Msg m;
        for (uint32_t i = 0; i < n; ++i) m.data.push_back(ring[next + i] = byte(alphabet));
        next += n;
        blocks.push_back(m);
        want.push_back(m);
    }
    bool block(const std::vector<Seq>& seqs, uint32_t tail, uint32_t alphabet, bool fitted, bool huffman = true,
               bool outside = false) {
        uint32_t n = tail;
        for (const Seq& s : seqs) n += s.ll + s.ml;
        if (n == 0 || n > max) return bad("message size");
        uint64_t win = 0;
        const uint64_t pos = place(n, &win);
        LzHostStats st;
        Msg m;
        uint32_t q = next;
        for (const Seq& s : seqs) {
            for (uint32_t i = 0; i < s.ll; ++i) m.data.push_back(ring[q++] = byte(alphabet));
            if (!outside && pos + (q - next) < win + s.off) return bad("match starts before the compressor's window");
            if (s.ml < 3 || s.off == 0) return bad("match");
            for (uint32_t i = 0; i < s.ml; ++i, ++q) {
                uint32_t from;
                if (s.off <= q) from = q - s.off;
                else if (s.off - q <= dict_len) from = dict_len - (s.off - q);
                else return bad("offset beyond the history");
                m.data.push_back(ring[q] = ring[from]);
            }
            st.lo.push_back(s.ll | (s.ml << 16));
            st.off.push_back(s.off);
        }
        for (uint32_t i = 0; i < tail; ++i) m.data.push_back(ring[q++] = byte(alphabet));
        LzHostOptions opt;
        opt.huffman = huffman;
        opt.fitted = fitted;
        opt.max = max;
        opt.slack = 16;  // (a directed block may be a little longer than its message)
        Bytes out;
        const uint32_t w = lz_host_write(m.data.data(), n, fse, opt, &out, &st);
        if (!w) return bad("the writer did not write the block");
        Msg b;
        b.is_block = true;
        b.data.assign(out.begin(), out.begin() + w);
        next += n;
        blocks.push_back(b);
        want.push_back(m);
        return true;
    }
    bool bad(const char* what) {
        err = what;
        return false;
    }
    // plain messages up to the ring's restart: the next message starts a new segment
    void fill() {
        while (next + max <= TAMD_UNLZ_RING) plain(max, 256);
    }
};

struct Group {
    const char* name;
    std::vector<Gen> streams;
};

static bool directed_groups(const uint8_t* fse, std::vector<Group>* out) {
    uint32_t seed = 1;
    bool ok = true;
    {  // chunks: nseq around the multiples of TAMD_UNLZ_CHUNK, every sequence (ll 1, ml 4); the first
        // match of a chunk reads what the last match of the chunk before wrote (offset = ml).
        // (127 / 128: the 1- / 2-byte count.  The 3-byte count needs 32,512 sequences, more than a
        // 24,000-byte history holds: not here.)
        Group g{"chunks", {}};
        const uint32_t ns[] = {1, 63, 64, 65, 127, 128, 129, 191, 192, 193};
        for (int fitted = 0; fitted < 2; ++fitted)
            for (uint32_t n : ns) {
                Gen s(1300, seed++, fse);
                s.plain(300, 256);
                s.plain(300, 256);
                std::vector<Seq> q;
                for (uint32_t i = 0; i < n; ++i) q.push_back(Seq{1, 4, i && i % TAMD_UNLZ_CHUNK == 0 ? 4u : 40u + (i * 7u) % 200u});
                ok = ok && s.block(q, 0, 256, fitted != 0);
                g.streams.push_back(s);
            }
        out->push_back(g);
    }
    {  // hazards: within one chunk, where a match's source lies against the bytes not yet waited for
        Group g{"hazards", {}};
        Gen s(1300, seed++, fse);
        s.plain(400, 256);
        s.plain(400, 256);
        const uint32_t lls[] = {0, 1, 63, 64, 65, 128};
        int k = 0;
        for (uint32_t ll : lls) {
            std::vector<std::vector<Seq>> pats;
            if (ll) {
                pats.push_back({Seq{ll, 8, ll}});  // the source is the literals just written
                pats.push_back({Seq{ll, 8, 1}});
            }
            pats.push_back({Seq{3, 10, 200}, Seq{ll, 5, ll + 5}});          // the previous match's output
            pats.push_back({Seq{ll, 6, ll + 6}});                           // ends where the chunk's bytes begin
            pats.push_back({Seq{1, 8, 1}, Seq{ll, 5, 8 + ll + 5}});         // ends where the bytes since the last wait begin
            pats.push_back({Seq{1, 8, 1}, Seq{ll, 3, 8 + ll + 1}});         // starts one byte below that point
            pats.push_back({Seq{1, 8, 1}, Seq{2, 9, 3}, Seq{ll, 4, ll + 2}});  // three sequences, the third into the second
            pats.push_back({Seq{ll, 6, ll + 300}});                         // wholly in older bytes: no wait
            pats.push_back({Seq{1, 8, 1}, Seq{ll, 6, 8 + ll + 300}});
            for (const auto& p : pats) ok = ok && s.block(p, 2, 256, (k++ & 1) != 0);
        }
        // one byte below the chunk's first byte to one byte past it (period 2)
        ok = ok && s.block({Seq{1, 4, 2}}, 2, 256, false);
        g.streams.push_back(s);
        // the same decisions for a match into the previous segment
        Gen e(1300, seed++, fse);
        e.fill();
        // The wait of an external match is taken only when it reads ring bytes that the current
        // segment has overwritten in this very chunk.  The reader and the reference both follow
        // such an offset (they read the ring as it physically is), no compressor writes one: the
        // one case here outside the window.  First message of the new segment: 100 literals, then
        // 20 bytes from ring offset 50.
        const uint32_t dl = e.next;
        ok = ok && e.block({Seq{100, 20, 100 + (dl - 50)}}, 2, 256, false, true, true);
        uint32_t q = e.next + 10;
        ok = ok && e.block({Seq{10, 12, q + 500}}, 2, 256, false);       // inside the segment before: no wait, no rest
        q = e.next + 5;
        ok = ok && e.block({Seq{5, 6 + 10, q + 6}}, 2, 256, true);        // crosses into the new segment
        g.streams.push_back(e);
        out->push_back(g);
    }
    {  // overlap: the period below, at and above the lane count; the length around one and two passes
        Group g{"overlap", {}};
        const uint32_t offs[] = {1, 2, 3, 7, 8, 9, 63, 64, 65}, mls[] = {3, 4, 63, 64, 65, 127, 128, 129, 300};
        for (uint32_t off : offs) {
            Gen s(1300, seed++, fse);
            s.plain(300, 256);
            s.plain(300, 256);
            std::vector<Seq> q;
            for (uint32_t ml : mls) q.push_back(Seq{2, ml, off});
            ok = ok && s.block(q, 3, 256, (off & 1) != 0);
            g.streams.push_back(s);
        }
        out->push_back(g);
    }
    {  // external: behind a ring restart, matches into the previous segment and across its end
        Group g{"external", {}};
        for (uint32_t max : {1300u, 4000u}) {
            Gen s(max, seed++, fse);
            s.fill();
            for (int behind = 0; behind < 2; ++behind)
                // kind 0: the continued part is longer than the offset; 1: inside; 2: up to the
                // segment's last byte; 3..6: crossing by 1, 63, 64, 65 bytes
                for (int kind = 0; kind < 7; ++kind) {
                    const bool restart = s.next + max > TAMD_UNLZ_RING;
                    const uint32_t at = restart ? 0u : s.next;
                    std::vector<Seq> p;
                    uint32_t q = at;
                    if (behind) {
                        p.push_back(Seq{3, 4, q + 3 + 200});
                        q += 9;
                    }
                    const uint32_t ll = behind ? 2u : 0u;
                    const uint32_t cross[] = {1, 63, 64, 65};
                    if (kind == 0) p.push_back(Seq{ll, 9 + (q + 9 + 7), q + 9});
                    else if (kind == 1) p.push_back(Seq{ll, 20, q + 300});
                    else if (kind == 2) p.push_back(Seq{ll, 17, q + 17});
                    else p.push_back(Seq{ll, 9 + cross[kind - 3], q + 9});
                    ok = ok && s.block(p, 2, 256, (kind & 1) != 0);
                }
            g.streams.push_back(s);
        }
        out->push_back(g);
    }
    {  // sizes: block bytes around the copy's 256-byte pass and TAMD_LZ_MAX_MESSAGE; literal counts
        // around the LDS buffer, the four streams' shares and the raw headers
        Group g{"sizes", {}};
        for (uint32_t target : {255u, 256u, 257u, 259u, 1535u, 1536u, 1537u}) {
            uint32_t L = target - 8;
            bool hit = false;
            for (int it = 0; it < 8 && !hit; ++it) {
                Gen s(4000, seed, fse);
                s.plain(600, 256);
                if (!s.block({Seq{L, 4, 100}}, 0, 256, false, false)) break;
                const uint32_t b = (uint32_t)s.blocks.back().data.size();
                if (b == target) {
                    g.streams.push_back(s);
                    hit = true;
                } else {
                    L += target - b;
                }
            }
            ok = ok && hit;
            ++seed;
        }
        const uint32_t hl[] = {256, 257, 258, 259, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 1535, 1536, 1537};
        int k = 0;
        for (uint32_t L : hl) {
            // (a uniform alphabet of 128: no symbol fills 64 table entries; it beats raw literals
            // only where there are many)
            const uint32_t alphabet = L > 1000 && (k++ & 1) ? 128u : 0u;
            Gen s(4000, seed++, fse);
            s.plain(600, alphabet);
            ok = ok && s.block({Seq{L, 4, 100}}, 0, alphabet, true);
            g.streams.push_back(s);
        }
        // the raw header's 1, 2 and 3 bytes (4095 literals do not fit a stream of 4000: 8000 there)
        for (uint32_t L : {31u, 32u, 4095u, 4096u}) {
            Gen s(L > 4000 ? 8000u : 4000u, seed++, fse);
            s.plain(600, 256);
            ok = ok && s.block({Seq{L, 4, 100}}, 0, 256, false, false);
            g.streams.push_back(s);
        }
        out->push_back(g);
    }
    if (!ok)
        for (const Group& g : *out)
            for (size_t i = 0; i < g.streams.size(); ++i)
                if (!g.streams[i].err.empty()) printf("FAIL directed %s stream %zu: %s\n", g.name, i, g.streams[i].err.c_str());
    return ok;
}

static void print_set(const char* name, const std::vector<uint32_t>& v) {
    std::vector<uint32_t> u(v);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    printf(", \"%s\": [", name);
    for (size_t i = 0; i < u.size(); ++i) printf("%s%u", i ? ", " : "", u[i]);
    printf("]");
}

static int mode_directed(const char* cases_out) {
    uint8_t fse[TAMD_FSE_BYTES];
    tamd_fse_blob(fse);
    std::vector<Group> groups;
    if (!directed_groups(fse, &groups)) {
        printf("FAIL the generator could not make a case\n");
        return 1;
    }
    FILE* fo = cases_out ? fopen(cases_out, "wb") : nullptr;
    if (cases_out && !fo) return fail("cannot write the cases", 0, 0);
    uint32_t n_streams = 0;
    for (const Group& g : groups) n_streams += (uint32_t)g.streams.size();
    if (fo) {
        fwrite("UNLZ", 1, 4, fo);
        fwrite(&n_streams, 4, 1, fo);
    }
    size_t si = 0;
    for (const Group& g : groups) {
        unsigned long long before[TAMD_CNT_ALL], c[TAMD_CNT_ALL];
        memcpy(before, g_cnt, sizeof(before));
        std::vector<uint32_t> nseq, chunks, lit_type, n_str, lit_sel, bytes, nbig;
        unsigned long long n_blocks = 0;
        for (const Gen& s : g.streams) {
            std::vector<Seen> seen;
            if (run_pair(s.blocks, &s.want, s.max, si++, g.name, &seen)) return 1;
            std::vector<Case> cs(s.blocks.size());
            for (size_t k = 0; k < s.blocks.size(); ++k) {
                cs[k].msg = s.blocks[k];
                cs[k].restored = s.want[k].data;
                if (!s.blocks[k].is_block) continue;
                ++n_blocks;
                const Seen& e = seen[k];
                nseq.push_back(e.nseq);
                chunks.push_back((e.nseq + TAMD_UNLZ_CHUNK - 1u) / TAMD_UNLZ_CHUNK);
                lit_type.push_back(e.lit_type);
                bytes.push_back((uint32_t)s.blocks[k].data.size());
                if (e.lit_type >= 2) {
                    n_str.push_back(e.n_streams);
                    lit_sel.push_back(e.lit_sel);
                }
                if (e.lit_type == 2) nbig.push_back(e.nbig ? 1u : 0u);
            }
            if (fo) write_cases(fo, s.max, cs, true);
        }
        for (int i = 0; i < TAMD_CNT_ALL; ++i) c[i] = g_cnt[i] - before[i];
        printf("{\"group\": \"%s\", \"streams\": %zu, \"blocks\": %llu", g.name, g.streams.size(), n_blocks);
        print_set("nseq", nseq);
        print_set("chunks", chunks);
        print_set("lit_type", lit_type);
        print_set("huf_streams", n_str);
        print_set("lit_sel", lit_sel);
        print_set("huf_big_symbol", nbig);
        print_set("block_bytes", bytes);
        printf(", \"paths\": {");
        print_counters(c, ", ");
        printf("}, \"waits\": {");
        for (int i = TAMD_CNT_N; i < TAMD_CNT_ALL; ++i) printf("%s\"%s\": %llu", i > TAMD_CNT_N ? ", " : "", kWaitName[i - TAMD_CNT_N], c[i]);
        printf("}}\n");
    }
    if (fo) fclose(fo);
    printf("ok\n");
    return 0;
}

// ---- which paths a set of inputs reaches -------------------------------------------------------
struct Input {
    uint32_t max;
    std::vector<Msg> blocks;
    std::vector<Msg> want;  // the messages, where they are known (else empty)
    std::string from;
    bool rejects = false;   // the last message is a block to be rejected (sens only)
};

// The reference's blocks of a stream file (`limit` > 0: the first `limit` messages of each), then
// the streams of block files (blocks=) and case files (cases=) as they are.
static bool collect_inputs(int argc, char** argv, size_t limit, std::vector<Input>* out) {
    std::vector<Stream> streams;
    if (!read_streams(argv[2], &streams) || streams.empty()) return false;
    for (const Stream& st : streams) {
        Input in;
        in.max = st.max;
        in.blocks = ref_blocks(st);
        in.want = st.msgs;
        if (limit && in.blocks.size() > limit) {
            in.blocks.resize(limit);
            in.want.resize(limit);
        }
        in.from = argv[2];
        out->push_back(in);
    }
    for (int i = 3; i < argc; ++i) {
        const std::string a = argv[i];
        const bool cases = a.compare(0, 6, "cases=") == 0;
        if (!cases && a.compare(0, 7, "blocks=") != 0) continue;
        std::vector<Stream> more;
        const char* path = argv[i] + (cases ? 6 : 7);
        if (!read_streams(path, &more, cases)) return false;
        for (const Stream& st : more) {
            Input in;
            in.max = st.max;
            in.blocks = st.msgs;
            in.from = path;
            out->push_back(in);
        }
    }
    return true;
}

static int mode_reach(int argc, char** argv) {
    std::vector<Input> inputs;
    if (!collect_inputs(argc, argv, 0, &inputs)) return fail("cannot read the inputs", 0, 0);
    for (size_t s = 0; s < inputs.size(); ++s)
        if (run_pair(inputs[s].blocks, inputs[s].want.empty() ? nullptr : &inputs[s].want, inputs[s].max, s, "block rejected")) return 1;
    for (int i = 0; i < TAMD_CNT_N; ++i) printf("path %s %llu\n", kCntName[i], g_cnt[i]);
    for (int i = TAMD_CNT_N; i < TAMD_CNT_ALL; ++i) printf("wait %s %llu\n", kWaitName[i - TAMD_CNT_N], g_cnt[i]);
    printf("ok\n");
    return 0;
}

// ---- the reader on 64 emulated lanes -----------------------------------------------------------
// Every lane is a fibre that runs the kernel's message loop (unlz.hip, restated in emu_lane) and
// calls unlz.h with (lane, 64).  A sync hands control back to the scheduler; when every lane has
// arrived the scheduler starts the next phase, one lane after the other in the order of the run.
// Any order of the lanes between two syncs is a legal execution of a wave, so a phase that reads
// what another lane of the same phase writes gives wrong bytes here, every time.
//
// A sync in code that only one lane runs (lane 0 builds the Huffman weights' table by itself with
// nl = 1) holds nobody up on the device, where the other lanes wait at the branch's end: a lane
// found at another site than the rest is run on alone until it joins them.
struct Site {
    const char* func;
    int line;
};
static bool same_site(const Site& a, const Site& b) { return a.line == b.line && strcmp(a.func, b.func) == 0; }

struct Emu {
    static const uint32_t NL = 64, STACK = 256u << 10;
    ucontext_t sched, lane[NL];
    char* stacks = nullptr;
    bool active = false, done[NL];
    Site at[NL];
    uint32_t cur = 0, rng = 1;
    Site skip = {"", -1};
    std::vector<Site> reached;
    void (*body)(uint32_t) = nullptr;
};
static Emu g_emu;

static void emu_sync(const char* func, int line) {
    Emu& E = g_emu;
    if (!E.active) return;
    if (line == E.skip.line && strcmp(func, E.skip.func) == 0) return;
    E.at[E.cur].func = func;
    E.at[E.cur].line = line;
    swapcontext(&E.lane[E.cur], &E.sched);
}

static void emu_entry(unsigned lane) {
    g_emu.body(lane);
    g_emu.done[lane] = true;
}

// Runs `body` on 64 lanes; order 0: ascending, 1: descending, 2: a shuffle redrawn at every sync.
// False when the lanes did not stay together (possible only with a site skipped).
static bool emu_run(void (*body)(uint32_t), int order, uint32_t seed) {
    Emu& E = g_emu;
    if (!E.stacks) E.stacks = (char*)malloc((size_t)Emu::NL * Emu::STACK);
    E.body = body;
    E.rng = seed * 2654435761u + 1u;
    for (uint32_t l = 0; l < Emu::NL; ++l) {
        getcontext(&E.lane[l]);
        E.lane[l].uc_stack.ss_sp = E.stacks + (size_t)l * Emu::STACK;
        E.lane[l].uc_stack.ss_size = Emu::STACK;
        E.lane[l].uc_link = &E.sched;
        makecontext(&E.lane[l], (void (*)())emu_entry, 1, (unsigned)l);
        E.done[l] = false;
    }
    E.active = true;
    bool together = true;
    uint32_t perm[Emu::NL];
    for (;;) {
        for (uint32_t l = 0; l < Emu::NL; ++l) perm[l] = order == 1 ? Emu::NL - 1u - l : l;
        if (order == 2)
            for (uint32_t l = Emu::NL - 1u; l > 0; --l) {
                E.rng = E.rng * 1664525u + 1013904223u;
                std::swap(perm[l], perm[(E.rng >> 8) % (l + 1u)]);
            }
        for (uint32_t i = 0; i < Emu::NL; ++i) {
            E.cur = perm[i];
            swapcontext(&E.sched, &E.lane[E.cur]);
        }
        // where the most lanes stand is where the wave stands
        uint32_t best = 0, best_n = 0, n_done = 0;
        for (uint32_t l = 0; l < Emu::NL; ++l) {
            if (E.done[l]) {
                ++n_done;
                continue;
            }
            uint32_t n = 0;
            for (uint32_t m = 0; m < Emu::NL; ++m) n += !E.done[m] && same_site(E.at[l], E.at[m]);
            if (n > best_n) {
                best_n = n;
                best = l;
            }
        }
        if (n_done == Emu::NL) break;
        if (n_done || best_n <= Emu::NL / 2u) {
            together = false;
            break;
        }
        const Site here = E.at[best];
        for (uint32_t i = 0; i < Emu::NL && together; ++i) {
            E.cur = perm[i];
            for (uint32_t tries = 0; !same_site(E.at[E.cur], here); ++tries) {
                if (tries > 100000u) together = false;
                else swapcontext(&E.sched, &E.lane[E.cur]);
                if (E.done[E.cur]) together = false;
                if (!together) break;
            }
        }
        if (!together) break;
        bool known = false;
        for (const Site& s : E.reached) known = known || same_site(s, here);
        if (!known) E.reached.push_back(here);
    }
    E.active = false;
    return together;
}

// One stream as the kernel's job sees it.  `pad`: bytes behind every buffer (a run with a site
// skipped may decode nonsense; most of it then shows as wrong bytes and not as a fault).
struct EmuJob {
    uint32_t cap = 0;
    const std::vector<Msg>* msgs = nullptr;
    tamd_unlz_state* S = nullptr;
    tamd_unlz_work* W = nullptr;
    uint8_t *ring = nullptr, *lit = nullptr, *big = nullptr, *blk = nullptr, *in = nullptr, *out = nullptr;
    std::vector<size_t> in_at;
    std::vector<int32_t> status;
    std::vector<uint32_t> restored;
    std::vector<Seen> state;
};
static EmuJob g_job;

// unlz.hip's loop over a job's messages (a fresh stream; every message has an output slot).
static void emu_lane(uint32_t lane) {
    EmuJob& J = g_job;
    tamd_unlz_state* S = J.S;
    if (lane == 0) tamd_unlz_reset(S);
    emu_sync("message_loop", 1);
    for (size_t mi = 0; mi < J.msgs->size(); ++mi) {
        const Msg& m = (*J.msgs)[mi];
        const uint32_t n = (uint32_t)m.data.size();
        int32_t rc = S->failed ? TAMD_UNLZ_E_FAILED : (n == 0 || n > J.cap) ? TAMD_UNLZ_E_SIZE : TAMD_UNLZ_OK;
        uint32_t r = 0;
        if (!rc) {
            uint8_t* const o = J.out + mi * (size_t)J.cap;
            const uint8_t* src = J.in + J.in_at[mi];
            if (lane == 0) tamd_unlz_place(S, J.cap);
            if (m.is_block) {
                if (n <= TAMD_LZ_MAX_MESSAGE) {
                    for (uint32_t i = 4u * lane; i < n; i += 256u) memcpy(J.blk + i, src + i, 4);
                    src = J.blk;
                }
                emu_sync("message_loop", 2);
                rc = tamd_unlz_block(S, J.W, J.ring, src, n, J.cap, o, J.lit, TAMD_LZ_MAX_MESSAGE, J.big, J.cap, lane, Emu::NL, &r);
            } else {
                emu_sync("message_loop", 3);
                tamd_unlz_insert(S, J.ring, src, n, o, lane, Emu::NL);
                r = n;
            }
        }
        if (lane == 0) {
            J.status[mi] = rc;
            J.restored[mi] = rc ? 0u : r;
            if (rc && !S->failed) S->failed = rc;
            for (int i = 0; i < 3; ++i) J.state[mi].rep[i] = S->rep[i];
            J.state[mi].next = S->next;
            J.state[mi].dict_len = S->dict_len;
        }
        emu_sync("message_loop", 4);
    }
}

// One input on the lanes in one order against what the walk saw; null when all is equal.
static const char* emu_input(const Input& in, const std::vector<Seen>& want, int order, uint32_t seed, size_t pad, size_t* where) {
    EmuJob& J = g_job;
    const size_t n_msgs = in.blocks.size();
    J.cap = in.max;
    J.msgs = &in.blocks;
    J.in_at.assign(n_msgs, 0);
    size_t in_bytes = 0;
    for (size_t k = 0; k < n_msgs; ++k) {
        J.in_at[k] = in_bytes;
        in_bytes += in.blocks[k].data.size() + 32;  // (the device's input has 32 readable bytes behind it)
    }
    const size_t out_bytes = n_msgs * (size_t)in.max;
    // (LDS is not cleared on the device: the state and the working memory start as garbage)
    J.S = (tamd_unlz_state*)malloc(sizeof(tamd_unlz_state));
    J.W = (tamd_unlz_work*)malloc(sizeof(tamd_unlz_work));
    memset(J.S, 0xEE, sizeof(tamd_unlz_state));
    // (with a site skipped the working memory starts as zeros: a lane that ran ahead on garbage
    // counts would not come to an end, and what it read of the block before shows the same)
    memset(J.W, pad > 64 ? 0 : 0xEE, sizeof(tamd_unlz_work));
    J.ring = (uint8_t*)calloc(1, TAMD_UNLZ_RING + pad);
    J.lit = (uint8_t*)calloc(1, TAMD_LZ_MAX_MESSAGE + pad);
    J.big = (uint8_t*)calloc(1, in.max + pad);
    J.blk = (uint8_t*)calloc(1, TAMD_LZ_MAX_MESSAGE + 16 + pad);
    J.in = (uint8_t*)calloc(1, in_bytes + pad);
    J.out = (uint8_t*)malloc(out_bytes + pad);
    memset(J.out, 0xA5, out_bytes + pad);
    for (size_t k = 0; k < n_msgs; ++k) memcpy(J.in + J.in_at[k], in.blocks[k].data.data(), in.blocks[k].data.size());
    J.status.assign(n_msgs, 1);
    J.restored.assign(n_msgs, 0);
    J.state.assign(n_msgs, Seen());
    const char* diff = nullptr;
    *where = 0;
    if (!emu_run(emu_lane, order, seed)) diff = "the lanes did not stay together";
    for (size_t k = 0; k < n_msgs && !diff; ++k) {
        const uint8_t* o = J.out + k * (size_t)in.max;
        const Seen& w = want[k];
        *where = k;
        if (J.status[k] != w.status) diff = "status";
        else if (J.restored[k] != w.bytes.size()) diff = "restored length";
        else if (memcmp(o, w.bytes.data(), w.bytes.size())) diff = "restored bytes";
        else if (memcmp(J.state[k].rep, w.rep, sizeof(w.rep))) diff = "repeat offsets";
        else if (J.state[k].next != w.next || J.state[k].dict_len != w.dict_len) diff = "ring offset or dictionary length";
        else
            for (size_t i = w.bytes.size(); i < in.max && !diff; ++i)
                if (o[i] != 0xA5) diff = "a byte written behind the message";
    }
    free(J.S);
    free(J.W);
    free(J.ring);
    free(J.lit);
    free(J.big);
    free(J.blk);
    free(J.in);
    free(J.out);
    return diff;
}

// The walk and the reference over every input: what the lanes must reproduce.
static int lanes_expect(const std::vector<Input>& inputs, std::vector<std::vector<Seen>>* want) {
    want->resize(inputs.size());
    for (size_t s = 0; s < inputs.size(); ++s)
        if (run_pair(inputs[s].blocks, inputs[s].want.empty() ? nullptr : &inputs[s].want, inputs[s].max, s, "block rejected", &(*want)[s],
                     inputs[s].rejects))
            return 1;
    return 0;
}

static const char* kOrderName[3] = {"ascending", "descending", "shuffled"};

// Every input in one order; 0 when all equal.
static int lanes_order(const std::vector<Input>& inputs, const std::vector<std::vector<Seen>>& want, int order, size_t pad) {
    for (size_t s = 0; s < inputs.size(); ++s) {
        size_t k = 0;
        const char* diff = emu_input(inputs[s], want[s], order, (uint32_t)s, pad, &k);
        if (diff) {
            printf("DIFF %s order: input %zu (%s, max %u), message %zu: %s\n", kOrderName[order], s, inputs[s].from.c_str(), inputs[s].max, k, diff);
            fflush(stdout);
            return 1;
        }
    }
    return 0;
}

static bool parse_site(const char* arg, std::string* func, Site* site) {
    const char* colon = strchr(arg, ':');
    if (!colon) return false;
    func->assign(arg, colon);
    site->func = func->c_str();
    site->line = atoi(colon + 1);
    return true;
}

static int mode_lanes(int argc, char** argv) {
    std::vector<Input> inputs;
    if (!collect_inputs(argc, argv, 0, &inputs)) return fail("cannot read the inputs", 0, 0);
    std::string func;
    bool skipping = false;
    for (int i = 3; i < argc; ++i)
        if (strncmp(argv[i], "skip=", 5) == 0) skipping = parse_site(argv[i] + 5, &func, &g_emu.skip);
    std::vector<std::vector<Seen>> want;
    if (lanes_expect(inputs, &want)) return 1;
    size_t n_msgs = 0;
    for (const Input& in : inputs) n_msgs += in.blocks.size();
    fflush(stdout);
    // the three orders side by side, a process each
    pid_t pid[3];
    for (int order = 0; order < 3; ++order) {
        pid[order] = fork();
        if (pid[order] == 0) _exit(lanes_order(inputs, want, order, skipping ? (4u << 20) : 64u));
    }
    int bad = 0;
    for (int order = 0; order < 3; ++order) {
        int st = 0;
        waitpid(pid[order], &st, 0);
        if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
            printf("FAIL %s order%s\n", kOrderName[order], WIFEXITED(st) ? "" : ": the run ended by a signal");
            ++bad;
        }
    }
    printf("lanes: %zu streams, %zu messages, 3 orders\n", inputs.size(), n_msgs);
    if (bad) return 1;
    printf("ok\n");
    return 0;
}

static int mode_sens(int argc, char** argv) {
    std::vector<Input> inputs;
    if (!collect_inputs(argc, argv, 40, &inputs)) return fail("cannot read the inputs", 0, 0);
    {
        // The sync behind the Huffman streams carries the streams' verdicts to all lanes (the
        // literals themselves are read behind later syncs), and a verdict differs from 0 only in
        // a block that is rejected: the one such block of this mode.  A directed block with four
        // Huffman streams gets a byte of its second stream changed until the walk finds the
        // stream not consumed exactly (and the reference rejects the block as well).
        uint8_t fse[TAMD_FSE_BYTES];
        tamd_fse_blob(fse);
        Gen s(4000, 77, fse);
        s.plain(600, 0);
        if (!s.block({Seq{1200, 4, 100}}, 0, 0, true)) return fail("sens: the Huffman block", 0, 0);
        Input in;
        in.max = s.max;
        in.from = "a rejected Huffman stream";
        in.rejects = true;
        bool found = false;
        const uint32_t third = (uint32_t)s.blocks.back().data.size() / 3u;
        for (uint32_t at = third; at < third + 40u && !found; ++at) {
            in.blocks = s.blocks;
            in.blocks.back().data[at] ^= 0x5a;
            Walk wk(s.max);
            RefDec rd(s.max);
            Bytes a;
            wk.feed(in.blocks[0], &a);
            rd.feed(in.blocks[0], &a);
            found = wk.feed(in.blocks[1], &a) == TAMD_UNLZ_E_HUFSTREAM && wk.W->n_streams == 4 && rd.feed(in.blocks[1], &a) <= 0;
        }
        if (!found) return fail("sens: no rejected Huffman stream", 0, 0);
        inputs.push_back(in);
    }
    // (the directed corpus and the rewrites first: they find most differences at once)
    std::stable_sort(inputs.begin(), inputs.end(), [&](const Input& a, const Input& b) { return a.want.empty() && !b.want.empty(); });
    std::vector<std::vector<Seen>> want;
    if (lanes_expect(inputs, &want)) return 1;
    // the sites reached: one run with nothing skipped (which must itself be clean)
    if (lanes_order(inputs, want, 0, 64)) return 1;
    const std::vector<Site> sites = g_emu.reached;
    fflush(stdout);
    const size_t jobs = 8;
    std::vector<pid_t> pids(sites.size(), 0);
    std::vector<int> verdict(sites.size(), -1);  // 0: no difference, 1: a difference, 2: ended by a signal
    size_t started = 0, running = 0, finished = 0;
    while (finished < sites.size()) {
        while (started < sites.size() && running < jobs) {
            const pid_t p = fork();
            if (p == 0) {
                g_emu.skip = sites[started];
                alarm(100);
                int differs = 0;
                for (int order = 0; order < 3 && !differs; ++order) differs = lanes_order(inputs, want, order, 4u << 20);
                _exit(differs);
            }
            pids[started++] = p;
            ++running;
        }
        int st = 0;
        const pid_t p = wait(&st);
        for (size_t i = 0; i < started; ++i)
            if (pids[i] == p) {
                verdict[i] = WIFEXITED(st) ? WEXITSTATUS(st) : 2;
                --running;
                ++finished;
            }
    }
    for (size_t i = 0; i < sites.size(); ++i)
        printf("site %s %d %s\n", sites[i].func, sites[i].line,
               verdict[i] == 0 ? "unneeded" : verdict[i] == 1 ? "necessary" : "necessary (the run without it ended by a signal)");
    printf("ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "directed") return mode_directed(argc > 2 ? argv[2] : nullptr);
    if (argc >= 3 && std::string(argv[1]) == "lanes") return mode_lanes(argc, argv);
    if (argc >= 3 && std::string(argv[1]) == "sens") return mode_sens(argc, argv);
    if (argc >= 3 && std::string(argv[1]) == "reach") return mode_reach(argc, argv);
    if (argc >= 2 && std::string(argv[1]) == "tables") return mode_tables();
    if (argc >= 2 && std::string(argv[1]) == "ring") return mode_ring();
    if (argc < 3) {
        printf("usage: unlz_check tables | ring | directed [<cases out>] | check|mutants|bench|lanes|sens|reach <streams> ...\n");
        return 2;
    }
    std::vector<Stream> streams;
    if (!read_streams(argv[2], &streams) || streams.empty()) {
        printf("FAIL cannot read %s\n", argv[2]);
        return 2;
    }
    const std::string mode = argv[1];
    if (mode == "check") return mode_check(streams, argc > 3 ? argv[3] : nullptr);
    if (mode == "mutants") return mode_mutants(streams, argc > 3 ? argv[3] : nullptr);
    if (mode == "bench") return mode_bench(streams, argc > 3 ? (unsigned)atoi(argv[3]) : 16u, argc > 4 && atoi(argv[4]) > 0 ? (unsigned)atoi(argv[4]) : 3u);
    return 2;
}
