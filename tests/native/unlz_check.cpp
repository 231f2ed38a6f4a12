// unlz_check.cpp -- TEST ONLY.  A serial host walk of the block reader the decompression kernel
// uses (tonk_amd/csrc/unlz.h alone, one "lane"), against the reference's zstd
// (oracle/_ref/libmsgcodec_ref.so: MessageCompressor / MessageDecompressor restated).
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
//
// Stream files: "UNLZ", u32 streams; per stream u32 max, u32 messages; per message u32 is_block,
// u32 bytes, the bytes.  Case files add per message i32 status, u32 restored, the restored bytes.
static unsigned long long g_cnt[64];
#define TAMD_UNLZ_COUNT(what) (++g_cnt[what])
#include "../../tonk_amd/csrc/unlz.h"
#include "lz_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static bool read_streams(const char* path, std::vector<Stream>* out) {
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
static int run_pair(const std::vector<Msg>& blocks, const std::vector<Msg>* want, uint32_t max, size_t s, const char* what) {
    Walk wk(max);
    RefDec rd(max);
    Bytes a, b;
    for (size_t k = 0; k < blocks.size(); ++k) {
        const int32_t rc = wk.feed(blocks[k], &a);
        const int r = rd.feed(blocks[k], &b);
        if (rc || r <= 0) return fail(what, s, k, rc, r);
        if (a != b) return fail("walk differs from the reference decompressor", s, k);
        if (want && a != (*want)[k].data) return fail("walk differs from the message", s, k);
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

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "tables") return mode_tables();
    if (argc >= 2 && std::string(argv[1]) == "ring") return mode_ring();
    if (argc < 3) {
        printf("usage: unlz_check tables | ring | check|mutants|bench <streams> ...\n");
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
