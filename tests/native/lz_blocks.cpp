// lz_blocks.cpp -- TEST ONLY.  A host checker of what the compressor returned (the kernel of
// tonk_amd/csrc/lz.hip through either API, or the host compressor of lz_host.h): every block is
// read back with the project's own block reader (tonk_amd/csrc/unlz.h, one "lane") and held
// against the message, the history-ring rule and the host block writer.  Needs no reference
// library.
//
//   lz_blocks check <cases>
//       Per stream the messages go through a decoder state in order (a block through
//       tamd_unlz_block, a message sent as is through tamd_unlz_insert) with RingTrack (lz.h)
//       beside it for each message's linear position and window start, over the linear stream (the
//       messages end to end).  Per block, in this order:
//         block form   the reader accepts the block and restores the message
//         acceptance   the block is at most min(len - 1, max) bytes
//         literals     the literals section is Raw
//         offsets      no repeat offsets: every Offset_Value is above 3 (of the reader's offset
//                      counters only TAMD_CNT_OFF_NEW moves)
//         sequences    every match length is at least 4; literal and match lengths sum to len
//         window       every match source starts at or after the message's window start and
//                      before the match
//         maximality   every match ends at the message's end, or the byte after it differs from
//                      the byte after its source.  The kernel has no case of a legitimately
//                      shorter match: a probe is cut only by the message's end (lim = n - i), a
//                      probe that matched in full is extended to the first difference or the
//                      message's end whichever chunk it began in, and the parse takes a match
//                      word as it stands.  Nothing is exempt.
//         rewrite      the sequences read back, written again by lz_host_write (tamd_seq_choose,
//                      the header words, the descriptions in LL, OF, ML order,
//                      tamd_fse_sequences_t), give the block byte for byte and its size
//       Prints one JSON line per stream (the reach record, "ok" and the first failure's reason
//       with its message) and a total; exit status 1 when any stream failed.
//   lz_blocks host <streams> <cases out> [huffman=0|1] [minmatch=N] [fitted=0|1] [len_cap=N]
//                                        [slack=N] [win_back=N] [flip=1]
//       The host compressor of lz_host.h over a stream file's messages, written as a case file
//       (the defaults: raw literals, everything else as the kernel does it).  flip=1: one bit of
//       a table description flipped in each stream's first block with a fitted table.
//
// Case files (unlz_check's layout): "UNLZ", u32 streams; per stream u32 max, u32 messages; per
// message u32 is_block, u32 bytes, the bytes (the block, or the message when it was sent as is),
// i32 status (0), u32 restored, the restored bytes (a block's message).
static unsigned long long g_cnt[64];
#define TAMD_UNLZ_COUNT(what) (++g_cnt[what])
#include "../../tonk_amd/csrc/unlz.h"
#include "lz_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;
struct Msg {
    bool is_block = false;
    Bytes data;     // the block, or the message sent as is
    Bytes message;  // a block's message
};
struct Stream {
    uint32_t max = 0;
    std::vector<Msg> msgs;
};

static bool read_file(const char* path, bool cases, std::vector<Stream>* out) {
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
            uint32_t isb = 0, len = 0, r = 0;
            int32_t status = 0;
            ok = fread(&isb, 4, 1, f) == 1 && fread(&len, 4, 1, f) == 1 && len <= (1u << 20);
            Msg g;
            g.is_block = isb != 0;
            g.data.resize(len);
            if (ok && len) ok = fread(g.data.data(), 1, len, f) == len;
            if (ok && cases) {
                ok = fread(&status, 4, 1, f) == 1 && fread(&r, 4, 1, f) == 1 && r <= (1u << 20);
                g.message.resize(r);
                if (ok && r) ok = fread(g.message.data(), 1, r, f) == r;
            }
            st.msgs.push_back(g);
        }
        out->push_back(st);
    }
    fclose(f);
    return ok;
}

static void write_file(FILE* f, const std::vector<Stream>& streams) {
    const uint32_t n = (uint32_t)streams.size();
    fwrite("UNLZ", 1, 4, f);
    fwrite(&n, 4, 1, f);
    for (const Stream& st : streams) {
        const uint32_t m = (uint32_t)st.msgs.size();
        fwrite(&st.max, 4, 1, f);
        fwrite(&m, 4, 1, f);
        for (const Msg& g : st.msgs) {
            const uint32_t isb = g.is_block, len = (uint32_t)g.data.size(), r = (uint32_t)g.message.size();
            const int32_t status = 0;
            fwrite(&isb, 4, 1, f);
            fwrite(&len, 4, 1, f);
            if (len) fwrite(g.data.data(), 1, len, f);
            fwrite(&status, 4, 1, f);
            fwrite(&r, 4, 1, f);
            if (r) fwrite(g.message.data(), 1, r, f);
        }
    }
}

// One stream's decoder with buffers of exactly the sizes the reader may touch.
struct Walk {
    uint32_t max;
    tamd_unlz_state *S, *S2;  // S2: the copy the sequences are read back through
    tamd_unlz_work* W;
    uint8_t *ring, *lit, *out;
    explicit Walk(uint32_t mx) : max(mx) {
        S = (tamd_unlz_state*)malloc(sizeof(tamd_unlz_state));
        S2 = (tamd_unlz_state*)malloc(sizeof(tamd_unlz_state));
        W = (tamd_unlz_work*)malloc(sizeof(tamd_unlz_work));
        ring = (uint8_t*)malloc(TAMD_UNLZ_RING);
        lit = (uint8_t*)malloc(mx);
        out = (uint8_t*)malloc(mx);
        memset(S, 0, sizeof(*S));
        memset(W, 0, sizeof(*W));
        memset(ring, 0, TAMD_UNLZ_RING);
        tamd_unlz_reset(S);
    }
    ~Walk() {
        free(S);
        free(S2);
        free(W);
        free(ring);
        free(lit);
        free(out);
    }
    Walk(const Walk&) = delete;
};

// The reach record of a stream (and, merged, of the file).
struct Record {
    unsigned long long blocks[2] = {0, 0}, as_is[2] = {0, 0};  // len <= TAMD_LZ_MAX_MESSAGE, above
    unsigned long long modes[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // LL, ML, OF x predefined, RLE, fitted
    std::set<uint32_t> nseq_seen;
    unsigned long long seq_header[2] = {0, 0};  // one-byte, two-byte sequence count
    unsigned long long lit_header[3] = {0, 0, 0}, no_literals = 0;
    uint32_t off_max = 0, off_min = ~0u;
    unsigned long long dist1 = 0, overlap = 0, ext_match = 0, ext_cross = 0, restarts = 0;
    uint32_t code_max[3] = {0, 0, 0};  // LL, ML, OF
    unsigned long long ml_over_16 = 0, ml_over_528 = 0, ml_whole[2] = {0, 0};
    unsigned long long src_pos_max = 0, msg_pos_max = 0;
    unsigned long long seqs = 0, seqs_past_64k = 0;  // the latter: in messages at linear positions above 65535
    unsigned long long src_cross_64k = 0, dst_cross_64k = 0;  // matches whose source / target crosses a multiple of 65536
    unsigned long long in_bytes = 0, out_bytes = 0;
    void merge(const Record& r) {
        for (int i = 0; i < 2; ++i) {
            blocks[i] += r.blocks[i];
            as_is[i] += r.as_is[i];
            seq_header[i] += r.seq_header[i];
            ml_whole[i] += r.ml_whole[i];
        }
        for (int k = 0; k < 3; ++k) {
            for (int m = 0; m < 3; ++m) modes[k][m] += r.modes[k][m];
            lit_header[k] += r.lit_header[k];
            if (r.code_max[k] > code_max[k]) code_max[k] = r.code_max[k];
        }
        nseq_seen.insert(r.nseq_seen.begin(), r.nseq_seen.end());
        no_literals += r.no_literals;
        if (r.off_max > off_max) off_max = r.off_max;
        if (r.off_min < off_min) off_min = r.off_min;
        dist1 += r.dist1;
        overlap += r.overlap;
        ext_match += r.ext_match;
        ext_cross += r.ext_cross;
        restarts += r.restarts;
        ml_over_16 += r.ml_over_16;
        ml_over_528 += r.ml_over_528;
        if (r.src_pos_max > src_pos_max) src_pos_max = r.src_pos_max;
        if (r.msg_pos_max > msg_pos_max) msg_pos_max = r.msg_pos_max;
        seqs += r.seqs;
        seqs_past_64k += r.seqs_past_64k;
        src_cross_64k += r.src_cross_64k;
        dst_cross_64k += r.dst_cross_64k;
        in_bytes += r.in_bytes;
        out_bytes += r.out_bytes;
    }
    void print(const char* lead) const {
        printf("{%s, \"lz_max_message\": %u", lead, TAMD_LZ_MAX_MESSAGE);
        printf(", \"blocks_small\": %llu, \"blocks_big\": %llu, \"as_is_small\": %llu, \"as_is_big\": %llu", blocks[0], blocks[1],
               as_is[0], as_is[1]);
        const char* tn[3] = {"ll", "ml", "of"};
        for (int k = 0; k < 3; ++k)
            printf(", \"%s_modes\": {\"predefined\": %llu, \"rle\": %llu, \"fitted\": %llu}", tn[k], modes[k][0], modes[k][1],
                   modes[k][2]);
        printf(", \"nseq_seen\": [");
        bool first = true;
        for (uint32_t v : nseq_seen) {
            printf("%s%u", first ? "" : ", ", v);
            first = false;
        }
        printf("], \"nseq_max\": %u", nseq_seen.empty() ? 0u : *nseq_seen.rbegin());
        printf(", \"seq_header_1\": %llu, \"seq_header_2\": %llu", seq_header[0], seq_header[1]);
        printf(", \"lit_header_1\": %llu, \"lit_header_2\": %llu, \"lit_header_3\": %llu, \"no_literals\": %llu", lit_header[0],
               lit_header[1], lit_header[2], no_literals);
        printf(", \"off_max\": %u, \"off_min\": %u, \"dist1\": %llu, \"overlap\": %llu", off_max, seqs ? off_min : 0u, dist1,
               overlap);
        printf(", \"ext_match\": %llu, \"ext_cross\": %llu, \"ring_restarts\": %llu", ext_match, ext_cross, restarts);
        printf(", \"ll_code_max\": %u, \"ml_code_max\": %u, \"of_code_max\": %u", code_max[0], code_max[1], code_max[2]);
        printf(", \"ml_over_16\": %llu, \"ml_over_528\": %llu, \"ml_whole_small\": %llu, \"ml_whole_big\": %llu", ml_over_16,
               ml_over_528, ml_whole[0], ml_whole[1]);
        printf(", \"src_pos_max\": %llu, \"msg_pos_max\": %llu, \"sequences\": %llu, \"sequences_past_64k\": %llu", src_pos_max,
               msg_pos_max, seqs, seqs_past_64k);
        printf(", \"src_cross_64k\": %llu, \"dst_cross_64k\": %llu, \"in_bytes\": %llu, \"out_bytes\": %llu}\n", src_cross_64k,
               dst_cross_64k, in_bytes, out_bytes);
    }
};

// One stream.  Returns the first failure's reason (null: none) with its message in *at.
static const char* check_stream(const Stream& st, const uint8_t* fse, Record* R, size_t* at) {
    Bytes lin;  // the linear stream
    for (const Msg& m : st.msgs) {
        const Bytes& b = m.is_block ? m.message : m.data;
        lin.insert(lin.end(), b.begin(), b.end());
    }
    Walk wk(st.max);
    RingTrack rt;
    rt.max = st.max;
    std::vector<uint8_t> rewritten;
    for (size_t k = 0; k < st.msgs.size(); ++k) {
        *at = k;
        const Msg& m = st.msgs[k];
        const Bytes& msg = m.is_block ? m.message : m.data;
        const uint32_t n = (uint32_t)msg.size();
        if (n == 0 || n > st.max) return "message size 0 or above the stream's maximum";
        uint64_t pos = 0, win = 0;
        rt.place(n, &pos, &win);
        const int big = n > TAMD_LZ_MAX_MESSAGE;
        const unsigned long long restarts0 = g_cnt[TAMD_CNT_RESTART];
        tamd_unlz_place(wk.S, st.max);
        R->restarts += g_cnt[TAMD_CNT_RESTART] - restarts0;
        if (pos > R->msg_pos_max) R->msg_pos_max = pos;
        R->in_bytes += n;
        if (!m.is_block) {
            tamd_unlz_insert(wk.S, wk.ring, msg.data(), n, wk.out, 0, 1);
            ++R->as_is[big];
            R->out_bytes += n;
            continue;
        }
        // exact copies: the reader must not touch a byte outside the block
        const uint32_t bn = (uint32_t)m.data.size();
        if (bn == 0) return "empty block";
        uint8_t* blk = (uint8_t*)malloc(bn);
        memcpy(blk, m.data.data(), bn);
        struct Free {
            uint8_t* p;
            ~Free() { free(p); }
        } free_blk{blk};
        const uint32_t lit_cap = st.max < TAMD_LZ_MAX_MESSAGE ? st.max : TAMD_LZ_MAX_MESSAGE;
        // ---- block form: the sequences are read back on a copy of the state first (its counts
        // are put back: the walk's are the record)
        unsigned long long saved[64];
        memcpy(saved, g_cnt, sizeof(saved));
        memcpy(wk.S2, wk.S, sizeof(tamd_unlz_state));
        std::vector<uint32_t> lo, off;
        int32_t rc = tamd_unlz_lit_header(blk, bn, st.max, wk.W);
        const uint32_t lit_type = wk.W->lit_type, lit_n = wk.W->lit_n;
        uint32_t modes = 0, nseq = 0;
        if (!rc && lit_type == 0) {
            wk.W->seq_done = wk.W->lit_used = wk.W->produced = 0;
            for (uint32_t i = 0; i < 3; ++i) wk.W->rep[i] = wk.S2->rep[i];
            rc = tamd_unlz_seq_header(wk.S2, wk.W, blk, bn, 0, 1);
            nseq = wk.W->nseq;
            modes = wk.W->modes;
            while (!rc && wk.W->seq_done < wk.W->nseq) {
                rc = tamd_unlz_seq_chunk(wk.S2, wk.W, blk, st.max, wk.S2->next);
                for (uint32_t c = 0; c < wk.W->chunk_n; ++c) {
                    if (wk.W->seq_ll[c] > 0xffffu || wk.W->seq_ml[c] > 0xffffu) return "a length above 65535";
                    lo.push_back(wk.W->seq_ll[c] | (wk.W->seq_ml[c] << 16));
                    off.push_back(wk.W->seq_off[c]);
                }
            }
        }
        memcpy(g_cnt, saved, sizeof(saved));
        uint32_t restored = 0;
        rc = tamd_unlz_block(wk.S, wk.W, wk.ring, blk, bn, st.max, wk.out, wk.lit, lit_cap, wk.lit, st.max, 0, 1, &restored);
        if (rc) return "block rejected by the reader";
        if (restored != n || memcmp(wk.out, msg.data(), n) != 0) return "block does not restore the message";
        // ---- acceptance rule
        if (bn > (n - 1u < st.max ? n - 1u : st.max)) return "block above min(len - 1, max)";
        // ---- literals
        if (lit_type != 0) return "literals not raw";
        if (nseq == 0 || lo.size() != nseq) return "no sequences";
        // ---- no repeat offsets
        for (int c = TAMD_CNT_REP0; c <= TAMD_CNT_REP_LL0_DEC; ++c)
            if (g_cnt[c] != saved[c]) return "repeat offset";
        if (g_cnt[TAMD_CNT_OFF_NEW] - saved[TAMD_CNT_OFF_NEW] != nseq) return "repeat offset";
        // ---- sequences
        uint64_t total = lit_n;
        uint32_t lits_in_seqs = 0;
        for (uint32_t v : lo) {
            if ((v >> 16) < 4u) return "match below 4";
            total += v >> 16;
            lits_in_seqs += v & 0xffffu;
        }
        if (total != n || lits_in_seqs > lit_n) return "lengths do not sum to the message";
        // ---- window and maximality, in the linear stream
        uint64_t t = pos;
        for (size_t q = 0; q < lo.size(); ++q) {
            const uint32_t ll = lo[q] & 0xffffu, ml = lo[q] >> 16, o = off[q];
            t += ll;
            if (o == 0 || o > t) return "match source before the stream";
            const uint64_t src = t - o;
            if (src < win) return "match source before the window start";
            const uint64_t e = t + ml;
            if (e < pos + n && lin[e] == lin[e - o]) return "match not maximal";
            // the record
            if (o > R->off_max) R->off_max = o;
            if (o < R->off_min) R->off_min = o;
            R->dist1 += o == 1;
            R->ml_over_16 += ml > 16;
            R->ml_over_528 += ml > 16 + 512;
            R->ml_whole[big] += ml == n;
            if (src > R->src_pos_max) R->src_pos_max = src;
            R->src_cross_64k += (src >> 16) != ((src + ml - 1) >> 16);
            R->dst_cross_64k += (t >> 16) != ((e - 1) >> 16);
            const uint32_t cd[3] = {tamd_ll_code(ll), tamd_ml_code(ml), 31u - (uint32_t)__builtin_clz(o + 3u)};
            for (int i = 0; i < 3; ++i)
                if (cd[i] > R->code_max[i]) R->code_max[i] = cd[i];
            t = e;
        }
        // ---- rewrite identity
        LzHostOptions opt;
        opt.huffman = false;
        opt.slack = n;  // (the acceptance rule is checked above: the writer writes whatever the size)
        LzHostStats hs;
        hs.lo = lo;
        hs.off = off;
        const uint32_t w = lz_host_write(msg.data(), n, fse, opt, &rewritten, &hs);
        const uint32_t a = hs.seq_at - hs.hs - hs.dl;  // the literals section's size
        if (!hs.seq_at || bn < hs.seq_at || memcmp(blk, rewritten.data(), a + hs.hs - 1u) != 0)
            return "literals section or sequence count differs from the host writer";
        if (memcmp(blk + a + hs.hs - 1u, rewritten.data() + a + hs.hs - 1u, 1u + hs.dl) != 0)
            return "tables differ from tamd_seq_choose";
        if (w != bn) return "size differs from the host writer's";
        if (memcmp(blk, rewritten.data(), bn) != 0) return "bit stream differs from tamd_fse_sequences_t";
        // ---- the record
        ++R->blocks[big];
        R->out_bytes += bn;
        R->seqs += nseq;
        if (pos > 65535) R->seqs_past_64k += nseq;
        R->nseq_seen.insert(nseq);
        ++R->seq_header[nseq < 128 ? 0 : 1];
        ++R->lit_header[lit_n < 32 ? 0 : lit_n < 4096 ? 1 : 2];
        R->no_literals += lit_n == 0;
        ++R->modes[0][modes >> 6];
        ++R->modes[1][(modes >> 2) & 3u];
        ++R->modes[2][(modes >> 4) & 3u];
        R->overlap += g_cnt[TAMD_CNT_OVERLAP] - saved[TAMD_CNT_OVERLAP];
        R->ext_match += g_cnt[TAMD_CNT_EXT_MATCH] - saved[TAMD_CNT_EXT_MATCH];
        R->ext_cross += g_cnt[TAMD_CNT_EXT_CROSS] - saved[TAMD_CNT_EXT_CROSS];
    }
    return nullptr;
}

static int mode_check(const char* path) {
    std::vector<Stream> streams;
    if (!read_file(path, true, &streams) || streams.empty()) {
        printf("FAIL cannot read %s\n", path);
        return 2;
    }
    uint8_t fse[TAMD_FSE_BYTES];
    tamd_fse_blob(fse);
    Record total;
    size_t failed = 0;
    for (size_t s = 0; s < streams.size(); ++s) {
        Record R;
        size_t at = 0;
        const char* why = check_stream(streams[s], fse, &R, &at);
        char lead[256];
        snprintf(lead, sizeof(lead), "\"stream\": %zu, \"max\": %u, \"messages\": %zu, \"ok\": %s, \"failed_message\": %ld, \"reason\": \"%s\"",
                 s, streams[s].max, streams[s].msgs.size(), why ? "false" : "true", why ? (long)at : -1L, why ? why : "");
        R.print(lead);
        failed += why != nullptr;
        if (!why) total.merge(R);
    }
    char lead[128];
    snprintf(lead, sizeof(lead), "\"total\": true, \"streams\": %zu, \"failed\": %zu, \"ok\": %s", streams.size(), failed,
             failed ? "false" : "true");
    total.print(lead);
    return failed ? 1 : 0;
}

static int mode_host(const char* in, const char* outp, int argc, char** argv) {
    std::vector<Stream> streams;
    if (!read_file(in, false, &streams) || streams.empty()) {
        printf("FAIL cannot read %s\n", in);
        return 2;
    }
    LzHostOptions opt;
    opt.huffman = false;
    bool flip = false;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        const size_t eq = a.find('=');
        if (eq == std::string::npos) return 2;
        const std::string key = a.substr(0, eq);
        const uint32_t v = (uint32_t)strtoul(a.c_str() + eq + 1, nullptr, 10);
        if (key == "huffman") opt.huffman = v != 0;
        else if (key == "minmatch") opt.minmatch = v;
        else if (key == "fitted") opt.fitted = v != 0;
        else if (key == "len_cap") opt.len_cap = v;
        else if (key == "slack") opt.slack = v;
        else if (key == "win_back") opt.win_back = v;
        else if (key == "flip") flip = v != 0;
        else return 2;
    }
    uint8_t fse[TAMD_FSE_BYTES];
    tamd_fse_blob(fse);
    std::vector<Stream> res;
    for (const Stream& st : streams) {
        Bytes lin;
        for (const Msg& m : st.msgs) lin.insert(lin.end(), m.data.begin(), m.data.end());
        lin.resize(lin.size() + 16);
        RingTrack rt;
        rt.max = st.max;
        opt.max = st.max;
        std::vector<int64_t> table(1u << 14, -1);
        Bytes out;
        Stream rs;
        rs.max = st.max;
        bool flipped = !flip;
        for (const Msg& m : st.msgs) {
            const uint32_t n = (uint32_t)m.data.size();
            uint64_t pos = 0, win = 0;
            rt.place(n, &pos, &win);
            LzHostStats hs;
            const uint32_t w = n >= 8 ? lz_host_block(lin.data(), pos, n, win, table, fse, opt, &out, &hs) : 0u;
            Msg b;
            b.is_block = w != 0;
            if (w) {
                b.data.assign(out.begin(), out.begin() + w);
                b.message = m.data;
                if (!flipped && opt.fitted) {
                    // the first description byte of a fitted table: bit 4, the lowest bit of the first count
                    const uint32_t order[3] = {0u, 2u, 1u};
                    uint32_t d = hs.seq_at - hs.dl;
                    for (uint32_t k : order) {
                        if (hs.tt.mode[k] == TAMD_MODE_FSE) {
                            b.data[d] ^= 0x10u;
                            flipped = true;
                            break;
                        }
                        d += hs.tt.desc_len[k];
                    }
                }
            } else {
                b.data = m.data;
            }
            rs.msgs.push_back(b);
        }
        res.push_back(rs);
    }
    FILE* fo = fopen(outp, "wb");
    if (!fo) return 2;
    write_file(fo, res);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (mode == "check" && argc == 3) return mode_check(argv[2]);
    if (mode == "host" && argc >= 4) return mode_host(argv[2], argv[3], argc - 4, argv + 4);
    printf("usage: lz_blocks check <cases> | host <streams> <cases out> [key=value ...]\n");
    return 2;
}
