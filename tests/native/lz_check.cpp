// lz_check.cpp -- TEST ONLY.  Checks the zstd block writer the compression kernel uses (the
// host+device helpers of tonk_amd/csrc/lz.h: FSE tables of the predefined distributions,
// literal/sequence headers, the backward sequence bit stream) against the reference's zstd
// decoder (oracle/_ref/libmsgcodec_ref.so, MessageDecompressor restated over thirdparty/zstd),
// under the host compressor of lz_host.h.  The GPU tests run the kernel itself against the same
// decoder.
//
// usage: lz_check [messages] [seed] [huffman] [minmatch] [fitted]   -> prints "ok <compressed> <total>" or the first mismatch
#include "lz_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" {
void* ref_decomp_new(unsigned max);
void ref_insert(void* d, const uint8_t* data, unsigned bytes);
int ref_decomp(void* d, const uint8_t* src, unsigned bytes, uint8_t* out, unsigned cap);
void ref_decomp_free(void* d);
}

static uint32_t rng_state = 1;
static unsigned fitted_tables[3] = {0, 0, 0}, rle_tables[3] = {0, 0, 0};
static unsigned huffman_blocks = 0;
static uint64_t lit_bytes = 0, seq_bytes = 0, n_seqs = 0, lit_small = 0;
static double est_fitted = 0;  // estimated bytes of the sequence streams with block-fitted tables
#include <math.h>
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

int main(int argc, char** argv) {
    const unsigned n_msgs = argc > 1 ? (unsigned)atoi(argv[1]) : 400;
    rng_state = argc > 2 ? (uint32_t)atoi(argv[2]) : 1;
    LzHostOptions opt;
    if (argc > 3) opt.huffman = atoi(argv[3]) != 0;
    if (argc > 4) opt.minmatch = (uint32_t)atoi(argv[4]);
    if (argc > 5) opt.fitted = atoi(argv[5]) != 0;
    const unsigned kMax = 1300;
    uint8_t fse[TAMD_FSE_BYTES];
    tamd_fse_blob(fse);
    {  // the kernel's packed maps agree with the encoder/decoder tables the host writer uses
        const uint16_t* e16 = (const uint16_t*)(fse + TAMD_FSE_E16);
        const struct { uint32_t enc, dec, e, nsym, size; } t[3] = {
            {TAMD_FSE_LL_ENC, TAMD_FSE_LL_DEC, TAMD_FSE_LL_E16, 36, 64},
            {TAMD_FSE_ML_ENC, TAMD_FSE_ML_DEC, TAMD_FSE_ML_E16, 53, 64},
            {TAMD_FSE_OF_ENC, TAMD_FSE_OF_DEC, TAMD_FSE_OF_E16, 29, 32}};
        for (const auto& c : t)
            for (uint32_t sy = 0; sy < c.nsym; ++sy)
                for (uint32_t y = 0; y < c.size; ++y) {
                    const uint32_t u = fse[c.enc + sy * c.size + y], w = e16[c.e + sy * c.size + y];
                    if ((w & 63u) != u || ((w >> 6) & 15u) != fse[c.dec + 2 * u] || (w >> 10) != y - fse[c.dec + 2 * u + 1]) {
                        printf("packed FSE map differs (symbol %u, state %u)\n", sy, y);
                        return 1;
                    }
                }
    }
    // a stream of messages: words from a small vocabulary, random bytes, repeats of old messages
    std::vector<uint8_t> stream;
    std::vector<unsigned> lens;
    const char* words[] = {"siamese ", "tonk ", "packet ", "recovery ", "window ", "lane ", "sum ", "ack ", "0123 "};
    for (unsigned k = 0; k < n_msgs; ++k) {
        const unsigned n = 8 + rnd() % (kMax - 8);
        const unsigned kind = rnd() % 4;
        const size_t at = stream.size();
        if (kind == 3 && at > 4000) {  // repeat an earlier stretch
            const size_t from = at - 1 - rnd() % (at < 40000 ? at - 1 : 40000);
            for (unsigned i = 0; i < n; ++i) stream.push_back(stream[from + i < at ? from + i : at - 1]);
        } else {
            for (unsigned i = 0; i < n;) {
                if (kind == 0) {
                    stream.push_back((uint8_t)rnd());
                    ++i;
                } else if (kind == 2) {  // novel text: skewed letters (Huffman-coded literals)
                    const uint32_t r = rnd() % 100;
                    stream.push_back((uint8_t)(r < 40 ? 'e' + r % 4 : r < 80 ? 'a' + r % 12 : ' ' + r % 64));
                    ++i;
                } else {
                    const char* w = words[rnd() % 9];
                    for (const char* c = w; *c && i < n; ++c, ++i) stream.push_back((uint8_t)*c);
                }
            }
        }
        lens.push_back(n);
    }
    void* dec = ref_decomp_new(kMax);
    RingTrack ring;
    ring.max = kMax;
    std::vector<int64_t> table(1u << 14, -1);
    uint64_t total_in = 0, total_out = 0;
    unsigned compressed = 0;
    std::vector<uint8_t> out, got(kMax + 64);
    const uint8_t* s = stream.data();
    for (unsigned k = 0; k < n_msgs; ++k) {
        const unsigned n = lens[k];
        uint64_t pos = 0, win = 0;
        ring.place(n, &pos, &win);
        LzHostStats st;
        const unsigned w = lz_host_block(s, pos, n, win, table, fse, opt, &out, &st);
        const std::vector<uint32_t>&lo = st.lo, &off = st.off;
        if (!lo.empty()) {
            lit_bytes += st.lits;
            n_seqs += lo.size();
            if (st.small) lit_small += st.lits;
            huffman_blocks += st.huffman;
            for (uint32_t k = 0; opt.fitted && k < 3; ++k) {
                if (st.tt.mode[k] == TAMD_MODE_FSE) ++fitted_tables[k];
                if (st.tt.mode[k] == TAMD_MODE_RLE) ++rle_tables[k];
            }
        }
        if (st.seq_room) {
            if (!opt.fitted) {  // the packed-map writer agrees with the table writer
                std::vector<uint8_t> alt(n);
                const uint32_t nb2 = tamd_fse_sequences(lo.data(), off.data(), (uint32_t)lo.size(), fse, alt.data(), st.seq_room);
                if (nb2 != st.seq_bytes || memcmp(alt.data(), &out[st.seq_at], nb2) != 0) {
                    printf("sequence writers differ at message %u\n", k);
                    return 1;
                }
            }
            seq_bytes += st.seq_bytes + st.hs + st.dl;
            {  // entropy of the three code streams per block + the same extra bits + ~8 B of table headers each
                uint32_t hl[64] = {0}, hm[64] = {0}, ho[32] = {0};
                double extra = 0;
                for (size_t q = 0; q < lo.size(); ++q) {
                    const uint32_t llc = tamd_ll_code(lo[q] & 0xffffu), mlc = tamd_ml_code(lo[q] >> 16);
                    const uint32_t ofc = 31u - (uint32_t)__builtin_clz(off[q] + 3u);
                    ++hl[llc]; ++hm[mlc]; ++ho[ofc];
                    extra += tamd_ll_bits(llc) + tamd_ml_bits(mlc) + ofc;
                }
                auto ent = [&](const uint32_t* h, int k) {
                    double e = 0, t = (double)lo.size();
                    for (int i = 0; i < k; ++i) if (h[i]) e -= h[i] * log2(h[i] / t);
                    return e;
                };
                est_fitted += (ent(hl, 64) + ent(hm, 64) + ent(ho, 32) + extra) / 8.0 + 3 * 8 + st.hs;
            }
        }
        if (w) {
            const int r = ref_decomp(dec, out.data(), w, got.data(), (unsigned)got.size());
            if (r != (int)n || memcmp(got.data(), s + pos, n) != 0) {
                printf("mismatch at message %u (n %u, block %u bytes, %zu sequences, rc %d)\n", k, n, w, lo.size(), r);
                return 1;
            }
            ++compressed;
            total_out += w;
        } else {
            ref_insert(dec, s + pos, n);
            total_out += n;
        }
        total_in += n;
    }
    ref_decomp_free(dec);
    fprintf(stderr, "sequence sections now %llu bytes, with block-fitted tables about %.0f\n",
            (unsigned long long)seq_bytes, est_fitted);
    fprintf(stderr, "literal bytes %llu (in Huffman-able sections %llu), sequences %llu in %llu bytes\n",
            (unsigned long long)lit_bytes, (unsigned long long)lit_small, (unsigned long long)n_seqs,
            (unsigned long long)seq_bytes);
    fprintf(stderr, "fitted tables LL/ML/OF %u/%u/%u, RLE %u/%u/%u\n", fitted_tables[0], fitted_tables[1],
            fitted_tables[2], rle_tables[0], rle_tables[1], rle_tables[2]);
    printf("ok %u/%u compressed (%u with Huffman literals), %llu -> %llu bytes\n", compressed, n_msgs,
           huffman_blocks, (unsigned long long)total_in, (unsigned long long)total_out);
    return 0;
}
