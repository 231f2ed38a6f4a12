// recv_check -- the byte and state logic of the receive front (tonk_amd/csrc/recv.h) as a serial
// host walk.  Test-only; built plain and under the address and undefined-behaviour sanitizers
// (recv.mk) and run by tests/test_recv.py.
//
//   recv_check <recv_kat.txt>   replays every transcript of the fixture (the reference's recorded
//                               verdicts, nonces, register states and deciphered bytes) through
//                                 - the plain sequential model: one datagram after the other,
//                                   hashed under its real nonce, and
//                                 - the kernels' split (parse, predict, tag, resolve, decipher: the
//                                   functions recv.hip runs, lanes one after the other) with 1 and
//                                   16 lanes, the streams interleaved and in reverse list order,
//                                   the transcripts cut into calls of 1, 3 and all datagrams, the
//                                   datagrams at 16 misalignments between guards of 0xA5, with the
//                                   real guesses and with arbitrary ones;
//                               then the invalid datagrams, and a seeded soak of 2,000 connections
//                               x 64 datagrams (30 % corrupted tags, 10 % repeats) in which the
//                               split must equal the sequential model in every result, state word
//                               and byte.  Prints "ok <cases> repaired <share of the soak's
//                               datagrams whose tag the resolve step hashed again>" or the first
//                               failure.
#include "../../tonk_amd/csrc/recv.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

const uint32_t kGuard = 64;
const uint8_t kFill = 0xA5;

int fail(const char* what, long a = 0, long b = 0, long c = 0) {
    printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

uint64_t window_fnv(const uint64_t* st) {
    uint8_t b[TAMD_RECV_WORDS * 8];
    for (uint32_t w = 0; w < TAMD_RECV_WORDS; ++w)
        for (uint32_t k = 0; k < 8; ++k) b[8 * w + k] = (uint8_t)(st[TAMD_RECV_S_WINDOW + w] >> (8 * k));
    return fnv1a(b, sizeof(b));
}

struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    uint32_t below(uint32_t n) { return (uint32_t)((next() >> 20) % n); }
};

// The kernel's tag phase for one datagram (seal_check.cpp's walk): tiles staged granule by granule.
uint64_t hash_walk(const uint8_t* data, uint32_t len, uint64_t seed) {
    tamd_v16 tile[TAMD_SEAL_TILE_V16];
    memset(tile, 0xEE, sizeof(tile));
    tamd_t1ha st;
    tamd_t1ha_init(&st, len, seed);
    uint64_t hash = 0;
    const uint32_t tiles = (len + TAMD_SEAL_TILE - 1u) / TAMD_SEAL_TILE;
    for (uint32_t t = 0; t < tiles; ++t) {
        for (uint32_t g = 0; g < TAMD_SEAL_TILE_V16; ++g) {
            tamd_v16 v;
            if (tamd_seal_stage(data, len, t, g, &v)) tile[g] = v;
        }
        if (tamd_seal_hash_tile(&st, tile, t, &hash)) return hash;
    }
    return tamd_seal_hash_end(&st);
}

// A datagram on the wire and, for a line of the fixture, what the reference made of it.
struct Dgram {
    std::vector<uint8_t> wire;
    bool expect = false;
    uint32_t rc = 0, rotation = 0;
    uint64_t expanded = 0, largest = 0, base = 0, wfnv = 0, dfnv = 0;
};
struct Conn {
    uint64_t key = 0, base = 0;
    std::vector<Dgram> g;
};

// The sender (tests/native/recv_golden.cpp's rule for datagram k of a connection), sealed with
// seal.h's functions under the true nonce.
std::vector<uint8_t> make_datagram(uint64_t key, uint32_t k, uint64_t nonce, uint32_t nb, uint32_t sb, uint32_t hs, uint32_t bytes,
                                   uint32_t corrupt) {
    const uint32_t F = 6 + (hs ? 12 : 0) + nb + sb, M = bytes - F, T = bytes - 6;
    // (an aligned copy with room for the granules around it: seal.h reads whole granules)
    uint8_t* raw = (uint8_t*)aligned_alloc(64, (bytes + 63 + 64) / 64 * 64);
    uint8_t* b = raw;
    for (uint32_t i = 0; i < M; ++i) b[i] = (uint8_t)(i * 131u + bytes * 7u + k * 13u + 1u);
    uint32_t at = M;
    const uint32_t seq = k * 40503u + 7u;
    for (uint32_t j = 0; j < sb; ++j) b[at++] = (uint8_t)(seq >> (8 * j));
    for (uint32_t j = 0; j < nb; ++j) b[at++] = (uint8_t)(nonce >> (8 * j));
    for (uint32_t j = 0; hs && j < 12; ++j) b[at++] = (uint8_t)(k + j * 17u + 3u);
    const uint32_t ts24 = (k * 2654435761u + bytes) & 0xffffffu;
    const uint8_t flags = (uint8_t)(0x80u | (hs ? 0x40u : 0u) | (k % 3 == 0 ? 0x20u : 0u) | nb << 2 | sb);
    b[at++] = (uint8_t)ts24;
    b[at++] = (uint8_t)(ts24 >> 8);
    b[at++] = (uint8_t)(ts24 >> 16);
    b[at++] = flags;
    const tamd_seal_key K = tamd_seal_expand(key);
    tamd_seal_cipher(b, M, K, tamd_seal_adder(nonce), 0, 1);
    uint16_t tag = tamd_seal_datagram_tag(K, hash_walk(b, T, nonce ^ tamd_seal_key64(K)), b, T);
    if (corrupt) tag ^= (uint16_t)(1u << ((corrupt - 1) & 15));
    b[at++] = (uint8_t)tag;
    b[at++] = (uint8_t)(tag >> 8);
    std::vector<uint8_t> out(b, b + bytes);
    free(raw);
    return out;
}

int read_fixture(const char* path, std::vector<Conn>* conns) {
    FILE* f = fopen(path, "r");
    if (!f) return fail("cannot open the fixture");
    char line[512];
    long lineno = 0;
    while (fgets(line, sizeof(line), f)) {
        ++lineno;
        unsigned long long v[13];
        int nv = 0;
        char* at = line + 1;
        for (; nv < 13; ++nv) {
            char* end = nullptr;
            const unsigned long long x = strtoull(at, &end, 0);
            if (end == at) break;
            v[nv] = x;
            at = end;
        }
        if (line[0] == 'S' && nv == 2) {
            Conn c;
            c.key = v[0];
            c.base = v[1];
            conns->push_back(c);
        } else if (line[0] == 'G' && nv == 13 && !conns->empty()) {
            Conn& c = conns->back();
            Dgram d;
            d.wire = make_datagram(c.key, (uint32_t)c.g.size(), v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4],
                                   (uint32_t)v[5]);
            d.expect = true;
            d.rc = (uint32_t)v[6];
            d.expanded = v[7];
            d.largest = v[8];
            d.base = v[9];
            d.rotation = (uint32_t)v[10];
            d.wfnv = v[11];
            d.dfnv = v[12];
            c.g.push_back(d);
        } else {
            fclose(f);
            return fail("unreadable line", lineno);
        }
    }
    fclose(f);
    return conns->empty() ? fail("the fixture is empty") : 0;
}

// One call: items in list order, their slots in a buffer between guards.
struct Item {
    uint32_t stream, bytes;
    size_t off;
    const Dgram *src, *want;  // the datagram; the fixture's line where it has one
};
struct Call {
    std::vector<Item> items;
    uint8_t* buf = nullptr;  // 64-byte aligned
    size_t size = 0;
    ~Call() { free(buf); }
};

struct Results {
    std::vector<uint32_t> rc;
    std::vector<RecvResult> res;
};

// The plain sequential model, checked against the fixture's line where an item has one.
int call_seq(const Call& call, uint8_t* buf, uint64_t* states, const std::vector<tamd_seal_key>& keys, uint32_t maxb, Results* out) {
    const size_t n = call.items.size();
    out->rc.assign(n, 0);
    out->res.assign(n, RecvResult());
    for (size_t i = 0; i < n; ++i) {
        const Item& it = call.items[i];
        uint8_t* data = buf + it.off;
        uint64_t* st = states + (size_t)it.stream * TAMD_RECV_STATE_WORDS;
        const tamd_seal_key& K = keys[it.stream];
        memset(&out->res[i], 0, sizeof(RecvResult));
        const RecvFields f = tamd_recv_read_footer(data, it.bytes, maxb);
        if (!f.flags) {
            out->rc[i] = TAMD_RECV_INVALID;
            if (it.want) return fail("the fixture holds an invalid datagram", (long)i);
            continue;
        }
        tamd_recv_reg r = tamd_recv_load(st);
        const uint64_t nonce = tamd_recv_expand(r.largest, f.partial_nonce, f.nonce_bytes);
        RecvResult& o = out->res[i];
        o.nonce = nonce;
        o.message_bytes = it.bytes - tamd_recv_footer_bytes(f.flags);
        o.timestamp24 = f.ts24;
        o.partial_seq = f.partial_seq;
        o.flags = f.flags;
        o.seq_bytes = f.seq_bytes;
        o.nonce_bytes = f.nonce_bytes;
        o.handshake_bytes = f.handshake_bytes;
        uint32_t rc;
        if (tamd_recv_is_duplicate(r, nonce)) {
            rc = TAMD_RECV_DUPLICATE;
        } else if (!tamd_recv_tag_ok(K, hash_walk(data, it.bytes - 6, nonce ^ tamd_seal_key64(K)), data, it.bytes)) {
            rc = TAMD_RECV_BAD_TAG;
        } else {
            tamd_recv_accept(&r, nonce);
            tamd_recv_store(st, r);
            tamd_seal_cipher(data, o.message_bytes, K, tamd_seal_adder(nonce), 0, 1);
            const bool reordered = f.seq_bytes > 0 && f.seq_bytes < f.nonce_bytes && tamd_recv_less(nonce + 1, r.largest + 1);
            rc = reordered ? TAMD_RECV_REORDERED : TAMD_RECV_OK;
        }
        out->rc[i] = rc;
        if (const Dgram* w = it.want) {
            if (rc != w->rc) return fail("verdict", (long)i, rc, w->rc);
            if (nonce != w->expanded) return fail("expanded nonce", (long)i, (long)nonce, (long)w->expanded);
            if (st[0] != w->largest || st[1] != w->base || st[2] != w->rotation) return fail("register", (long)i, (long)st[0], (long)st[1]);
            if (window_fnv(st) != w->wfnv) return fail("window", (long)i);
            if (fnv1a(data, it.bytes) != w->dfnv) return fail("datagram bytes", (long)i);
        }
    }
    return 0;
}

// The kernels' split.  guesses 0: tamd_recv_predict_stream's; 1: arbitrary numbers (the results
// may not depend on them).  Adds the datagrams hashed again to *repaired.
void call_split(const Call& call, uint8_t* buf, uint64_t* states, const std::vector<tamd_seal_key>& keys, uint32_t maxb, uint32_t nl,
                uint32_t guesses, Results* out, long* repaired) {
    const uint32_t n = (uint32_t)call.items.size();
    std::vector<RecvDesc> d(n);
    std::vector<RecvFields> f(n);
    std::vector<uint64_t> pred(n, 0);
    std::vector<uint32_t> tag_ok(n, 0), rcw(n, 0xdead), clen(n, 0xdead);
    out->res.assign(n, RecvResult());
    for (uint32_t i = 0; i < n; ++i) memset(&out->res[i], 0, sizeof(RecvResult));
    for (uint32_t i = 0; i < n; ++i) d[i] = RecvDesc{(uint64_t)(uintptr_t)(buf + call.items[i].off), call.items[i].stream, call.items[i].bytes};
    // parse
    for (uint32_t i = 0; i < n; ++i) f[i] = tamd_recv_read_footer((const uint8_t*)d[i].data, d[i].bytes, maxb);
    // the CSR list, streams in the order they first appear (recv.cpp)
    std::vector<uint32_t> listed, start, idx(n), count(keys.size(), 0);
    for (uint32_t i = 0; i < n; ++i)
        if (count[d[i].stream]++ == 0) listed.push_back(d[i].stream);
    uint32_t acc = 0;
    for (uint32_t st : listed) {
        start.push_back(acc);
        acc += count[st];
        count[st] = start.back();
    }
    start.push_back(acc);
    for (uint32_t i = 0; i < n; ++i) idx[count[d[i].stream]++] = i;
    // predict
    for (size_t j = 0; j < listed.size(); ++j)
        tamd_recv_predict_stream(states + (size_t)listed[j] * TAMD_RECV_STATE_WORDS, idx.data() + start[j], start[j + 1] - start[j], f.data(),
                                 pred.data());
    if (guesses) {
        Rng rng{0x9e3779b97f4a7c15ull ^ n};
        for (uint32_t i = 0; i < n; ++i)
            if (rng.below(3)) pred[i] = rng.below(2) ? rng.next() : pred[i] + rng.below(3) - 1;
    }
    // tag
    for (uint32_t i = 0; i < n; ++i) {
        if (!f[i].flags) continue;
        const tamd_seal_key& K = keys[d[i].stream];
        const uint8_t* data = (const uint8_t*)d[i].data;
        tag_ok[i] = tamd_recv_tag_ok(K, hash_walk(data, d[i].bytes - 6, pred[i] ^ tamd_seal_key64(K)), data, d[i].bytes);
    }
    // resolve (the streams in the opposite order: they are independent)
    for (size_t j = listed.size(); j-- > 0;)
        tamd_recv_resolve_stream(states + (size_t)listed[j] * TAMD_RECV_STATE_WORDS, keys[listed[j]], idx.data() + start[j],
                                 start[j + 1] - start[j], d.data(), f.data(), pred.data(), tag_ok.data(), rcw.data(), out->res.data(),
                                 clen.data());
    // decipher
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t lane = 0; clen[i] && lane < nl; ++lane)
            tamd_seal_cipher((uint8_t*)d[i].data, clen[i], keys[d[i].stream], tamd_seal_adder(out->res[i].nonce), lane, nl);
    out->rc.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        out->rc[i] = rcw[i] & 0xffu;
        if (rcw[i] & TAMD_RECV_REPAIRED) ++*repaired;
    }
}

// The datagrams [from, from + chunk) of every connection as one call.  order 0: round robin over
// the connections; 1: connection by connection, the last one first.  Slots `pitch` apart from
// misalignment `mis`, 0xA5 everywhere else.
void build_call(const std::vector<Conn>& conns, size_t from, size_t chunk, uint32_t order, uint32_t mis, Call* call) {
    uint32_t longest = 0;
    std::vector<size_t> cnt(conns.size());
    size_t deepest = 0;
    for (size_t c = 0; c < conns.size(); ++c) {
        const size_t have = conns[c].g.size() > from ? conns[c].g.size() - from : 0;
        cnt[c] = have < chunk ? have : chunk;
        if (cnt[c] > deepest) deepest = cnt[c];
        for (size_t k = 0; k < cnt[c]; ++k)
            if (conns[c].g[from + k].wire.size() > longest) longest = (uint32_t)conns[c].g[from + k].wire.size();
    }
    const size_t pitch = longest + 5;
    call->items.clear();
    auto add = [&](size_t c, size_t k) {
        const Dgram& g = conns[c].g[from + k];
        call->items.push_back(Item{(uint32_t)c, (uint32_t)g.wire.size(), kGuard + mis + call->items.size() * pitch, &g, g.expect ? &g : nullptr});
    };
    if (order == 0) {
        for (size_t k = 0; k < deepest; ++k)
            for (size_t c = 0; c < conns.size(); ++c)
                if (k < cnt[c]) add(c, k);
    } else {
        for (size_t c = conns.size(); c-- > 0;)
            for (size_t k = 0; k < cnt[c]; ++k) add(c, k);
    }
    call->size = (kGuard + 16 + call->items.size() * pitch + kGuard + 63) / 64 * 64;
    free(call->buf);
    call->buf = (uint8_t*)aligned_alloc(64, call->size);
    memset(call->buf, kFill, call->size);
    for (const Item& it : call->items) memcpy(call->buf + it.off, it.src->wire.data(), it.src->wire.size());
}

// All of `conns` through both models, cut into calls of `chunk` datagrams per connection.
int replay(const std::vector<Conn>& conns, size_t chunk, uint32_t order, uint32_t mis, uint32_t nl, uint32_t guesses, uint32_t maxb,
           long* cases, long* repaired) {
    const size_t nc = conns.size();
    std::vector<tamd_seal_key> keys(nc);
    std::vector<uint64_t> seq_state(nc * TAMD_RECV_STATE_WORDS), split_state;
    size_t deepest = 0;
    for (size_t c = 0; c < nc; ++c) {
        keys[c] = tamd_seal_expand(conns[c].key);
        tamd_recv_reset_state(&seq_state[c * TAMD_RECV_STATE_WORDS], conns[c].base);
        if (conns[c].g.size() > deepest) deepest = conns[c].g.size();
    }
    split_state = seq_state;
    Results a, b;
    for (size_t from = 0; from < deepest; from += chunk) {
        Call call;
        build_call(conns, from, chunk, order, mis, &call);
        uint8_t* other = (uint8_t*)aligned_alloc(64, call.size);
        memcpy(other, call.buf, call.size);
        int bad = call_seq(call, call.buf, seq_state.data(), keys, maxb, &a);
        if (!bad) {
            call_split(call, other, split_state.data(), keys, maxb, nl, guesses, &b, repaired);
            if (memcmp(call.buf, other, call.size)) bad = fail("the split's bytes differ from the sequential model's", (long)from, mis, nl);
            else if (seq_state != split_state) bad = fail("the split's register states differ", (long)from, mis, nl);
            for (size_t i = 0; !bad && i < call.items.size(); ++i) {
                if (a.rc[i] != b.rc[i]) bad = fail("the split's verdict differs", (long)from, (long)i, b.rc[i]);
                else if (memcmp(&a.res[i], &b.res[i], sizeof(RecvResult))) bad = fail("the split's result record differs", (long)from, (long)i);
            }
            // nothing but the slots changed
            for (size_t p = 0; !bad && p < kGuard + mis; ++p)
                if (other[p] != kFill) bad = fail("a write in front of the call's slots", (long)p);
            for (size_t i = 0; !bad && i < call.items.size(); ++i) {
                const size_t end = i + 1 < call.items.size() ? call.items[i + 1].off : call.size;
                for (size_t p = call.items[i].off + call.items[i].bytes; p < end; ++p)
                    if (other[p] != kFill) {
                        bad = fail("a write behind a slot", (long)i, (long)p);
                        break;
                    }
            }
        }
        free(other);
        if (bad) return 1;
        *cases += (long)call.items.size();
    }
    return 0;
}

// The causes of rc 1, each with the state and the bytes untouched, among valid datagrams.
int check_invalid(long* cases) {
    std::vector<Conn> conns(1);
    conns[0].key = 0x0123456789abcdefull;
    conns[0].base = 10;
    auto add = [&](std::vector<uint8_t> w) {
        Dgram d;
        d.wire = w;
        conns[0].g.push_back(d);
    };
    add(make_datagram(conns[0].key, 0, 11, 1, 0, 0, 40, 0));
    std::vector<uint8_t> w = make_datagram(conns[0].key, 1, 12, 1, 0, 0, 40, 0);
    w[40 - 3] &= 0x7f;  // not a connection datagram
    add(w);
    add(std::vector<uint8_t>(5, 0x80));                              // shorter than six bytes
    add(make_datagram(conns[0].key, 3, 12, 1, 0, 0, 101, 0));        // above the maximum (100)
    w = make_datagram(conns[0].key, 4, 12, 3, 3, 1, 24, 0);
    w.erase(w.begin());                                              // 23 bytes, its flags ask for 24
    add(w);
    w = std::vector<uint8_t>(6, 0);
    w[3] = 0x80 | 1 << 2;                                            // six bytes, one nonce byte announced
    add(w);
    add(make_datagram(conns[0].key, 6, 12, 1, 0, 0, 100, 0));        // exactly the maximum: valid
    add(make_datagram(conns[0].key, 7, 13, 3, 3, 1, 24, 0));         // exactly its footer: valid
    const uint32_t want[] = {0, 1, 1, 1, 1, 1, 0, 0};
    for (uint32_t nl : {1u, 16u})
        for (size_t chunk : {(size_t)1, (size_t)8}) {
            // (replay compares the split with the sequential model, bytes and states included)
            long repaired = 0;
            if (replay(conns, chunk, 0, 3, nl, 0, 100, cases, &repaired)) return 1;
        }
    // the verdicts themselves
    Call call;
    build_call(conns, 0, 8, 0, 7, &call);
    std::vector<tamd_seal_key> keys(1, tamd_seal_expand(conns[0].key));
    std::vector<uint64_t> st(TAMD_RECV_STATE_WORDS);
    tamd_recv_reset_state(st.data(), conns[0].base);
    Results r;
    long repaired = 0;
    std::vector<uint8_t> before(call.buf, call.buf + call.size);
    call_split(call, call.buf, st.data(), keys, 100, 1, 0, &r, &repaired);
    for (size_t i = 0; i < 8; ++i) {
        if (r.rc[i] != want[i]) return fail("an invalid datagram's verdict", (long)i, r.rc[i]);
        if (want[i] == 1 && memcmp(call.buf + call.items[i].off, before.data() + call.items[i].off, call.items[i].bytes))
            return fail("an invalid datagram was written", (long)i);
    }
    if (st[0] != 13 || repaired != 0) return fail("the invalid datagrams moved the register", (long)st[0], repaired);
    return 0;
}

// 2,000 connections x 64 datagrams: loss, reordering, jumps, 30 % corrupted tags, 10 % repeats.
int soak(long* cases, double* share) {
    Rng rng{0x243f6a8885a308d3ull};
    std::vector<Conn> conns(2000);
    for (Conn& c : conns) {
        c.key = rng.below(8) ? rng.next() : 0;
        c.base = rng.below(4) ? rng.next() >> rng.below(60) : 0xffffffffffffff00ull + rng.below(512);
        uint64_t cur = c.base;
        for (uint32_t k = 0; k < 64; ++k) {
            if (k && rng.below(10) == 0) {  // the datagram before, again
                Dgram again = c.g.back();
                c.g.push_back(again);
                continue;
            }
            const uint32_t how = rng.below(20);
            uint64_t nonce;
            if (how < 12) nonce = cur + 1 + rng.below(3);
            else if (how < 16) nonce = cur - rng.below(60);
            else if (how < 18) nonce = cur + rng.below(9000);
            else if (how < 19) nonce = cur + 4096 + 64 * rng.below(70);
            else nonce = cur - 4000 - rng.below(400);
            const uint32_t nb = rng.below(4), sb = rng.below(4), hs = rng.below(10) == 0;
            const uint32_t F = 6 + (hs ? 12 : 0) + nb + sb, bytes = F + (rng.below(6) ? rng.below(90) : rng.below(400));
            const uint32_t corrupt = rng.below(10) < 3 ? 1 + rng.below(16) : 0;
            Dgram d;
            d.wire = make_datagram(c.key, k, nonce, nb, sb, hs, bytes, corrupt);
            c.g.push_back(d);
            if (!corrupt && tamd_recv_less(cur, nonce)) cur = nonce;  // (roughly what the receiver will hold)
        }
    }
    long repaired = 0;
    if (replay(conns, 16, 0, 5, 16, 0, 65535, cases, &repaired)) return 1;
    long again = 0;
    if (replay(conns, 64, 1, 11, 1, 1, 65535, cases, &again)) return 1;
    *share = (double)repaired / (2000.0 * 64.0);
    if (repaired == 0) return fail("the soak repaired no guess");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: recv_check <recv_kat.txt>");
    std::vector<Conn> conns;
    if (read_fixture(argv[1], &conns)) return 1;
    long cases = 0, repaired = 0;
    // the fixture: calls of 1 (the split degenerates to the sequential order), 3 and all datagrams
    const size_t chunks[] = {1, 3, 100000};
    uint32_t run = 0;
    for (uint32_t mis = 0; mis < 16; ++mis) {
        const size_t chunk = chunks[run % 3];
        const uint32_t order = (run / 3) & 1, nl = mis & 1 ? 16 : 1, guesses = (run % 5) == 4;
        if (replay(conns, chunk, order, mis, nl, guesses, 65535, &cases, &repaired)) {
            printf("(chunk %zu, order %u, misalignment %u, lanes %u, guesses %u)\n", chunk, order, mis, nl, guesses);
            return 1;
        }
        ++run;
    }
    if (check_invalid(&cases)) return 1;
    double share = 0;
    if (soak(&cases, &share)) return 1;
    printf("ok %ld repaired %.4f\n", cases, share);
    return 0;
}
