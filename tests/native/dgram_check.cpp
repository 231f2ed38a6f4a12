// dgram_check -- the byte logic of datagram building and parsing (tonk_amd/csrc/dgram.h) as a serial
// host walk: one lane, or the kernel's sixteen lanes one after the other, runs exactly the
// functions the kernels run.  Test-only; built plain and under the address and undefined-behaviour
// sanitizers (dgram.mk) and run by tests/test_dgram.py.
//
//   dgram_check <dgram_kat.txt>   every line of the fixture (the reference's recorded results; its
//                                 formats, draws and generators are stated in dgram_golden.cpp):
//                                 B lines at 16 source x 16 destination misalignments between
//                                 guards of 0xA5, P lines at 16 misalignments in both modes with
//                                 tables of 1, 16 and 700 entries; then the refusals; prints
//                                 "ok <cases>" or the first failure
#include "../../tonk_amd/csrc/dgram.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

const uint32_t kGuard = 64, kLanes = 16;
const uint32_t kTypes[6] = {3, 6, 0, 5, 31, 1};

int fail(const char* what, long a = 0, long b = 0, long c = 0) {
    printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

uint32_t mix(uint32_t seed, uint32_t c) {
    uint32_t h = seed ^ (c * 0x9E3779B1u);
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

struct Draw {
    uint32_t seed, c = 0;
    explicit Draw(uint32_t s) : seed(s) {}
    uint8_t byte() { return (uint8_t)mix(seed, c++); }
    uint32_t word(unsigned n) {
        uint32_t v = 0;
        for (unsigned k = 0; k < n; ++k) v |= (uint32_t)byte() << (8 * k);
        return v;
    }
    void fill(std::vector<uint8_t>& out, uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) out.push_back(byte());
    }
};

uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// 64-byte aligned storage
struct Aligned {
    uint8_t* p;
    size_t n;
    explicit Aligned(size_t bytes) : p((uint8_t*)aligned_alloc(64, (bytes + 63) / 64 * 64)), n((bytes + 63) / 64 * 64) {}
    ~Aligned() { free(p); }
};

bool all_fill(const uint8_t* lo, const uint8_t* hi) {
    for (const uint8_t* p = lo; p < hi; ++p)
        if (*p != 0xA5) return false;
    return true;
}

std::vector<std::vector<uint8_t>> g_sections;  // the message sections of the B lines

// tamd_dgram_frames for one datagram: its messages (in list order, or from the last to the first)
// and its footer, each by one lane or by sixteen one after the other.
void build_walk(uint8_t* dst, const std::vector<const uint8_t*>& src, const uint32_t* type, const uint32_t* bytes,
                const uint32_t* offset, uint32_t message_bytes, const uint8_t* footer, uint32_t footer_len, uint32_t nl, bool backwards) {
    const uint32_t count = (uint32_t)src.size();
    if (backwards)
        for (uint32_t lane = 0; lane < nl; ++lane) tamd_dgram_put_footer(dst + message_bytes, footer, footer_len, lane, nl);
    for (uint32_t q = 0; q < count; ++q) {
        const uint32_t k = backwards ? count - 1 - q : q;
        const uint32_t hb = type[k] == TAMD_DGRAM_T_RAW ? 0u : TAMD_DGRAM_FRAME;
        for (uint32_t lane = 0; lane < nl; ++lane)
            tamd_dgram_put(dst + offset[k], src[k], bytes[k], hb, hb ? tamd_dgram_header(type[k], bytes[k]) : 0u, lane, nl);
    }
    if (!backwards)
        for (uint32_t lane = 0; lane < nl; ++lane) tamd_dgram_put_footer(dst + message_bytes, footer, footer_len, lane, nl);
}

int check_b(const std::vector<unsigned long long>& v, long lineno) {
    if (v.size() < 6 || v.size() != 6 + 2 * v[5] + 5) return fail("unreadable B line", lineno);
    const uint32_t seed = (uint32_t)v[0], seq_bytes = (uint32_t)v[1], nonce_bytes = (uint32_t)v[2], hs = (uint32_t)v[3];
    const uint32_t flag_bits = (uint32_t)v[4], count = (uint32_t)v[5];
    const unsigned long long* r = v.data() + 6 + 2 * count;
    std::vector<uint32_t> type(count), bytes(count), offset(count);
    for (uint32_t k = 0; k < count; ++k) {
        type[k] = (uint32_t)v[6 + 2 * k];
        bytes[k] = (uint32_t)v[7 + 2 * k];
    }
    Draw d(seed);
    const uint32_t seq = d.word(4), nonce = d.word(4), ts24 = d.word(3);
    std::vector<uint8_t> handshake;
    d.fill(handshake, 12);
    std::vector<std::vector<uint8_t>> body(count);
    size_t body_total = 0;
    for (uint32_t k = 0; k < count; ++k) {
        if (type[k] != TAMD_DGRAM_T_PADDING) d.fill(body[k], bytes[k]);
        body_total += bytes[k] + 48;
    }
    const tamd_dgram_plan p = tamd_dgram_layout(type.data(), bytes.data(), count, offset.data(), seq_bytes, nonce_bytes, hs, flag_bits, 65535, 65535);
    if (p.rc || p.out_bytes != r[0] || p.message_bytes != r[1] || p.reliable_offset != r[2] || p.reliable_bytes != r[3])
        return fail("B layout", lineno, p.out_bytes, p.reliable_offset);
    if (p.out_bytes > 8 && tamd_dgram_layout(type.data(), bytes.data(), count, offset.data(), seq_bytes, nonce_bytes, hs, flag_bits, p.out_bytes - 1, 65535).rc != 1)
        return fail("B one byte above the maximum accepted", lineno);
    if (tamd_dgram_layout(type.data(), bytes.data(), count, offset.data(), seq_bytes, nonce_bytes, hs, flag_bits, 65535, p.out_bytes - 1).rc != 1)
        return fail("B one byte above the pitch accepted", lineno);
    if (tamd_dgram_layout(type.data(), bytes.data(), count, offset.data(), seq_bytes, nonce_bytes, hs, flag_bits, p.out_bytes, p.out_bytes).rc != 0)
        return fail("B exactly the maximum refused", lineno);
    uint8_t footer[TAMD_DGRAM_FOOTER];
    const uint32_t flen = tamd_dgram_footer(footer, seq, seq_bytes, nonce, nonce_bytes, hs ? handshake.data() : nullptr, ts24, flag_bits);
    if (p.message_bytes + flen != p.out_bytes) return fail("B footer length", lineno, flen);

    Aligned out(kGuard * 2 + 32 + p.out_bytes), from(kGuard * 2 + body_total + 64);
    for (uint32_t sm = 0; sm < 16; ++sm) {
        // the bodies scattered in `from` between 0xA5, body k at misalignment (sm + 5 k) & 15
        memset(from.p, 0xA5, from.n);
        std::vector<const uint8_t*> src(count);
        uint8_t* at = from.p + kGuard;
        for (uint32_t k = 0; k < count; ++k) {
            at += (((sm + 5u * k) & 15u) + 16u - ((uintptr_t)at & 15u)) & 15u;
            src[k] = type[k] == TAMD_DGRAM_T_PADDING ? nullptr : at;
            if (!body[k].empty()) memcpy(at, body[k].data(), bytes[k]);
            at += bytes[k] + 17u;
        }
        for (uint32_t dm = 0; dm < 16; ++dm) {
            memset(out.p, 0xA5, out.n);
            uint8_t* dst = out.p + kGuard + dm;
            build_walk(dst, src, type.data(), bytes.data(), offset.data(), p.message_bytes, footer, flen, (sm ^ dm) & 1 ? kLanes : 1u, dm & 2);
            if (fnv1a(dst, p.out_bytes) != r[4]) return fail("B bytes", lineno, sm, dm);
            if (!all_fill(out.p, dst) || !all_fill(dst + p.out_bytes, out.p + out.n)) return fail("B wrote outside the datagram", lineno, sm, dm);
            if (sm == 0 && dm == 0) g_sections.push_back(std::vector<uint8_t>(dst, dst + p.message_bytes));
        }
    }
    return 0;
}

void frame(std::vector<uint8_t>& s, uint32_t type, uint32_t bytes, Draw* d) {
    const uint32_t h = tamd_dgram_header(type, bytes);
    s.push_back((uint8_t)h);
    s.push_back((uint8_t)(h >> 8));
    for (uint32_t i = 0; i < bytes; ++i) s.push_back(d ? d->byte() : (uint8_t)0);
}

bool section_of(const std::vector<unsigned long long>& v, std::vector<uint8_t>& s) {
    const uint32_t gen = (uint32_t)v[0], a = (uint32_t)v[1], b = (uint32_t)v[2], c = (uint32_t)v[3];
    s.clear();
    if (gen == 0) {
        if (a >= g_sections.size()) return false;
        s = g_sections[a];
    } else if (gen == 1) {
        Draw d(1000 + a);
        frame(s, a & 1 ? 6 : 3, (a < 2 ? 2 : a) - 2, &d);
        frame(s, 6, 7, &d);
        frame(s, 4, 1, &d);
    } else if (gen == 2) {
        for (uint32_t k = 0; k < a; ++k) frame(s, k & 1 ? 6 : 3, 0, nullptr);
    } else if (gen == 3) {
        Draw d(a);
        d.fill(s, b);
    } else if (gen == 4) {
        Draw d(4000 + a * 64 + b * 8 + c);
        std::vector<uint32_t> starts;
        for (uint32_t k = 0; k < a; ++k) {
            starts.push_back((uint32_t)s.size());
            frame(s, kTypes[k % 6], (k * 5 + a) % 23, &d);
        }
        if (b >= a) return false;
        if (c == 2) {
            const uint32_t h = tamd_dgram_header(kTypes[b % 6], 2047);
            s[starts[b]] = (uint8_t)h;
            s[starts[b] + 1] = (uint8_t)(h >> 8);
        } else if (c == 3) {
            s.resize(starts[b]);
            s.push_back(0x5a);
        } else {
            std::vector<uint8_t> t(s.begin(), s.begin() + starts[b]);
            Draw e(d.seed + 1000);
            frame(t, TAMD_DGRAM_T_ACKACK, c / 10, &e);
            if (b + 1 < a) t.insert(t.end(), s.begin() + starts[b + 1], s.end());
            s = t;
        }
    } else if (gen == 5) {
        Draw d(5000);
        for (uint32_t k = 0; k < 31; ++k) frame(s, 6, 2047, &d);
        frame(s, 6, 65535 - 31 * 2049 - 2, &d);
    } else {
        return false;
    }
    return true;
}

// tamd_dgram_sections for one section: tiles staged granule by granule (stale bytes of the tile
// before are left where nothing is staged, as in LDS), the walk advanced over each.
tamd_dgram_walk parse_walk(const uint8_t* data, uint32_t bytes, uint32_t mode, uint32_t* table, uint32_t cap) {
    tamd_v16 tile[TAMD_DGRAM_TILE_V16];
    memset(tile, 0xEE, sizeof(tile));
    tamd_dgram_walk w;
    tamd_dgram_walk_init(&w, bytes);
    const uint32_t tiles = (bytes + TAMD_DGRAM_TILE - 1u) / TAMD_DGRAM_TILE;
    for (uint32_t t = 0; t < tiles; ++t) {
        for (uint32_t g = 0; g < TAMD_DGRAM_TILE_V16; ++g) {
            tamd_v16 v;
            if (tamd_dgram_stage(data, bytes, t, g, &v)) tile[g] = v;
        }
        tamd_dgram_walk_tile(&w, (const uint8_t*)tile, t, mode, table, cap);
    }
    tamd_dgram_walk_end(&w);
    return w;
}

int check_p(const std::vector<unsigned long long>& v, long lineno) {
    if (v.size() != 15) return fail("unreadable P line", lineno);
    std::vector<uint8_t> s;
    if (!section_of(v, s) || s.size() != v[4]) return fail("P section", lineno, (long)s.size());
    const uint32_t bytes = (uint32_t)s.size();
    const uint32_t caps[3] = {1, 16, 700};
    Aligned buf(kGuard * 2 + 32 + bytes);
    std::vector<uint32_t> full(40000), table(701);
    for (uint32_t mode = 0; mode < 2; ++mode) {
        const unsigned long long* r = v.data() + 5 + 5 * mode;
        for (uint32_t mis = 0; mis < 16; ++mis) {
            memset(buf.p, 0xA5, buf.n);
            uint8_t* at = buf.p + kGuard + mis;
            if (bytes) memcpy(at, s.data(), bytes);
            const uint64_t before = fnv1a(buf.p, buf.n);
            const tamd_dgram_walk w = parse_walk(at, bytes, mode, full.data(), (uint32_t)full.size());
            if (w.status != r[0] || w.count != r[1] || w.rel_lo != r[2] || w.rel_hi - w.rel_lo != r[3])
                return fail("P results", lineno, mode, w.status);
            std::vector<uint8_t> le;
            for (uint32_t k = 0; k < w.count; ++k)
                for (uint32_t b = 0; b < 4; ++b) le.push_back((uint8_t)(full[k] >> (8 * b)));
            if (fnv1a(le.data(), le.size()) != r[4]) return fail("P table", lineno, mode, mis);
            // a table of `cap` entries: the same entries up to cap, the count in full, nothing behind
            const uint32_t cap = caps[(mis + mode) % 3];
            for (uint32_t& e : table) e = 0xA5A5A5A5u;
            const tamd_dgram_walk c = parse_walk(at, bytes, mode, table.data(), cap);
            if (c.status != w.status || c.count != w.count || c.rel_lo != w.rel_lo || c.rel_hi != w.rel_hi) return fail("P capped results", lineno, mode, cap);
            for (uint32_t k = 0; k < table.size(); ++k)
                if (table[k] != (k < cap && k < w.count ? full[k] : 0xA5A5A5A5u)) return fail("P capped table", lineno, cap, k);
            if (fnv1a(buf.p, buf.n) != before) return fail("P wrote to the section", lineno);
        }
    }
    return 0;
}

int check_fixture(const char* path, long* cases) {
    FILE* f = fopen(path, "r");
    if (!f) return fail("cannot open the fixture");
    std::vector<char> line(4096);
    long lineno = 0, n_b = 0, n_p = 0;
    while (fgets(line.data(), (int)line.size(), f)) {
        ++lineno;
        std::vector<unsigned long long> v;
        char* at = line.data() + 1;
        for (;;) {
            char* end = nullptr;
            const unsigned long long x = strtoull(at, &end, 0);
            if (end == at) break;
            v.push_back(x);
            at = end;
        }
        if (line[0] == 'B') {
            if (check_b(v, lineno)) return 1;
            ++n_b;
        } else if (line[0] == 'P') {
            if (check_p(v, lineno)) return 1;
            ++n_p;
        } else {
            return fail("unreadable line", lineno);
        }
    }
    fclose(f);
    if (!n_b || !n_p) return fail("the fixture lacks a kind of line", n_b, n_p);
    *cases += n_b + n_p;
    return 0;
}

// Datagrams that must be refused (tonk_datagram.h), and those next to them that must not.
int check_refusals(long* cases) {
    struct Case { const char* name; uint32_t rc, count, type[4], bytes[4], seq_bytes, nonce_bytes, flag_bits; };
    const Case cs[] = {
        {"type 32", 1, 1, {32}, {5}, 1, 0, 0},
        {"type 31", 0, 1, {31}, {5}, 1, 0, 0},
        {"2048 bytes", 1, 1, {3}, {2048}, 0, 0, 0},
        {"2047 bytes", 0, 1, {3}, {2047}, 0, 0, 0},
        {"seq_bytes 4", 1, 1, {3}, {5}, 4, 0, 0},
        {"nonce_bytes 4", 1, 1, {3}, {5}, 0, 4, 0},
        {"reliable without a sequence number", 1, 1, {6}, {5}, 0, 1, 0},
        {"reliable before unreliable", 1, 2, {6, 3}, {5, 5}, 1, 1, 0},
        {"reliable before AckAck", 1, 2, {5, 2}, {5, 3}, 1, 1, 0},
        {"Padding behind reliable", 0, 3, {6, 4, 4}, {5, 9, 0}, 1, 1, 0},
        {"reliable behind that Padding", 1, 3, {6, 4, 6}, {5, 9, 1}, 1, 1, 0},
        {"unreliable behind that Padding", 1, 3, {6, 4, 3}, {5, 9, 1}, 1, 1, 0},
        {"Padding before reliable", 0, 2, {4, 6}, {9, 5}, 1, 1, 0},
        {"no message", 0, 0, {0}, {0}, 0, 0, 0},
        {"OnlyFEC with a header", 1, 1, {6}, {50}, 0, 1, TAMD_DGRAM_F_ONLYFEC},
        {"OnlyFEC with a sequence number", 1, 1, {255}, {50}, 1, 1, TAMD_DGRAM_F_ONLYFEC},
        {"OnlyFEC of two", 1, 2, {255, 255}, {50, 50}, 0, 1, TAMD_DGRAM_F_ONLYFEC},
        {"OnlyFEC of none", 1, 0, {0}, {0}, 0, 1, TAMD_DGRAM_F_ONLYFEC},
        {"OnlyFEC", 0, 1, {255}, {4000}, 0, 1, TAMD_DGRAM_F_ONLYFEC},
        {"raw outside OnlyFEC", 1, 1, {255}, {50}, 0, 1, 0},
    };
    for (const Case& c : cs) {
        uint32_t offset[4];
        const tamd_dgram_plan p = tamd_dgram_layout(c.type, c.bytes, c.count, offset, c.seq_bytes, c.nonce_bytes, 0, c.flag_bits, 65535, 65535);
        if (p.rc != c.rc) return fail(c.name, p.rc);
        ++*cases;
    }
    {  // Padding ends the reliable span before it
        const uint32_t type[3] = {3, 6, 4}, bytes[3] = {4, 10, 7};
        uint32_t offset[3];
        const tamd_dgram_plan p = tamd_dgram_layout(type, bytes, 3, offset, 2, 0, 0, 0, 1500, 1500);
        if (p.rc || p.reliable_offset != 6 || p.reliable_bytes != 12 || p.message_bytes != 27 || p.out_bytes != 35) return fail("span before Padding");
        ++*cases;
    }
    {  // of the caller's flag bits only SeqComp and OnlyFEC are taken
        if (tamd_dgram_flags(2, 3, 1, 0xffu) != (0x80u | 0x40u | 0x20u | 0x10u | 3u << 2 | 2u)) return fail("flags");
        if (tamd_dgram_flags(0, 0, 0, 0xcfu) != 0x80u) return fail("flags taken from the caller");
        ++*cases;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: dgram_check <dgram_kat.txt>");
    long cases = 0;
    if (check_fixture(argv[1], &cases) || check_refusals(&cases)) return 1;
    printf("ok %ld\n", cases);
    return 0;
}
