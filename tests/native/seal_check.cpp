// seal_check -- the byte logic of the datagram cipher and tag (tonk_amd/csrc/seal.h) as a serial
// host walk: one lane (or eight lanes one after the other) runs exactly the functions the kernel
// runs across a wave.  Test-only; built plain and under the address and undefined-behaviour
// sanitizers (seal.mk) and run by tests/test_seal.py.
//
//   seal_check <seal_kat.txt>   every line of the fixture (the reference's recorded outputs) at
//                               source misalignments 0..15 between guards of 0xA5, every sealed D
//                               datagram opened back to its plaintext, and the rejections with
//                               nothing written; prints "ok <cases>" or the first failure
#include "../../tonk_amd/csrc/seal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

const uint32_t kGuard = 64;

int fail(const char* what, long a = 0, long b = 0, long c = 0) {
    printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

uint8_t payload_byte(uint32_t len, uint32_t msg, uint32_t i) { return (uint8_t)(i * 131u + len * 7u + msg * 13u + 1u); }

uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// 16-byte aligned storage with room for the aligned granules around any datagram inside it
struct Aligned {
    uint8_t* p;
    size_t n;
    explicit Aligned(size_t bytes) : p((uint8_t*)aligned_alloc(64, (bytes + 63) / 64 * 64)), n(bytes) {}
    ~Aligned() { free(p); }
};

// `len` payload bytes at misalignment `mis` inside `buf`, 0xA5 around them; returns their address.
uint8_t* place(Aligned& buf, uint32_t len, uint32_t msg, uint32_t mis) {
    memset(buf.p, 0xA5, kGuard + 16 + len + kGuard);
    uint8_t* at = buf.p + kGuard + mis;
    for (uint32_t i = 0; i < len; ++i) at[i] = payload_byte(len, msg, i);
    return at;
}

bool guards_ok(const Aligned& buf, const uint8_t* at, uint32_t len) {
    for (const uint8_t* p = buf.p; p < at; ++p)
        if (*p != 0xA5) return false;
    for (const uint8_t* p = at + len; p < buf.p + kGuard + 16 + len + kGuard; ++p)
        if (*p != 0xA5) return false;
    return true;
}

// The kernel's cipher phase for one datagram: `nl` lanes, one after the other.
void cipher_walk(uint8_t* data, uint32_t len, const tamd_seal_key& K, uint64_t nonce, uint32_t nl) {
    const tamd_seal_key A = tamd_seal_adder(nonce);
    for (uint32_t lane = 0; lane < nl; ++lane) tamd_seal_cipher(data, len, K, A, lane, nl);
}

// The kernel's tag phase for one datagram: tiles staged granule by granule (stale bytes of the
// tile before are left where nothing is staged, as in LDS), the state advanced over each.
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

// tamd_seal_packets for one datagram in the connected layout; returns its result code.
int datagram_walk(bool open, uint8_t* data, uint32_t bytes, uint32_t msg, uint32_t max_bytes, const tamd_seal_key& K,
                  uint64_t nonce, uint32_t nl) {
    if (!tamd_seal_valid(bytes, msg, max_bytes)) return TAMD_SEAL_INVALID;
    const uint32_t T = bytes - TAMD_SEAL_UNTAGGED;
    if (!open) cipher_walk(data, msg, K, nonce, nl);
    const uint16_t tag = tamd_seal_datagram_tag(K, hash_walk(data, T, nonce ^ tamd_seal_key64(K)), data, T);
    if (!open) {
        data[T + 4] = (uint8_t)tag;
        data[T + 5] = (uint8_t)(tag >> 8);
        return TAMD_SEAL_OK;
    }
    if ((uint16_t)(data[T + 4] | data[T + 5] << 8) != tag) return TAMD_SEAL_BAD_TAG;
    cipher_walk(data, msg, K, nonce, nl);
    return TAMD_SEAL_OK;
}

void stamp(uint8_t* data, uint32_t bytes, uint32_t ts24, uint32_t flags) {
    const uint32_t T = bytes - 6;
    const uint8_t f[6] = {(uint8_t)ts24, (uint8_t)(ts24 >> 8), (uint8_t)(ts24 >> 16), (uint8_t)flags, 0, 0};
    memcpy(data + T, f, 6);
}

int check_fixture(const char* path, long* cases) {
    FILE* f = fopen(path, "r");
    if (!f) return fail("cannot open the fixture");
    Aligned buf(kGuard * 2 + 32 + 65535), plain(65535 + 64);
    char line[256];
    long lineno = 0, n_c = 0, n_i = 0, n_d = 0;
    while (fgets(line, sizeof(line), f)) {
        ++lineno;
        // a kind letter, then up to seven numbers (hexadecimal with 0x, else decimal)
        unsigned long long v[7] = {0, 0, 0, 0, 0, 0, 0};
        int nv = 0;
        char* at_ch = line + 1;
        for (; nv < 7; ++nv) {
            char* end = nullptr;
            const unsigned long long x = strtoull(at_ch, &end, 0);
            if (end == at_ch) break;
            v[nv] = x;
            at_ch = end;
        }
        const uint64_t key = v[0];
        if (line[0] == 'C' && nv == 6) {
            const uint64_t seq = v[1], fnv = v[5];
            const uint32_t len = (uint32_t)v[2], msg = (uint32_t)v[3], tag = (uint32_t)v[4];
            const tamd_seal_key K = tamd_seal_expand(key);
            for (uint32_t mis = 0; mis < 16; ++mis) {
                uint8_t* at = place(buf, len, msg, mis);
                cipher_walk(at, msg, K, seq, mis & 1 ? 8 : 1);
                const unsigned got = tamd_seal_tag16(hash_walk(at, len, seq ^ tamd_seal_key64(K)));
                if (got != tag) return fail("C tag", lineno, mis, got);
                if (fnv1a(at, len) != fnv) return fail("C bytes", lineno, mis);
                if (!guards_ok(buf, at, len)) return fail("C wrote outside the data", lineno, mis);
                cipher_walk(at, msg, K, seq, 3);  // (deciphering is the same walk)
                for (uint32_t i = 0; i < len; ++i)
                    if (at[i] != payload_byte(len, msg, i)) return fail("C round trip", lineno, mis, i);
            }
            ++n_c;
        } else if (line[0] == 'I' && nv == 3) {
            if (tamd_seal_tag_int(tamd_seal_expand(key), (uint32_t)v[1]) != v[2]) return fail("I", lineno);
            ++n_i;
        } else if (line[0] == 'D' && nv == 7) {
            const uint64_t seq = v[1], fnv = v[6];
            const uint32_t len = (uint32_t)v[2], msg = (uint32_t)v[3], ts24 = (uint32_t)v[4], flags = (uint32_t)v[5];
            const tamd_seal_key K = tamd_seal_expand(key);
            for (uint32_t mis = 0; mis < 16; ++mis) {
                uint8_t* at = place(buf, len, msg, mis);
                stamp(at, len, ts24, flags);
                memcpy(plain.p, at, len);
                const uint32_t nl = mis & 1 ? 8 : 1;
                if (datagram_walk(false, at, len, msg, 65535, K, seq, nl) != TAMD_SEAL_OK) return fail("D seal rc", lineno, mis);
                if (fnv1a(at, len) != fnv) return fail("D sealed bytes", lineno, mis);
                if (!guards_ok(buf, at, len)) return fail("D seal wrote outside the datagram", lineno, mis);
                // one bit of the tag flipped: refused for certain, and left as it was
                at[len - 2 + (mis >> 3)] ^= (uint8_t)(1u << (mis & 7));
                const uint64_t before = fnv1a(at, len);
                if (datagram_walk(true, at, len, msg, 65535, K, seq, nl) != TAMD_SEAL_BAD_TAG) return fail("D damaged tag accepted", lineno, mis);
                if (fnv1a(at, len) != before) return fail("D a refused datagram was written", lineno, mis);
                at[len - 2 + (mis >> 3)] ^= (uint8_t)(1u << (mis & 7));
                if (datagram_walk(true, at, len, msg, 65535, K, seq, nl) != TAMD_SEAL_OK) return fail("D open rc", lineno, mis);
                if (memcmp(at, plain.p, len - 2)) return fail("D opened bytes", lineno, mis);
                if (!guards_ok(buf, at, len)) return fail("D open wrote outside the datagram", lineno, mis);
            }
            ++n_d;
        } else {
            return fail("unreadable line", lineno);
        }
    }
    fclose(f);
    if (!n_c || !n_i || !n_d) return fail("the fixture lacks a kind of line", n_c, n_i, n_d);
    *cases += n_c + n_i + n_d;
    return 0;
}

// Datagrams that must be refused with nothing written.
int check_rejects(long* cases) {
    Aligned buf(kGuard * 2 + 32 + 256);
    const tamd_seal_key K = tamd_seal_expand(0x0123456789abcdefull);
    struct Case { const char* name; uint32_t bytes, msg, max_bytes; };
    const Case cs[] = {{"bytes 5", 5, 0, 1500}, {"bytes 0", 0, 0, 1500}, {"message_bytes = T + 1", 40, 35, 1500},
                       {"bytes above the maximum", 100, 10, 99}};
    for (const Case& c : cs)
        for (int open = 0; open < 2; ++open) {
            uint8_t* at = place(buf, c.bytes, c.msg, 3);
            const uint64_t before = fnv1a(buf.p, kGuard * 2 + 16 + c.bytes);
            if (datagram_walk(open, at, c.bytes, c.msg, c.max_bytes, K, 9, 1) != TAMD_SEAL_INVALID) return fail(c.name, open);
            if (fnv1a(buf.p, kGuard * 2 + 16 + c.bytes) != before) return fail("an invalid datagram was written", c.bytes, open);
            ++*cases;
        }
    {  // exactly at the bounds: accepted (T = 0; message_bytes = T; bytes = max)
        uint8_t* at = place(buf, 6, 0, 5);
        if (datagram_walk(false, at, 6, 0, 6, K, 9, 1) != TAMD_SEAL_OK || datagram_walk(true, at, 6, 0, 6, K, 9, 1) != TAMD_SEAL_OK)
            return fail("T = 0");
        at = place(buf, 40, 34, 5);
        if (datagram_walk(false, at, 40, 34, 40, K, 9, 1) != TAMD_SEAL_OK || datagram_walk(true, at, 40, 34, 40, K, 9, 1) != TAMD_SEAL_OK)
            return fail("message_bytes = T");
        // a flipped bit of the first byte, the last tagged byte, the timestamp and the flags; another
        // nonce; another key (a 16-bit tag: these particular changes are all seen)
        datagram_walk(false, at, 40, 34, 40, K, 9, 1);
        for (uint32_t victim : {0u, 33u, 35u, 37u}) {
            at[victim] ^= 0x10;
            if (datagram_walk(true, at, 40, 34, 40, K, 9, 1) != TAMD_SEAL_BAD_TAG) return fail("a damaged byte was accepted", victim);
            at[victim] ^= 0x10;
        }
        if (datagram_walk(true, at, 40, 34, 40, K, 10, 1) != TAMD_SEAL_BAD_TAG) return fail("nonce off by one accepted");
        if (datagram_walk(true, at, 40, 34, 40, K, 9 | 1ull << 32, 1) != TAMD_SEAL_BAD_TAG) return fail("nonce high word accepted");
        if (datagram_walk(true, at, 40, 34, 40, tamd_seal_expand(0x0123456789abcdeeull), 9, 1) != TAMD_SEAL_BAD_TAG)
            return fail("another key accepted");
        ++*cases;
    }
    {  // the footer gather
        for (uint32_t total : {1u, 6u, 23u, 24u, 25u, 200u}) {
            uint8_t* at = place(buf, total, 0, 7);
            uint8_t got[24], want[24];
            memset(want, 0, 24);
            const uint32_t tl = total < 24 ? total : 24;
            memcpy(want + 24 - tl, at + total - tl, tl);
            tamd_seal_footer24(at, total, got);
            if (memcmp(got, want, 24)) return fail("footer", total);
            ++*cases;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: seal_check <seal_kat.txt>");
    long cases = 0;
    if (check_fixture(argv[1], &cases) || check_rejects(&cases)) return 1;
    printf("ok %ld\n", cases);
    return 0;
}
