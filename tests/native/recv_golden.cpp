// recv_golden -- writes the transcripts of tests/golden/recv_kat.txt.gz: what the reference's
// security::StrikeRegister, CounterExpand (Counter.h) and security::SimpleCipher make of the
// datagrams below, in the order of SessionIncoming::ProcessDatagram's front
// (TonkineseIncoming.cpp:110-173 and :216).  Test-only and not built by any test:
// tests/golden/make_recv_kat.sh compiles it against the reference and regenerates the fixture.
//
//   S key base      a connection starts: Initialize(key), StrikeRegister::Reset(base)
//   G nonce nonce_bytes seq_bytes handshake bytes corrupt  rc expanded largest base rotation window after
//                   datagram k (0, 1, ... since the S line) of the connection.  Inputs: the
//                   sender's true nonce, the nonce bytes sent, the sequence bytes, the handshake
//                   flag, the datagram's length, corrupt c > 0: bit (c - 1) & 15 of the tag flipped.
//                   Then the reference's verdict (0 accepted, 2 "Bad checksum", 3 "Ignored dupe",
//                   4 "Ignored re-ordered"), the nonce it expanded, and after the datagram
//                   LargestSequence, WindowBase, WindowBitRotation, the FNV-1a-64 of the 64 window
//                   words (little-endian bytes) and of the datagram's bytes as the reference left them.
//
// The datagram of a G line (T = bytes - 6, F = its footer bytes, M = bytes - F):
//   byte i < M               (i * 131 + bytes * 7 + k * 13 + 1) & 255, ciphered under the true nonce
//   sequence bytes           the low bytes of (k * 40503 + 7)
//   nonce bytes              the low bytes of the true nonce
//   handshake byte j         (k + j * 17 + 3) & 255
//   timestamp                (k * 2654435761 + bytes) & 0xffffff
//   flags                    0x80 | handshake 0x40 | 0x20 when k % 3 == 0 | nonce_bytes << 2 | seq_bytes
//   tag                      Tag(data, T, true nonce) ^ TagInt(timestamp << 8 | flags)
#include "SimpleCipher.h"
#include "StrikeRegister.h"

#include <stdint.h>
#include <stdio.h>
#include <vector>

namespace {

uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// (the members are protected)
struct Register : security::StrikeRegister {
    uint64_t largest() const { return LargestSequence.ToUnsigned(); }
    uint64_t base() const { return WindowBase.ToUnsigned(); }
    unsigned rotation() const { return WindowBitRotation; }
    uint64_t window_fnv() const {
        uint8_t b[kWordCount * 8];
        for (unsigned w = 0; w < kWordCount; ++w)
            for (unsigned k = 0; k < 8; ++k) b[8 * w + k] = (uint8_t)(SlidingWindow[w] >> (8 * k));
        return fnv1a(b, sizeof(b));
    }
};

uint32_t field(const uint8_t* end, unsigned nb) {
    uint32_t v = 0;
    for (unsigned k = 0; k < nb; ++k) v |= (uint32_t)end[-(int)nb + (int)k] << (8 * k);
    return v;
}

struct Conn {
    Register ar;
    security::SimpleCipher cipher;
    unsigned k = 0;

    Conn(uint64_t key, uint64_t base) {
        cipher.Initialize(key);
        ar.Reset(base);
        printf("S 0x%llx 0x%llx\n", (unsigned long long)key, (unsigned long long)base);
    }

    // The front of ProcessDatagram; the handshake hook says "continue".
    int process(uint8_t* data, unsigned bytes, uint64_t* expanded) {
        const uint8_t* footer = data + bytes - 1 - 2;
        const uint8_t flags = footer[0];
        footer -= 3;
        const uint32_t ts24 = footer[0] | (uint32_t)footer[1] << 8 | (uint32_t)footer[2] << 16;
        const unsigned hs = (flags & 0x40) ? 12 : 0, nb = (flags >> 2) & 3, sb = flags & 3;
        footer -= hs;
        uint64_t nonce;
        if (nb == 0)
            nonce = ar.GetNextExpected().ToUnsigned();
        else
            nonce = ar.Expand(field(footer, nb), nb).ToUnsigned();
        *expanded = nonce;
        if (ar.IsDuplicate(nonce)) return 3;
        const uint16_t expected = cipher.Tag(data, bytes - 6, nonce);
        const uint16_t tag = (uint16_t)(data[bytes - 2] | data[bytes - 1] << 8);
        if ((tag ^ cipher.TagInt(ts24 << 8 | flags)) != expected) return 2;
        ar.Accept(nonce);
        cipher.Cipher(data, bytes - (6 + hs + nb + sb), nonce);
        if (sb > 0 && sb < nb && ar.GetNextExpected() > Counter64(nonce + 1)) return 4;
        return 0;
    }

    void send(uint64_t nonce, unsigned nb, unsigned sb = 0, unsigned hs = 0, unsigned bytes = 48, unsigned corrupt = 0) {
        const unsigned F = 6 + (hs ? 12 : 0) + nb + sb, M = bytes - F, T = bytes - 6;
        std::vector<uint8_t> b(bytes);
        for (unsigned i = 0; i < M; ++i) b[i] = (uint8_t)(i * 131u + bytes * 7u + k * 13u + 1u);
        unsigned at = M;
        const uint32_t seq = k * 40503u + 7u;
        for (unsigned j = 0; j < sb; ++j) b[at++] = (uint8_t)(seq >> (8 * j));
        for (unsigned j = 0; j < nb; ++j) b[at++] = (uint8_t)(nonce >> (8 * j));
        for (unsigned j = 0; hs && j < 12; ++j) b[at++] = (uint8_t)(k + j * 17u + 3u);
        const uint32_t ts24 = (k * 2654435761u + bytes) & 0xffffffu;
        const uint8_t flags = (uint8_t)(0x80u | (hs ? 0x40u : 0u) | (k % 3 == 0 ? 0x20u : 0u) | nb << 2 | sb);
        b[at++] = (uint8_t)ts24;
        b[at++] = (uint8_t)(ts24 >> 8);
        b[at++] = (uint8_t)(ts24 >> 16);
        b[at++] = flags;
        cipher.Cipher(b.data(), M, nonce);
        uint16_t tag = cipher.Tag(b.data(), T, nonce);
        tag ^= cipher.TagInt(ts24 << 8 | flags);
        if (corrupt) tag ^= (uint16_t)(1u << ((corrupt - 1) & 15));
        b[at++] = (uint8_t)tag;
        b[at++] = (uint8_t)(tag >> 8);
        uint64_t expanded = 0;
        const int rc = process(b.data(), bytes, &expanded);
        printf("G 0x%llx %u %u %u %u %u %d 0x%llx 0x%llx 0x%llx %u 0x%016llx 0x%016llx\n", (unsigned long long)nonce, nb, sb, hs ? 1 : 0,
               bytes, corrupt, rc, (unsigned long long)expanded, (unsigned long long)ar.largest(), (unsigned long long)ar.base(),
               ar.rotation(), (unsigned long long)ar.window_fnv(), (unsigned long long)fnv1a(b.data(), bytes));
        ++k;
    }

    // accepted steps of at most 0x3fffff with three nonce bytes until `target` is the largest
    void walk_to(uint64_t target) {
        while (ar.largest() != target) {
            const uint64_t left = target - ar.largest();
            send(ar.largest() + (left > 0x3fffffu ? 0x3fffffu : left), 3);
        }
    }
};

const uint64_t kKeys[4] = {0x0123456789abcdefull, 0, 0xffffffff00000001ull, 0x00000000deadbeefull};
unsigned g_conn = 0;
uint64_t next_key() { return kKeys[g_conn++ % 4]; }

// the nonce widths across the wraps of the low 8, 16 and 24 bits, forwards and backwards
void wraps() {
    const uint64_t edges[] = {0xffull, 0xffffull, 0xffffffull, 0xffffffffull, 0xffffffffffffffffull};
    for (uint64_t w : edges)
        for (unsigned nb = 0; nb <= 3; ++nb) {
            Conn c(next_key(), w - 8);
            for (uint64_t d = 1; d <= 20; d += (nb && d % 5 == 0 ? 2 : 1)) c.send(w - 8 + d, nb, d % 4 == 0 ? 1 : 0);
            if (nb == 0) continue;
            // back over the wrap: the numbers left out above, then repeats
            for (uint64_t d : {16u, 11u, 6u, 16u, 3u, 20u}) c.send(w - 8 + d, nb);
            c.send(w - 8, nb);       // the base itself: never struck, but not above the largest
            c.send(w - 9, nb);       // below the base
        }
}

// gaps of exactly MSB - 1, MSB, MSB + 1 ahead of and behind the largest, per width
void msb_gaps() {
    for (unsigned nb = 1; nb <= 3; ++nb) {
        const uint64_t msb = 1ull << (8 * nb - 1), L = 0x5000000ull + 1000;
        for (int dir = 0; dir < 2; ++dir)
            for (int64_t off = -1; off <= 1; ++off) {
                Conn c(next_key(), dir ? L - 4 * msb : L);
                if (dir) c.walk_to(L);
                c.send(dir ? L - (msb + off) : L + (msb + off), nb);
                c.send(c.ar.largest() + 1, 0);
                c.send(dir ? L - (msb + off) : L + (msb + off), nb);  // again
            }
    }
}

void reorder() {
    Conn c(next_key(), 0);
    for (uint64_t n = 1; n <= 60; n += 2) c.send(n, 1);
    for (uint64_t n = 60; n >= 2; n -= 2) c.send(n, 1, 0, 0, 40 + (unsigned)n);
    for (uint64_t n : {7u, 8u, 59u, 60u, 61u, 61u}) c.send(n, 2);
    c.send(0, 1);  // the base: bit 0 was never struck
    c.send(0, 1);
}

// jumps that keep the window (4095), slide it by 1 (4096, 4096 + 63), 2 (4096 + 64) and 63 words
// (4096 + 62 * 64 and 63 more), reset it (from 4096 + 63 * 64 on), and go far beyond
void jumps() {
    const uint64_t J[] = {4095, 4096, 4096 + 63, 4096 + 64, 4096 + 62 * 64, 4096 + 62 * 64 + 63, 4096 + 63 * 64, 4096 + 64 * 64, 4096 + 64 * 64 + 1, 20000, 1ull << 20,
                          0x7fffffull, 0x800000ull, 0x800001ull, 1ull << 33};
    for (uint64_t j : J)
        for (uint64_t base : {0ull, 640ull + 17}) {
            Conn c(next_key(), base);
            for (uint64_t n : {1u, 2u, 3u, 64u, 65u, 130u, 4000u}) c.send(base + n, 2);
            c.send(base + j, 3);
            const uint64_t wb = c.ar.base();
            // around the new base, the old bits, the words that were cleared
            for (uint64_t n : {wb - 1, wb, wb + 1, base + 4000, base + 130, base + 65, base + 64, base + 3, wb + 63, wb + 64, base + j,
                               base + j - 1, base + j + 1})
                c.send(n, 3, 1);
            c.send(c.ar.largest() + 1, 0);
        }
}

// the rotation wraps past 4096 several times; reordering and repeats on the way
void rotation() {
    Conn c(next_key(), 5);
    uint64_t n = 5;
    for (unsigned k = 0; k < 260; ++k) {
        n += 100 + (k % 7);
        c.send(n, 1);
        if (k % 9 == 4) c.send(n - 30, 1);
        if (k % 13 == 6) c.send(n - 30, 2);
        if (k % 17 == 3) c.send(n - 4000, 2);
        if (k % 31 == 30) c.send(n - 4200, 2);  // below the base
    }
}

void repeats_and_tags() {
    Conn c(next_key(), 0x1000);
    c.send(0x1001, 1);
    c.send(0x1001, 1);
    c.send(0x1002, 2, 0, 0, 48, 1);   // corrupted: not accepted
    c.send(0x1002, 2);                // the same nonce, intact: accepted now
    c.send(0x1002, 2);
    for (unsigned bit = 1; bit <= 16; ++bit) c.send(0x1003, 3, 2, 0, 60, bit);
    c.send(0x1003, 3, 2, 0, 60);
    c.send(0x1005, 0);  // no nonce bytes, but the next expected is 0x1004: bad tag
    c.send(0x1004, 0);
    c.send(0x1004, 0);  // now means 0x1005
}

// "Ignored re-ordered": sequence bytes fewer than nonce bytes and the datagram older than the newest
void reordered_rule() {
    for (unsigned nb = 0; nb <= 3; ++nb)
        for (unsigned sb = 0; sb <= 3; ++sb) {
            Conn c(next_key(), 200);
            c.send(201, nb, sb);
            c.send(205, nb ? nb : 1, sb);
            c.send(203, nb ? nb : 1, sb);    // older than the newest
            c.send(204, nb ? nb : 1, sb, 1);
            c.send(206, nb ? nb : 1, sb);    // the newest: in order
            c.send(206, nb ? nb : 1, sb);
        }
}

// the order of a tick: a failed tag between two datagrams changes what the third expands to
void order_case() {
    for (unsigned corrupt = 0; corrupt < 2; ++corrupt) {
        Conn c(0x0123456789abcdefull, 100);
        c.send(101, 1);
        c.send(300, 2, 0, 0, 48, corrupt);
        c.send(110, 1);
        c.send(111, 0);
    }
}

void lengths_and_handshakes() {
    const unsigned lens[] = {6, 7, 8, 13, 14, 22, 23, 24, 37, 38, 39, 46, 70, 71, 134, 135, 262, 1306};
    for (int zero = 0; zero < 2; ++zero) {  // (the second time without a cipher: key 0)
        Conn c(zero ? 0 : next_key(), 0);
        uint64_t n = 0;
        for (unsigned bytes : lens)
            for (unsigned nb = 0; nb <= 3; ++nb)
                for (unsigned sb = 0; sb <= 3; sb += 3)
                    for (unsigned hs = 0; hs < 2; ++hs) {
                        if (6 + (hs ? 12 : 0) + nb + sb > bytes) continue;
                        c.send(++n, nb, sb, hs, bytes);
                    }
    }
}

}  // namespace

int main() {
    wraps();
    msb_gaps();
    reorder();
    jumps();
    rotation();
    repeats_and_tags();
    reordered_rule();
    order_case();
    lengths_and_handshakes();
    return 0;
}
