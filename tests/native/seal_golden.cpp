// seal_golden -- writes the known answers of tests/golden/seal_kat.txt.gz: what the reference's
// security::SimpleCipher computes for the cases below.  Test-only and not built by any test:
// tests/golden/make_seal_kat.sh compiles it against the reference's SimpleCipher and t1ha and
// regenerates the fixture.
//
//   C key seq len msg tag fnv           Cipher over the first msg bytes, Tag over len bytes of the
//                                       result, FNV-1a-64 of those len bytes
//   I key data tag                      TagInt
//   D key seq bytes msg ts24 flags fnv  a whole connected datagram sealed as Tonk's sender does:
//                                       Cipher(msg), Tag(bytes - 6) ^ TagInt(ts24 << 8 | flags),
//                                       timestamp, flags and tag written; FNV of all bytes
//
// Byte i of a case is (i * 131 + len * 7 + msg * 13 + 1) & 255 (len = bytes for a D line; the six
// untagged bytes are then overwritten).
#include "SimpleCipher.h"

#include <stdint.h>
#include <stdio.h>
#include <vector>

namespace {

const uint64_t kKeys[5] = {0, 0x0123456789abcdefull, 0xffffffff00000001ull, 0x00000000deadbeefull, 0x8000000000000000ull};
const uint64_t kSeqs[5] = {0, 1, 0xffffffffull, 0x100000000ull, 0xabcdef0123456789ull};
const uint32_t kLong[] = {255, 256, 257, 1023, 1024, 1025, 1300, 1311, 1500, 4000, 65535};
const uint32_t kDatagrams[] = {6, 7, 8, 13, 14, 22, 23, 37, 38, 39, 46, 70, 71, 134, 135, 262, 1306, 1311, 4006, 65535};

uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

void fill(std::vector<uint8_t>& b, uint32_t len, uint32_t msg) {
    b.resize(len);
    for (uint32_t i = 0; i < len; ++i) b[i] = (uint8_t)(i * 131u + len * 7u + msg * 13u + 1u);
}

// each of {0, len, len / 2, len - 1, 17 (or `extra`)} that is <= len, once
std::vector<uint32_t> msgs(uint32_t len, uint32_t extra) {
    const int64_t c[5] = {0, len, len / 2, (int64_t)len - 1, extra};
    std::vector<uint32_t> out;
    for (int64_t m : c) {
        bool seen = m < 0 || m > (int64_t)len;
        for (uint32_t o : out) seen = seen || o == (uint32_t)m;
        if (!seen) out.push_back((uint32_t)m);
    }
    return out;
}

// all 25 key/sequence pairs up to `all`, two that move with the length beyond
std::vector<uint32_t> pairs(uint32_t len, uint32_t all) {
    std::vector<uint32_t> out;
    if (len <= all)
        for (uint32_t p = 0; p < 25; ++p) out.push_back(p);
    else {
        out.push_back(5 + (len * 7u) % 20u);  // (a non-zero key)
        out.push_back((len * 7u + 11u) % 25u);
    }
    return out;
}

void cipher_case(uint32_t p, uint32_t len, uint32_t msg) {
    std::vector<uint8_t> b;
    fill(b, len, msg);
    security::SimpleCipher c;
    c.Initialize(kKeys[p / 5]);
    c.Cipher(b.data(), msg, kSeqs[p % 5]);
    const unsigned tag = c.Tag(b.data(), len, kSeqs[p % 5]);
    printf("C 0x%llx 0x%llx %u %u 0x%04x 0x%016llx\n", (unsigned long long)kKeys[p / 5], (unsigned long long)kSeqs[p % 5], len,
           msg, tag, (unsigned long long)fnv1a(b.data(), len));
}

void datagram_case(uint32_t p, uint32_t bytes, uint32_t msg) {
    std::vector<uint8_t> b;
    fill(b, bytes, msg);
    const uint32_t T = bytes - 6;
    const uint32_t ts24 = (bytes * 2654435761u + msg * 40503u + p) & 0xffffffu;
    const uint8_t flags = (uint8_t)(bytes * 7u + msg * 3u + 0x80u + p);
    const uint64_t nonce = kSeqs[p % 5];
    security::SimpleCipher c;
    c.Initialize(kKeys[p / 5]);
    c.Cipher(b.data(), msg, nonce);
    uint16_t tag = c.Tag(b.data(), T, nonce);
    tag ^= c.TagInt(ts24 << 8 | flags);
    b[T] = (uint8_t)ts24;
    b[T + 1] = (uint8_t)(ts24 >> 8);
    b[T + 2] = (uint8_t)(ts24 >> 16);
    b[T + 3] = flags;
    b[T + 4] = (uint8_t)tag;
    b[T + 5] = (uint8_t)(tag >> 8);
    printf("D 0x%llx 0x%llx %u %u %u %u 0x%016llx\n", (unsigned long long)kKeys[p / 5], (unsigned long long)nonce, bytes, msg, ts24,
           (unsigned)flags, (unsigned long long)fnv1a(b.data(), bytes));
}

}  // namespace

int main() {
    std::vector<uint32_t> lens;
    for (uint32_t l = 0; l <= 130; ++l) lens.push_back(l);
    for (uint32_t l : kLong) lens.push_back(l);
    for (uint32_t len : lens)
        for (uint32_t p : pairs(len, 40))
            for (uint32_t msg : msgs(len, 17)) cipher_case(p, len, msg);
    const uint32_t ints[] = {0, 1, 0x80, 0xff, 0x12345678, 0xffffff00, 0xffffffff, 0xabcdef80};
    for (uint64_t key : kKeys)
        for (uint32_t v : ints) {
            security::SimpleCipher c;
            c.Initialize(key);
            printf("I 0x%llx 0x%x 0x%04x\n", (unsigned long long)key, v, (unsigned)c.TagInt(v));
        }
    for (uint32_t bytes : kDatagrams) {
        const uint32_t T = bytes - 6;
        for (uint32_t p : pairs(bytes, 46))
            for (uint32_t msg : msgs(T, T >= 12 ? T - 12 : 17)) datagram_case(p, bytes, msg);
    }
    return 0;
}
