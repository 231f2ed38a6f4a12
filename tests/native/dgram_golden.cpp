// dgram_golden -- writes the recorded results of tests/golden/dgram_kat.txt.gz: datagrams built with
// the reference's own frame and footer writers in sendQueuedDatagram's order, and message sections
// walked with its ReadByteStream under ProcessDatagram's rules (mode 0) and resumeProcessing's
// (mode 1).  Test-only and not built by any test: tests/golden/make_dgram_kat.sh compiles it
// against the reference's headers and regenerates the fixture.
//
//   B seed seq_bytes nonce_bytes handshake flag_bits count {type bytes} x count
//     out_bytes message_bytes reliable_offset reliable_bytes fnv
//         one datagram.  Its inputs come from draws d(seed, c) = the low byte of mix(seed, c) with a
//         counter c that starts at 0 and moves by one per byte drawn:
//             seq, nonce (4 bytes each, little-endian), timestamp (3), handshake (12; drawn whether
//             attached or not), then every message's body in list order; a Padding message
//             (type 4) draws nothing: its body is zeros.  type 255: a raw body without a header.
//         fnv: FNV-1a-64 of the out_bytes bytes (the two tag bytes are zeros).
//   P gen a b c bytes {status count reliable_offset reliable_bytes fnv} x 2 (mode 0, mode 1)
//         one message section of `bytes` bytes made by generator `gen` (below) from a, b, c.
//         count: the frames walked before the end or the error; fnv: of all count table entries
//         type << 27 | bytes << 16 | payload_offset as little-endian 32-bit words.
//
//   mix(seed, c): h = seed ^ c * 0x9E3779B1; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35;
//                 h ^= h >> 16   (32-bit wrapping)
//
//   generators of P sections (draws from seed with a running counter, as above):
//     0  a = index of a B line (from 0, in file order): the message section of that datagram
//     1  a = o: a frame of type (o & 1 ? 6 : 3) with max(o, 2) - 2 body bytes, so that the second
//        header starts at byte max(o, 2); then a frame of type 6 with 7 bytes, then one of type 4
//        with 1 byte; bodies drawn from seed 1000 + o
//     2  a = n: n frames without a body, types 3 and 6 in turn
//     3  a = seed, b = bytes: drawn bytes as they come
//     4  a = frames, b = at, c = what: `a` frames, frame k of type kTypes[k % 6] with
//        (k * 5 + a) % 23 body bytes drawn from seed 4000 + a * 64 + b * 8 + c; then
//        c = 2: frame `at` announces 2047 bytes (its body is left as it is);
//        c = 3: the section ends after frame `at` - 1 and one more byte (0x5a);
//        c = 20, 30, 40: frame `at` is replaced by an AckAck (type 2) of 2, 3, 4 body bytes drawn
//        from that seed + 1000; what follows it moves
//     5  frames of type 6 with 2047 body bytes, then one that fills up to 65535 bytes; seed 5000
#include "TonkineseProtocol.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tonk;

namespace {

const uint32_t kLens[16] = {0, 1, 2, 13, 14, 15, 16, 17, 18, 29, 30, 31, 32, 33, 1300, 2047};
const uint32_t kFecLens[18] = {1, 2, 15, 16, 17, 63, 64, 127, 128, 129, 1023, 1024, 1025, 1300, 1535, 1536, 1537, 4000};
const uint32_t kTypes[6] = {3, 6, 0, 5, 31, 1};

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
    void fill(uint8_t* p, uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) p[i] = byte();
    }
};

uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

struct Msg { uint32_t type, bytes; };

struct Walked { unsigned status, count, rel_off, rel_bytes; uint64_t fnv; };

// ProcessDatagram's walk (TonkineseIncoming.cpp:269-411) with its three errors; mode 1 leaves the
// AckAck rule out (resumeProcessing, onCompressed).
Walked walk(const uint8_t* data, unsigned bytes, int mode) {
    Walked w = {0, 0, 0, 0, 0};
    unsigned reliableStartOffset = 0, reliableEndOffset = 0;
    std::vector<uint8_t> table;
    siamese::ReadByteStream frameReader(data, bytes);
    while (frameReader.Remaining() >= protocol::kMessageFrameBytes) {
        const unsigned frameStartOffset = frameReader.BytesRead;
        unsigned messageType = frameReader.Read16();
        const unsigned messageBytes = messageType & protocol::kMessageLengthMask;
        if (frameReader.Remaining() < messageBytes) { w.status = 2; break; }
        messageType >>= protocol::kMessageLengthBits;
        const unsigned payloadOffset = frameReader.BytesRead;
        frameReader.Read(messageBytes);
        if (mode == 0 && messageType == protocol::MessageType_AckAck && messageBytes != protocol::kAckAckBytes) { w.status = 4; break; }
        uint8_t e[4];
        siamese::WriteU32_LE(e, messageType << 27 | messageBytes << 16 | payloadOffset);
        table.insert(table.end(), e, e + 4);
        ++w.count;
        if (messageType >= protocol::MessageType_StartOfReliables) {
            if (reliableEndOffset == 0) reliableStartOffset = frameStartOffset;
            reliableEndOffset = frameReader.BytesRead;
        }
    }
    if (w.status == 0 && frameReader.Remaining() > 0) w.status = 3;
    if (reliableEndOffset > reliableStartOffset) {
        w.rel_off = reliableStartOffset;
        w.rel_bytes = reliableEndOffset - reliableStartOffset;
    }
    w.fnv = fnv1a(table.data(), table.size());
    return w;
}

std::vector<std::vector<uint8_t>> g_sections;  // the message sections of the B lines
std::vector<bool> g_only_fec;

void b_line(uint32_t seed, unsigned seqBytes, unsigned nonceBytes, bool handshake, unsigned flagBits, const std::vector<Msg>& msgs) {
    Draw d(seed);
    const uint32_t seq = d.word(4), nonce = d.word(4), ts24 = d.word(3);
    uint8_t hs[12];
    d.fill(hs, 12);
    std::vector<uint8_t> buf(70000 + 64, 0);
    uint8_t* datagramData = buf.data();
    unsigned messageBytes = 0;
    for (const Msg& m : msgs) {
        if (m.type != 255) {
            protocol::WriteMessageFrameHeader(datagramData + messageBytes, m.type, m.bytes);
            messageBytes += protocol::kMessageFrameBytes;
        }
        if (m.type == protocol::MessageType_Padding) memset(datagramData + messageBytes, 0, m.bytes);
        else d.fill(datagramData + messageBytes, m.bytes);
        messageBytes += m.bytes;
    }
    // sendQueuedDatagram (TonkineseOutgoing.cpp:602-640), PostRecovery for the OnlyFEC flag
    uint8_t* footer = datagramData + messageBytes;
    uint8_t flags = protocol::kConnectionMask;
    if (flagBits & protocol::kSeqCompMask) flags |= protocol::kSeqCompMask;
    if (flagBits & protocol::kOnlyFECMask) flags |= protocol::kOnlyFECMask;
    if (seqBytes > 0) {
        flags |= seqBytes;
        uint8_t tmp[4];
        protocol::WriteFooterField(tmp, seq, seqBytes);  // (it may write a whole word)
        memcpy(footer, tmp, seqBytes);
        footer += seqBytes;
    }
    {
        uint8_t tmp[4];
        protocol::WriteFooterField(tmp, nonce, nonceBytes);
        memcpy(footer, tmp, nonceBytes);
        flags |= nonceBytes << 2;
        footer += nonceBytes;
    }
    if (handshake) {
        flags |= protocol::kHandshakeMask;
        const uint32_t b = siamese::ReadU32_LE(hs + 8);
        const uint64_t a = siamese::ReadU64_LE(hs);
        siamese::WriteU64_LE(footer, a);
        siamese::WriteU32_LE(footer + 8, b);
        footer += protocol::kHandshakeBytes;
    }
    siamese::WriteU24_LE(footer, ts24);
    footer += protocol::kTimestampBytes;
    footer[0] = flags;
    ++footer;
    siamese::WriteU16_LE(footer, 0);
    footer += protocol::kEncryptionTagBytes;
    const unsigned total = (unsigned)(footer - datagramData);
    Walked w = {0, 0, 0, 0, 0};
    if (!(flagBits & protocol::kOnlyFECMask)) w = walk(datagramData, messageBytes, 0);
    printf("B %u %u %u %u %u %u", seed, seqBytes, nonceBytes, handshake ? 1u : 0u, flagBits, (unsigned)msgs.size());
    for (const Msg& m : msgs) printf(" %u %u", m.type, m.bytes);
    printf(" %u %u %u %u 0x%016llx\n", total, messageBytes, w.rel_off, w.rel_bytes, (unsigned long long)fnv1a(datagramData, total));
    g_sections.push_back(std::vector<uint8_t>(datagramData, datagramData + messageBytes));
    g_only_fec.push_back((flagBits & protocol::kOnlyFECMask) != 0);
}

void p_line(unsigned gen, unsigned a, unsigned b, unsigned c, const std::vector<uint8_t>& s) {
    printf("P %u %u %u %u %u", gen, a, b, c, (unsigned)s.size());
    for (int mode = 0; mode < 2; ++mode) {
        const Walked w = walk(s.data(), (unsigned)s.size(), mode);
        printf(" %u %u %u %u 0x%016llx", w.status, w.count, w.rel_off, w.rel_bytes, (unsigned long long)w.fnv);
    }
    printf("\n");
}

void frame(std::vector<uint8_t>& s, unsigned type, unsigned bytes, Draw* d) {
    uint8_t h[2];
    protocol::WriteMessageFrameHeader(h, type, bytes);
    s.insert(s.end(), h, h + 2);
    for (unsigned i = 0; i < bytes; ++i) s.push_back(d ? d->byte() : (uint8_t)0);
}

}  // namespace

int main() {
    uint32_t line = 0;
    // every footer shape with 1, 2 and 3 messages, and with 17 for sixteen of them; reliable types
    // where a sequence number is attached
    for (unsigned combo = 0; combo < 64; ++combo) {
        const unsigned seqBytes = combo & 3, nonceBytes = (combo >> 2) & 3;
        const bool hs = (combo >> 4) & 1;
        const unsigned flagBits = (combo >> 5) & 1 ? protocol::kSeqCompMask : 0;
        for (unsigned count : {1u, 2u, 3u, 17u}) {
            if (count == 17 && (combo & 3) != (combo >> 4)) continue;
            std::vector<Msg> msgs;
            for (unsigned k = 0; k < count; ++k) {
                const unsigned rel[5] = {6, 5, 7, 31, 20}, unrel[3] = {3, 1, 0};
                msgs.push_back(Msg{seqBytes ? rel[(line + k) % 5] : unrel[(line + k) % 3], kLens[(line * 5 + k * 3) % 16]});
            }
            b_line(100 + line, seqBytes, nonceBytes, hs, flagBits, msgs);
            ++line;
        }
    }
    // a Padding frame last, of every length; behind reliable data and behind unreliable data
    for (unsigned k = 0; k < 16; ++k) {
        b_line(100 + line, 1 + k % 3, k % 4, k & 1, 0, {Msg{6, kLens[(k + 5) % 16]}, Msg{7, 3}, Msg{4, kLens[k]}});
        ++line;
        b_line(100 + line, k % 4, 3, 0, protocol::kSeqCompMask, {Msg{3, kLens[(k + 9) % 16]}, Msg{4, kLens[k]}});
        ++line;
    }
    // unreliable, then reliable: the reliable span does not start at 0
    for (unsigned k = 0; k < 16; ++k) {
        b_line(100 + line, 1 + k % 3, 1, 0, 0, {Msg{3, kLens[k]}, Msg{2, 3}, Msg{6, kLens[(k + 3) % 16]}, Msg{5, kLens[(k + 7) % 16]}});
        ++line;
    }
    // OnlyFEC: one raw body
    for (unsigned k = 0; k < 18; ++k) {
        b_line(100 + line, 0, k % 4, k == 5, protocol::kOnlyFECMask | (k & 1 ? protocol::kSeqCompMask : 0), {Msg{255, kFecLens[k]}});
        ++line;
    }
    {  // 65535 bytes: 31 frames of 2047, one of 1990, the longest footer
        std::vector<Msg> msgs(31, Msg{6, 2047});
        msgs.push_back(Msg{7, 65535 - 24 - 31 * 2049 - 2});
        b_line(100 + line, 3, 3, true, protocol::kSeqCompMask, msgs);
        ++line;
    }

    for (unsigned i = 0; i < g_sections.size(); ++i)
        if (!g_only_fec[i]) p_line(0, i, 0, 0, g_sections[i]);  // (OnlyFEC datagrams are not parsed)
    for (unsigned o = 0; o <= 1400; ++o) {
        Draw d(1000 + o);
        std::vector<uint8_t> s;
        frame(s, o & 1 ? 6 : 3, (o < 2 ? 2 : o) - 2, &d);
        frame(s, 6, 7, &d);
        frame(s, 4, 1, &d);
        p_line(1, o, 0, 0, s);
    }
    {
        std::vector<uint8_t> s;
        for (unsigned k = 0; k < 675; ++k) frame(s, k & 1 ? 6 : 3, 0, nullptr);
        p_line(2, 675, 0, 0, s);
    }
    for (unsigned k = 0; k < 202; ++k) {
        const unsigned bytes = k < 2 ? k : 2 + (mix(77, k) % 1399);
        Draw d(3000 + k);
        std::vector<uint8_t> s(bytes);
        d.fill(s.data(), bytes);
        p_line(3, 3000 + k, bytes, 0, s);
    }
    for (unsigned frames : {1u, 5u, 9u})
        for (unsigned pick = 0; pick < (frames == 1 ? 1u : 3u); ++pick)  // the first, a middle and the last frame
            for (unsigned what : {2u, 3u, 20u, 30u, 40u}) {
                const unsigned at = pick == 0 ? 0u : pick == 1 ? frames / 2 : frames - 1;
                Draw d(4000 + frames * 64 + at * 8 + what);
                std::vector<uint8_t> s;
                std::vector<unsigned> starts;
                for (unsigned k = 0; k < frames; ++k) {
                    starts.push_back((unsigned)s.size());
                    frame(s, kTypes[k % 6], (k * 5 + frames) % 23, &d);
                }
                if (what == 2) protocol::WriteMessageFrameHeader(s.data() + starts[at], kTypes[at % 6], 2047);
                if (what == 3) {
                    s.resize(starts[at]);
                    s.push_back(0x5a);
                }
                if (what >= 20) {
                    // the frame is rewritten as an AckAck; what follows it moves
                    std::vector<uint8_t> t(s.begin(), s.begin() + starts[at]);
                    Draw e(d.seed + 1000);
                    frame(t, protocol::MessageType_AckAck, what / 10, &e);
                    if (at + 1 < frames) t.insert(t.end(), s.begin() + starts[at + 1], s.end());
                    s = t;
                }
                p_line(4, frames, at, what, s);
            }
    {
        Draw d(5000);
        std::vector<uint8_t> s;
        for (unsigned k = 0; k < 31; ++k) frame(s, 6, 2047, &d);
        frame(s, 6, 65535 - 31 * 2049 - 2, &d);
        p_line(5, 0, 0, 0, s);
    }
    return 0;
}
