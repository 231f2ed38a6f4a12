// frame_check -- the byte logic of the framing kernels (tonk_amd/csrc/frame.h) as a serial host
// walk: one lane, or the 64, 128 and 256 lanes of one, two and four waves called one after the other
// with the same arguments, run exactly the functions the kernels run.  Test-only; built
// plain and under the address and undefined-behaviour sanitizers (frame.mk) and run by
// tests/test_batch.py.
//
//   frame_check                 every check below, the row and slot checks at each lane count; prints
//                               "ok <cases>" or the first failure
//   frame_check headers <file>  for len 1..70000: 4 bytes each, the header's byte count then its
//                               bytes (zero padded), for the comparison with the oracle's
//   frame_check rows <file>     the framed rows of the length x misalignment cases, back to back
//                               (each over its capacity), for the same comparison
//
// Expected values come from serial.h (the control plane's own length header), not from frame.h.
#include "../../tonk_amd/csrc/kernel_abi.h"
#include "../../tonk_amd/csrc/frame.h"
#include "../../tonk_amd/csrc/serial.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

const uint32_t kLens[] = {1, 2, 15, 16, 17, 63, 64, 127, 128, 129, 1023, 1024, 1025, 1300,
                          1535, 1536, 1537, 4000, 16383, 16384, 65535};
const uint32_t kGuard = 64;

int fail(const char* what, long a = 0, long b = 0, long c = 0) {
    printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

// (tests/test_batch.py builds the same bytes)
uint8_t payload_byte(uint32_t len, uint32_t mis, uint32_t i) { return (uint8_t)(i * 131u + len * 7u + mis * 13u + 1u); }

uint32_t row_cap(uint32_t len) { return (len + 3u + 63u) / 64u * 64u; }

// 16-byte aligned storage with room for the aligned granules around any packet inside it
struct Aligned {
    uint8_t* p;
    explicit Aligned(size_t n) : p((uint8_t*)aligned_alloc(64, (n + 63) / 64 * 64)) {}
    ~Aligned() { free(p); }
};

// The payload at misalignment `mis` inside `buf` (guards of 0xA5 around it); returns its address.
uint8_t* place(Aligned& buf, uint32_t len, uint32_t mis) {
    memset(buf.p, 0xA5, kGuard + 16 + len + kGuard);
    uint8_t* src = buf.p + kGuard + mis;
    for (uint32_t i = 0; i < len; ++i) src[i] = payload_byte(len, mis, i);
    return src;
}

// the lanes of a packet: the serial walk, then one, two and four waves (frame.h tamd_frame_waves)
const uint32_t kLanes[] = {1, 64, 128, 256};

// One packet into its row, every lane of `nl` in turn.
void frame_one(uint8_t* row, uint32_t cap, const uint8_t* src, uint32_t len, uint32_t raw, uint32_t nl) {
    for (uint32_t lane = 0; lane < nl; ++lane) tamd_frame_row(row, cap, src, len, raw, lane, nl);
}

// One record through the kernel's flow, every lane of `nl` in turn.
UnframeOut unframe_one(const std::vector<UnframeDesc>& d, uint32_t i, const uint8_t* arena, uint64_t pitch, uint32_t nl,
                       uint32_t write = 1) {
    std::vector<UnframeOut> out(d.size(), UnframeOut{0xdeadu, 0xdeadu});
    for (uint32_t lane = 0; lane < nl; ++lane) tamd_unframe_packet(d.data(), i, arena, pitch, out.data(), write, lane, nl);
    return out[i];
}

bool all_a5(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (p[i] != 0xA5) return false;
    return true;
}

int check_headers() {
    for (uint32_t len = 1; len <= 70000; ++len) {
        uint32_t word = 0, hb2 = 0, len2 = 0;
        const uint32_t hb = tamd_frame_header(len, &word);
        uint8_t want[4] = {0, 0, 0, 0};
        const unsigned wn = tamd::put_length_header(len, want);
        uint32_t ww = want[0] | want[1] << 8 | want[2] << 16 | (uint32_t)want[3] << 24;
        if (hb != wn || word != ww) return fail("header encode", len, hb, wn);
        if (tamd_unframe_header(word, hb + len, len, &hb2, &len2) != TAMD_FRAME_OK || hb2 != hb || len2 != len)
            return fail("header round trip", len, hb2, len2);
    }
    return 0;
}

int check_rows(long* cases, uint32_t nl) {
    Aligned src_buf(kGuard * 2 + 32 + 65535), dst_buf(kGuard * 2 + 32 + 65535), arena(row_cap(65535) + 64);
    for (uint32_t len : kLens)
        for (uint32_t mis = 0; mis < 16; ++mis) {
            const uint8_t* src = place(src_buf, len, mis);
            const uint32_t cap = row_cap(len);
            uint8_t* row = arena.p;
            memset(row, 0xEE, cap + 64);
            frame_one(row, cap, src, len, 0, nl);
            uint8_t hdr[4];
            const uint32_t hb = tamd::put_length_header(len, hdr);
            if (memcmp(row, hdr, hb)) return fail("framed header", len, mis, nl);
            if (memcmp(row + hb, src, len)) return fail("framed payload", len, mis, nl);
            for (uint32_t z = hb + len; z < cap; ++z)
                if (row[z]) return fail("framed zeros", len, mis, z);
            for (uint32_t z = cap; z < cap + 64; ++z)
                if (row[z] != 0xEE) return fail("write past the row", len, mis, z);
            // back into a slot at every misalignment of the destination for the short lengths, a few otherwise
            for (uint32_t dm = 0; dm < 16; dm += (len <= 129 ? 1 : 5)) {
                memset(dst_buf.p, 0xA5, kGuard * 2 + 32 + len);
                uint8_t* dst = dst_buf.p + kGuard + dm;
                std::vector<UnframeDesc> d(1, UnframeDesc{(uint64_t)(uintptr_t)dst, 0, hb + len, 0, 0});
                // (the upper bound a decoder knows may be larger than the packet: try both)
                for (uint32_t slack = 0; slack < 2; ++slack) {
                    d[0].upper = hb + len + (slack && hb + len + 9 <= cap ? 9 : 0);
                    const UnframeOut o = unframe_one(d, 0, arena.p, len, nl);
                    if (o.status != TAMD_FRAME_OK || o.len != len) return fail("unframe status", len, mis, o.status);
                    if (memcmp(dst, src, len)) return fail("unframed payload", len, mis, nl);
                    if (!all_a5(dst_buf.p, kGuard + dm) || !all_a5(dst + len, kGuard + 32 - dm))
                        return fail("unframe wrote outside the payload", len, mis, dm);
                }
                ++*cases;
            }
            // a raw row (a recovery packet): no header either way
            memset(row, 0xEE, cap + 64);
            frame_one(row, cap, src, len, 1, nl);
            if (memcmp(row, src, len)) return fail("raw row", len, mis, nl);
            for (uint32_t z = len; z < cap; ++z)
                if (row[z]) return fail("raw zeros", len, mis, z);
            memset(dst_buf.p, 0xA5, kGuard * 2 + 32 + len);
            uint8_t* dst = dst_buf.p + kGuard + (mis * 7 + 3) % 16;
            std::vector<UnframeDesc> d(1, UnframeDesc{(uint64_t)(uintptr_t)dst, 0, len, 1, 0});
            const UnframeOut o = unframe_one(d, 0, arena.p, len, nl);
            if (o.status != TAMD_FRAME_OK || o.len != len || memcmp(dst, src, len)) return fail("raw copy out", len, mis, nl);
            if (!all_a5(dst_buf.p, (size_t)(dst - dst_buf.p)) || !all_a5(dst + len, kGuard)) return fail("raw copy outside", len, mis);
            // the footer gather
            uint8_t tail[8], want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            tamd_tail8(src, len, tail);
            const uint32_t tl = len < 8 ? len : 8;
            memcpy(want, src + len - tl, tl);
            if (memcmp(tail, want, 8)) return fail("tail", len, mis);
            ++*cases;
        }
    return 0;
}

// The lanes share the work and nothing else: over the lanes of a packet every byte of the row, and
// every byte of the slot, is written by exactly one lane.  Each lane runs alone on a poisoned copy;
// a byte counts as written by it when it differs from the poison afterwards (a byte whose value is
// the poison's shows in no lane: at most one then).
int check_one_writer(long* cases, uint32_t nl) {
    Aligned src_buf(kGuard * 2 + 32 + 65535), dst_buf(kGuard * 2 + 32 + 65535), arena(row_cap(65535)), framed(row_cap(65535));
    std::vector<uint16_t> writers(row_cap(65535));
    for (uint32_t len : kLens)
        for (uint32_t mis = 0; mis < 16; ++mis) {
            const uint8_t* src = place(src_buf, len, mis);
            const uint32_t cap = row_cap(len);
            frame_one(framed.p, cap, src, len, 0, 1);
            writers.assign(cap, 0);
            for (uint32_t lane = 0; lane < nl; ++lane) {
                memset(arena.p, 0xEE, cap);
                tamd_frame_row(arena.p, cap, src, len, 0, lane, nl);
                for (uint32_t z = 0; z < cap; ++z)
                    if (arena.p[z] != 0xEE) {
                        if (arena.p[z] != framed.p[z]) return fail("a lane's row byte", len, mis, z);
                        ++writers[z];
                    }
            }
            for (uint32_t z = 0; z < cap; ++z)
                if (writers[z] != (framed.p[z] != 0xEE ? 1 : 0)) return fail("row byte not written by exactly one lane", len, nl, z);
            const uint32_t hb = len <= 0x7fu ? 1u : len <= 0x3fffu ? 2u : 3u;
            uint8_t* dst = dst_buf.p + kGuard + (mis * 7 + 3) % 16;
            std::vector<UnframeDesc> d(1, UnframeDesc{(uint64_t)(uintptr_t)dst, 0, hb + len, 0, 0});
            UnframeOut out[1];
            writers.assign(cap, 0);
            for (uint32_t lane = 0; lane < nl; ++lane) {
                memset(dst_buf.p, 0xA5, kGuard * 2 + 32 + len);
                tamd_unframe_packet(d.data(), 0, framed.p, len, out, 1, lane, nl);
                if (!all_a5(dst_buf.p, (size_t)(dst - dst_buf.p)) || !all_a5(dst + len, kGuard))
                    return fail("a lane wrote outside the payload", len, mis, lane);
                for (uint32_t z = 0; z < len; ++z)
                    if (dst[z] != 0xA5) {
                        if (dst[z] != src[z]) return fail("a lane's slot byte", len, mis, z);
                        ++writers[z];
                    }
            }
            for (uint32_t z = 0; z < len; ++z)
                if (writers[z] != (src[z] != 0xA5 ? 1 : 0)) return fail("slot byte not written by exactly one lane", len, nl, z);
            ++*cases;
        }
    return 0;
}

// Rows that must be rejected with nothing written.
int check_rejects(long* cases, uint32_t nl) {
    Aligned arena(4 * 256), dst_buf(kGuard * 2 + 256);
    struct Case { const char* name; uint8_t b[4]; uint32_t upper; uint64_t pitch; uint32_t want; };
    const Case cs[] = {
        {"empty row", {5, 0, 0, 0}, 0, 100, TAMD_FRAME_E_HEADER},
        {"2-byte header in a 1-byte row", {0x81, 0x00, 0, 0}, 1, 1000, TAMD_FRAME_E_HEADER},
        {"3-byte header in a 2-byte row", {0xC0, 0x40, 0x00, 0}, 2, 100000, TAMD_FRAME_E_HEADER},
        {"4-byte header in a 3-byte row", {0xE0, 0x00, 0x00, 0x05}, 3, 100000, TAMD_FRAME_E_HEADER},
        {"length 0", {0, 1, 2, 3}, 64, 100, TAMD_FRAME_E_EMPTY},
        {"length 0, 2-byte header", {0x80, 0, 2, 3}, 64, 100, TAMD_FRAME_E_EMPTY},
        {"length + header one more than the upper bound", {100, 0, 0, 0}, 100, 1000, TAMD_FRAME_E_BOUND},
        {"the same, 2-byte header", {0x80, 200, 0, 0}, 201, 1000, TAMD_FRAME_E_BOUND},
        {"length one more than the pitch", {100, 0, 0, 0}, 200, 99, TAMD_FRAME_E_PITCH},
    };
    for (const Case& c : cs) {
        memset(arena.p, 0x11, 4 * 256);
        memcpy(arena.p, c.b, 4);
        memset(dst_buf.p, 0xA5, kGuard * 2 + 256);
        std::vector<UnframeDesc> d(1, UnframeDesc{(uint64_t)(uintptr_t)(dst_buf.p + kGuard), 0, c.upper, 0, 0});
        for (uint32_t write = 0; write < 2; ++write) {
            const UnframeOut o = unframe_one(d, 0, arena.p, c.pitch, nl, write);
            if (o.status != c.want || o.len != 0) return fail(c.name, o.status, c.want, write);
        }
        if (!all_a5(dst_buf.p, kGuard * 2 + 256)) return fail("a rejected row was written");
        ++*cases;
    }
    {  // exactly at the bounds: accepted
        memset(arena.p, 0x22, 256);
        arena.p[0] = 100;
        memset(dst_buf.p, 0xA5, kGuard * 2 + 256);
        std::vector<UnframeDesc> d(1, UnframeDesc{(uint64_t)(uintptr_t)(dst_buf.p + kGuard), 0, 101, 0, 0});
        const UnframeOut c = unframe_one(d, 0, arena.p, 100, nl, 0);  // the check alone: lengths, nothing written
        if (c.status != TAMD_FRAME_OK || c.len != 100 || !all_a5(dst_buf.p, kGuard * 2 + 256)) return fail("check only", c.status, c.len);
        const UnframeOut o = unframe_one(d, 0, arena.p, 100, nl);
        if (o.status != TAMD_FRAME_OK || o.len != 100 || memcmp(dst_buf.p + kGuard, arena.p + 1, 100)) return fail("exact bounds", o.status, o.len);
        d[0].raw = 1;  // a raw record longer than the slot
        const UnframeOut r = unframe_one(d, 0, arena.p, 100, nl);
        if (r.status != TAMD_FRAME_E_PITCH) return fail("raw past the pitch", r.status);
        ++*cases;
    }
    {  // a packet that does not fit its row is not framed
        Aligned src(256);
        memset(arena.p, 0xEE, 256);
        memset(src.p, 1, 256);
        frame_one(arena.p, 64, src.p, 64, 0, nl);
        for (uint32_t i = 0; i < 256; ++i)
            if (arena.p[i] != 0xEE) return fail("framed a packet larger than its row", i);
        ++*cases;
    }
    return 0;
}

// The kernels' launch shape (frame.h, used by frame.hip and batch.cpp): over the grid of n packets at
// wpp waves each, every (packet, lane) pair of the n * 64 * wpp is some thread's exactly once, and
// the threads beyond packet n - 1 (which return) are the only others.
int check_launch_shape(long* cases) {
    if (tamd_frame_waves(4096) != 1 || tamd_frame_waves(4097) != 2 || tamd_frame_waves(16384) != 2 || tamd_frame_waves(16385) != 4 ||
        tamd_frame_waves(1) != 1 || tamd_frame_waves(65535 + 11) != 4)
        return fail("waves per packet");
    const uint32_t ns[] = {1, 2, 3, 5, 8};
    for (uint32_t wpp = 1; wpp <= 4; wpp *= 2)
        for (uint32_t n : ns) {
            const uint32_t nl = 64u * wpp, grid = tamd_frame_grid(n, wpp);
            if ((uint64_t)grid * TAMD_FRAME_BLOCK < (uint64_t)n * nl || (uint64_t)(grid - 1) * TAMD_FRAME_BLOCK >= (uint64_t)n * nl)
                return fail("grid", wpp, n, grid);
            std::vector<uint32_t> seen((size_t)n * nl, 0);
            for (uint32_t block = 0; block < grid; ++block)
                for (uint32_t thread = 0; thread < TAMD_FRAME_BLOCK; ++thread) {
                    uint32_t lane = ~0u;
                    const uint32_t i = tamd_frame_packet(block, thread, wpp, &lane);
                    if (lane >= nl) return fail("lane out of range", wpp, n, lane);
                    if (i < n) ++seen[(size_t)i * nl + lane];
                }
            for (size_t k = 0; k < seen.size(); ++k)
                if (seen[k] != 1) return fail("(packet, lane) not visited exactly once", wpp, n, (long)k);
            ++*cases;
        }
    return 0;
}

int dump_headers(const char* path) {
    FILE* f = fopen(path, "wb");
    if (!f) return fail("open");
    for (uint32_t len = 1; len <= 70000; ++len) {
        uint32_t word = 0;
        const uint32_t hb = tamd_frame_header(len, &word);
        const uint8_t rec[4] = {(uint8_t)hb, (uint8_t)word, (uint8_t)(word >> 8), (uint8_t)(word >> 16)};
        fwrite(rec, 1, 4, f);
    }
    fclose(f);
    return 0;
}

int dump_rows(const char* path) {
    FILE* f = fopen(path, "wb");
    if (!f) return fail("open");
    Aligned src_buf(kGuard * 2 + 32 + 65535), arena(row_cap(65535));
    for (uint32_t len : kLens)
        for (uint32_t mis = 0; mis < 16; ++mis) {
            const uint8_t* src = place(src_buf, len, mis);
            memset(arena.p, 0xEE, row_cap(len));
            frame_one(arena.p, row_cap(len), src, len, 0, 1);
            fwrite(arena.p, 1, row_cap(len), f);
        }
    fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "headers")) return dump_headers(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "rows")) return dump_rows(argv[2]);
    long cases = 0;
    if (check_headers() || check_launch_shape(&cases)) return 1;
    for (uint32_t nl : kLanes)
        if (check_rows(&cases, nl) || check_rejects(&cases, nl) || (nl > 1 && check_one_writer(&cases, nl))) return 1;
    printf("ok %ld\n", cases);
    return 0;
}
