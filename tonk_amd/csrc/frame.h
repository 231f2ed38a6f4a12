// frame.h -- moving packets between a caller's device buffers and arena rows (tonk_batch.h): the
// per-packet byte logic shared by the kernels (frame.hip), their host side (batch.cpp) and the
// serial host walk of the tests (tests/native/frame_check.cpp).
//
//   framed row   : varint(len) || payload || zeros to the row's capacity   (serial.h length header)
//   raw row      : packet || zeros to the row's capacity                    (a received recovery packet)
//
// The functions are written for `nl` cooperating lanes (lane = 0..nl-1) that all call them with
// the same arguments and share nothing: the 16-byte chunks of a row or a slot are strided over the
// lanes.  The kernels run them with one or a few waves per packet; on the host nl = 1 (the tests'
// walk also calls the 64, 128 and 256 lanes of a packet one after the other).  No libc.
//
// Memory is read in aligned 16-byte granules: a granule is read when at least one of its bytes
// belongs to the packet, so a read never leaves the aligned 16 bytes around the packet's first
// and last byte.  Rows are written with aligned 16-byte stores only; a caller's slot with aligned
// 16-byte stores where whole granules belong to the packet and single bytes at its two ends.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TAMD_FRAME_FN __host__ __device__ static inline
#else
#define TAMD_FRAME_FN static inline
#endif

// status of an unframed row: 0 or why nothing was written
#define TAMD_FRAME_OK 0u
#define TAMD_FRAME_E_HEADER 1u  // the row is empty, or its length header is longer than the row
#define TAMD_FRAME_E_EMPTY 2u   // the header announces 0 bytes
#define TAMD_FRAME_E_BOUND 3u   // header + length reach beyond the row's upper bound
#define TAMD_FRAME_E_PITCH 4u   // the length is more than a slot of the caller holds

// The framing kernels' launch shape: blocks of TAMD_FRAME_BLOCK threads, one, two or four waves of
// 64 lanes per packet (`wpp`) by the call's largest packet, whole packets per block.
#define TAMD_FRAME_BLOCK 256u
TAMD_FRAME_FN uint32_t tamd_frame_waves(uint32_t bytes) { return bytes <= 4096u ? 1u : bytes <= 16384u ? 2u : 4u; }
TAMD_FRAME_FN uint32_t tamd_frame_grid(uint64_t n, uint32_t wpp) { return (uint32_t)((n * wpp + 3u) / 4u); }
// (packet index, lane within the packet's 64 * wpp lanes) of thread `thread` of block `block`;
// wpp divides the waves of a block.
TAMD_FRAME_FN uint32_t tamd_frame_packet(uint32_t block, uint32_t thread, uint32_t wpp, uint32_t* lane) {
    const uint32_t wave = block * (TAMD_FRAME_BLOCK / 64u) + thread / 64u;
    *lane = (wave % wpp) * 64u + (thread & 63u);
    return wave / wpp;
}

typedef struct tamd_v16 { uint32_t w[4]; } __attribute__((aligned(16))) tamd_v16;

// One aligned 16-byte load / store (a single dwordx4 access on the device).
TAMD_FRAME_FN tamd_v16 tamd_ld16(uintptr_t at) {
    tamd_v16 v;
    __builtin_memcpy(&v, __builtin_assume_aligned((const void*)at, 16), 16);
    return v;
}
TAMD_FRAME_FN void tamd_st16(void* at, const tamd_v16& v) { __builtin_memcpy(__builtin_assume_aligned(at, 16), &v, 16); }

// The length header of a payload of `len` bytes (1 .. 0x1fffff): its byte count; *word holds the
// header bytes in row order from bit 0 (serial.h put_length_header).
TAMD_FRAME_FN uint32_t tamd_frame_header(uint32_t len, uint32_t* word) {
    if (len <= 0x7fu) { *word = len; return 1; }
    if (len <= 0x3fffu) { *word = (0x80u | (len >> 8)) | (len & 0xffu) << 8; return 2; }
    *word = (0xC0u | (len >> 16)) | ((len >> 8) & 0xffu) << 8 | (len & 0xffu) << 16;
    return 3;
}

// The header of a framed row whose first four bytes are `w0` (row order from bit 0), checked
// against the bytes the row may hold (`upper`) and a slot of the caller (`pitch`), as the C ABI's
// read-back checks it (serial.h get_length_header, then length 0 and length beyond the row).
TAMD_FRAME_FN uint32_t tamd_unframe_header(uint32_t w0, uint32_t upper, uint64_t pitch, uint32_t* hb, uint32_t* len) {
    *hb = 0;
    *len = 0;
    if (upper < 1) return TAMD_FRAME_E_HEADER;
    const uint32_t b0 = w0 & 0xffu, b1 = (w0 >> 8) & 0xffu, b2 = (w0 >> 16) & 0xffu, b3 = w0 >> 24;
    uint32_t h, l;
    if ((b0 >> 6) <= 1) { h = 1; l = b0; }
    else if ((b0 >> 6) == 2) { h = 2; l = ((b0 << 8) | b1) & 0x3fffu; }
    else if ((b0 & 0xE0u) == 0xC0u) { h = 3; l = ((b0 << 16) | (b1 << 8) | b2) & 0x1fffffu; }
    else { h = 4; l = ((b0 << 24) | (b1 << 16) | (b2 << 8) | b3) & 0x1fffffffu; }
    if (h > upper) return TAMD_FRAME_E_HEADER;
    if (l == 0) return TAMD_FRAME_E_EMPTY;
    if (l > upper - h) return TAMD_FRAME_E_BOUND;
    if (l > pitch) return TAMD_FRAME_E_PITCH;
    *hb = h;
    *len = l;
    return TAMD_FRAME_OK;
}

// The 16 bytes at address `at` (any alignment).  Only bytes inside [lo, hi) mean anything: the one
// or two aligned granules under the 16 bytes are read where they overlap [lo, hi) and count as
// zero where they do not.  The dword part of the shift is the same for every chunk of a packet
// (selects on a uniform value), the byte part is a funnel shift of neighbouring dwords.
TAMD_FRAME_FN tamd_v16 tamd_load16(uintptr_t at, uintptr_t lo, uintptr_t hi) {
    const uint32_t s = (uint32_t)(at & 15u);
    const uintptr_t g = at - s;
    tamd_v16 x = {{0, 0, 0, 0}}, y = {{0, 0, 0, 0}};
    if (g + 16 > lo && g < hi) x = tamd_ld16(g);
    if (s == 0) return x;
    if (g + 32 > lo && g + 16 < hi) y = tamd_ld16(g + 16);
    const uint32_t q = s >> 2, r = (s & 3u) * 8u;
    const uint32_t t0 = q == 0 ? x.w[0] : q == 1 ? x.w[1] : q == 2 ? x.w[2] : x.w[3];
    const uint32_t t1 = q == 0 ? x.w[1] : q == 1 ? x.w[2] : q == 2 ? x.w[3] : y.w[0];
    const uint32_t t2 = q == 0 ? x.w[2] : q == 1 ? x.w[3] : q == 2 ? y.w[0] : y.w[1];
    const uint32_t t3 = q == 0 ? x.w[3] : q == 1 ? y.w[0] : q == 2 ? y.w[1] : y.w[2];
    const uint32_t t4 = q == 0 ? y.w[0] : q == 1 ? y.w[1] : q == 2 ? y.w[2] : y.w[3];
    tamd_v16 o;
    o.w[0] = (uint32_t)((((uint64_t)t1 << 32) | t0) >> r);
    o.w[1] = (uint32_t)((((uint64_t)t2 << 32) | t1) >> r);
    o.w[2] = (uint32_t)((((uint64_t)t3 << 32) | t2) >> r);
    o.w[3] = (uint32_t)((((uint64_t)t4 << 32) | t3) >> r);
    return o;
}

// Chunk `c` (row bytes [16c, 16c + 16)) of the row that frames the `len` bytes at `src` behind a
// header of `hb` bytes (`hword`; hb 0: a raw row): header bytes, then payload byte p - hb at row
// byte p, then zeros.
TAMD_FRAME_FN tamd_v16 tamd_frame_chunk(uintptr_t src, uint32_t len, uint32_t hb, uint32_t hword, uint32_t c) {
    const uint32_t p0 = 16u * c, end = hb + len;
    tamd_v16 v = {{0, 0, 0, 0}};
    if (p0 >= end) return v;
    v = tamd_load16(src + p0 - hb, src, src + len);
    if (end - p0 < 16u) {  // the packet's last chunk: zeros from row byte `end`
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t pos = p0 + 4u * k;
            const uint32_t keep = end > pos ? end - pos : 0u;
            if (keep < 4u) v.w[k] = keep ? v.w[k] & (0xffffffffu >> (32u - 8u * keep)) : 0u;
        }
    }
    if (c == 0 && hb) v.w[0] = (v.w[0] & ~((1u << (8u * hb)) - 1u)) | hword;
    return v;
}

// Lane `lane` of `nl`: its chunks of the row of `cap` bytes (a multiple of 16, at least hb + len)
// at `row`, which must be 16-byte aligned.  Nothing is written when the packet would not fit.
TAMD_FRAME_FN void tamd_frame_row(uint8_t* row, uint32_t cap, const uint8_t* src, uint32_t len, uint32_t raw,
                                  uint32_t lane, uint32_t nl) {
    uint32_t hword = 0;
    const uint32_t hb = raw ? 0u : tamd_frame_header(len, &hword);
    if (len == 0 || len > 0x1fffffu || hb + len > cap) return;
    for (uint32_t c = lane; c < cap / 16u; c += nl) tamd_st16(row + 16u * c, tamd_frame_chunk((uintptr_t)src, len, hb, hword, c));
}

// Lane `lane` of `nl`: its part of dst[i] = row[hb + i], i < len (the caller has checked the
// header: hb + len lie inside the row).  `row` is 16-byte aligned; no byte outside dst[0, len) is
// written.
TAMD_FRAME_FN void tamd_unframe_row(uint8_t* dst, const uint8_t* row, uint32_t hb, uint32_t len, uint32_t lane,
                                    uint32_t nl) {
    uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;  // bytes before the slot's first granule
    if (head > len) head = len;
    const uint32_t n16 = (len - head) / 16u;
    const uintptr_t from = (uintptr_t)row + hb, hi = from + len;
    for (uint32_t c = lane; c < n16; c += nl)
        tamd_st16(dst + head + 16u * c, tamd_load16(from + head + 16u * c, (uintptr_t)row, hi));
    for (uint32_t i = lane; i < head; i += nl) dst[i] = row[hb + i];
    for (uint32_t i = head + 16u * n16 + lane; i < len; i += nl) dst[i] = row[hb + i];
}

// The last min(total, 8) bytes of the packet of `total` bytes at `src`, zero filled to 8.
TAMD_FRAME_FN void tamd_tail8(const uint8_t* src, uint32_t total, uint8_t* out) {
    const uint32_t tl = total < 8u ? total : 8u;
    for (uint32_t k = 0; k < 8u; ++k) out[k] = k < tl ? src[total - tl + k] : (uint8_t)0;
}

// Lane `lane` of `nl`: its part of unframing record d[i] (kernel_abi.h UnframeDesc: the slot, the
// row in 64-byte units from `arena`, the bytes the row may hold): the header check, then with
// `write` the payload into the slot, then (lane 0) out[i].  A raw record copies `upper` bytes as
// they are.  Without `write` only out[i] is written: the caller learns every length and status
// before any payload moves.
template <class Desc, class Out>
TAMD_FRAME_FN void tamd_unframe_packet(const Desc* d, uint32_t i, const uint8_t* arena, uint64_t pitch, Out* out,
                                       uint32_t write, uint32_t lane, uint32_t nl) {
    const uint8_t* row = arena + (uint64_t)d[i].row * 64u;
    const uint32_t upper = d[i].upper;
    uint32_t hb = 0, len = upper, status = TAMD_FRAME_OK;
    if (!d[i].raw) {
        uint32_t w0 = 0;
        if (upper) __builtin_memcpy(&w0, __builtin_assume_aligned(row, 4), 4);
        status = tamd_unframe_header(w0, upper, pitch, &hb, &len);
    } else if (len > pitch) {
        status = TAMD_FRAME_E_PITCH;
    }
    if (status == TAMD_FRAME_OK && write) tamd_unframe_row((uint8_t*)d[i].dst, row, hb, len, lane, nl);
    if (lane == 0) {
        out[i].len = status == TAMD_FRAME_OK ? len : 0u;
        out[i].status = status;
    }
}
