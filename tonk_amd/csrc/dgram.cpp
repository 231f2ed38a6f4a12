// dgram.cpp -- include/tonk_datagram.h: batched building and parsing of datagrams in the caller's
// device memory.  A handle is the shared core (handle.h: lock, stream, pinned descriptor and result
// staging); it has no per-connection state.  Every call is one descriptor copy, one launch of a
// kernel of dgram.hip, one result copy (parse) and one wait.  The layout of a datagram -- every
// message's offset, the spans, the footer's bytes -- is computed here from lengths the caller gave
// (dgram.h tamd_dgram_layout, tamd_dgram_footer); the device moves the bytes.
#include "../../include/tonk_datagram.h"

#include "dgram.h"
#include "handle.h"
#include "kernel_abi.h"

#include <memory>

using namespace tamd;

namespace {

enum { kBuild = 0, kParse = 1, kKinds = 2 };

struct Framer {
    HandleCore core;
    tamd_dgram_params prm;
    std::vector<uint32_t> offs;  // a call's message offsets
};

}  // namespace

extern "C" {

void* tamd_dgram_create(const tamd_dgram_params* p, char* err, size_t err_len) {
    if (!p || p->max_datagram_bytes < 8 || p->max_datagram_bytes > 65535) return fail(err, err_len, "bad parameters");
    std::string why = device_check(p->device, "datagrams are built and parsed");
    if (!why.empty()) return fail(err, err_len, why);
    std::unique_ptr<Framer> s(new Framer());
    s->prm = *p;
    why = s->core.open(p->device);
    if (!why.empty()) return fail(err, err_len, why);
    return s.release();
}

void tamd_dgram_destroy(void* h) { destroy<Framer>(h); }
const char* tamd_dgram_error(void* h) { return error_text<Framer>(h); }
void tamd_dgram_set_timing(void* h, int on) { set_timing<Framer>(h, on); }
void tamd_dgram_kernel_ms(void* h, double* out, unsigned n) { kernel_ms<Framer>(h, out, n, kKinds); }

int tamd_dgram_build(void* h, uint32_t n, uint32_t m, const uint32_t* dgram, const uint32_t* type, const uint32_t* bytes,
                     const uint64_t* src, const uint32_t* seq, const uint32_t* seq_bytes, const uint32_t* nonce,
                     const uint32_t* nonce_bytes, const uint8_t* handshake, const uint8_t* has_handshake,
                     const uint32_t* timestamp24, const uint32_t* flag_bits, void* dev_out, uint64_t pitch,
                     uint32_t* out_bytes, uint32_t* message_bytes, uint32_t* reliable_offset, uint32_t* reliable_bytes,
                     int32_t* rc) {
    Framer* s = (Framer*)h;
    if (!s || !dev_out || (m && (!dgram || !type || !bytes || !src)) || (handshake && !has_handshake) ||
        (n && (!seq || !seq_bytes || !nonce || !nonce_bytes || !timestamp24 || !flag_bits || !out_bytes || !message_bytes ||
               !reliable_offset || !reliable_bytes || !rc)))
        return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk)) return e;
    HandleCore& c = s->core;
    for (uint32_t j = 0; j < m; ++j)
        if (dgram[j] >= n || (j && dgram[j] < dgram[j - 1])) return -2;
    if (pitch < tamd_dgram_footer_bytes(0, 0, 0)) return -3;
    if (!n) return 0;
    if (!c.room((size_t)m * sizeof(DgramMsg) + (size_t)n * sizeof(DgramFoot), 0)) return -4;
    s->offs.resize(m ? m : 1u);
    // (the footers start where the longest possible message list ends: 24 m is a multiple of 8)
    DgramMsg* dm = (DgramMsg*)c.desc.host;
    DgramFoot* df = (DgramFoot*)(c.desc.host + (size_t)m * sizeof(DgramMsg));
    uint32_t nm = 0, nf = 0, j = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t j0 = j;
        while (j < m && dgram[j] == i) ++j;
        const bool hs = handshake && has_handshake[i];
        const tamd_dgram_plan p = tamd_dgram_layout(type + j0, bytes + j0, j - j0, s->offs.data() + j0, seq_bytes[i], nonce_bytes[i], hs,
                                                    flag_bits[i], s->prm.max_datagram_bytes, pitch);
        rc[i] = (int32_t)p.rc;
        out_bytes[i] = p.out_bytes;
        message_bytes[i] = p.message_bytes;
        reliable_offset[i] = p.reliable_offset;
        reliable_bytes[i] = p.reliable_bytes;
        if (p.rc) continue;
        const uint64_t base = (uint64_t)(uintptr_t)dev_out + (uint64_t)i * pitch;
        for (uint32_t k = j0; k < j; ++k) {
            const uint32_t hb = type[k] == TAMD_DGRAM_T_RAW ? 0u : TAMD_DGRAM_FRAME;
            dm[nm++] = DgramMsg{base + s->offs[k], src[k], bytes[k], hb << 16 | (hb ? tamd_dgram_header(type[k], bytes[k]) : 0u)};
        }
        DgramFoot f;
        memset(&f, 0, sizeof(f));
        f.dst = base + p.message_bytes;
        f.len = tamd_dgram_footer(f.b, seq[i], seq_bytes[i], nonce[i], nonce_bytes[i], hs ? handshake + (size_t)i * TAMD_DGRAM_HANDSHAKE : nullptr,
                                  timestamp24[i], flag_bits[i]);
        df[nf++] = f;
    }
    if (!nf) return 0;
    // (the records of refused datagrams are left out: the footers move up behind the messages kept)
    DgramFoot* packed = (DgramFoot*)(c.desc.host + (size_t)nm * sizeof(DgramMsg));
    if (packed != df) memmove(packed, df, (size_t)nf * sizeof(DgramFoot));
    const size_t up = (size_t)nm * sizeof(DgramMsg) + (size_t)nf * sizeof(DgramFoot);
    const uint32_t per_block = 256u / 16u, blocks = (nm + nf + per_block - 1u) / per_block;
    const bool ok = c.run(kBuild, up, 0, [&] {
        hipLaunchKernelGGL(tamd_dgram_frames, dim3(blocks), dim3(256), 0, c.stream, (const DgramMsg*)c.desc.dev, nm,
                           (const DgramFoot*)(c.desc.dev + (size_t)nm * sizeof(DgramMsg)), nf);
    });
    return ok ? 0 : -4;
}

int tamd_dgram_parse(void* h, uint32_t n, const uint32_t* bytes, const uint32_t* offset, const void* dev, uint64_t pitch,
                     uint32_t mode, uint32_t cap, uint32_t* status, uint32_t* n_messages, uint32_t* reliable_offset,
                     uint32_t* reliable_bytes, uint32_t* table) {
    Framer* s = (Framer*)h;
    if (!s || !dev || mode > 1u || (n && (!bytes || !status || !n_messages || !reliable_offset || !reliable_bytes || (cap && !table))))
        return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk)) return e;
    HandleCore& c = s->core;
    const uint32_t maxb = s->prm.max_datagram_bytes;
    for (uint32_t i = 0; i < n; ++i)
        if (bytes[i] <= maxb && (uint64_t)(offset ? offset[i] : 0u) + bytes[i] > pitch) return -3;
    if (!n) return 0;
    const size_t heads = (size_t)n * sizeof(DgramOut), down = heads + (size_t)n * cap * sizeof(uint32_t);
    if (!c.room((size_t)n * sizeof(DgramSect), down)) return -4;
    DgramSect* d = (DgramSect*)c.desc.host;
    for (uint32_t i = 0; i < n; ++i)
        d[i] = DgramSect{(uint64_t)(uintptr_t)dev + (uint64_t)i * pitch + (offset ? offset[i] : 0u), bytes[i], bytes[i] <= maxb ? 0u : 1u};
    const bool ok = c.run(kParse, (size_t)n * sizeof(DgramSect), down, [&] {
        hipLaunchKernelGGL(tamd_dgram_sections, dim3((n + 63u) / 64u), dim3(512), 0, c.stream, (const DgramSect*)c.desc.dev, n, mode, cap,
                           (DgramOut*)c.out.dev, (uint32_t*)(c.out.dev + heads));
    });
    if (!ok) return -4;
    const DgramOut* o = (const DgramOut*)c.out.host;
    const uint32_t* t = (const uint32_t*)(c.out.host + heads);
    for (uint32_t i = 0; i < n; ++i) {
        const bool skipped = bytes[i] > maxb;
        status[i] = skipped ? 1u : o[i].status;
        n_messages[i] = skipped ? 0u : o[i].count;
        reliable_offset[i] = skipped ? 0u : o[i].rel_off;
        reliable_bytes[i] = skipped ? 0u : o[i].rel_bytes;
        const uint32_t kept = n_messages[i] < cap ? n_messages[i] : cap;
        if (kept) memcpy(table + (size_t)i * cap, t + (size_t)i * cap, (size_t)kept * sizeof(uint32_t));
    }
    return 0;
}

}  // extern "C"
