// kernel_abi.h -- the records the helper kernels of kernels.hip read and write, and the
// prototypes of every kernel the host launches (device.cpp, server.cpp, batch.cpp, seal.cpp, recv.cpp): one definition for both
// sides.  The records are plain C; the prototypes need a HIP translation unit.
#pragma once
#include <stdint.h>

#include "program.h"
#include "serve.h"

/* tamd_gen_rows: row offset (64-B units), packet index, payload length, row capacity, seed_data */
typedef struct GenDesc { uint32_t row, index, len, cap; uint64_t seed; } GenDesc;
/* tamd_gather_rows: arena row, bytes, output offset */
typedef struct GatherDesc { uint32_t row, len, out; } GatherDesc;
/* tamd_scatter_rows: arena row, bytes, offset in the staging buffer */
typedef struct ScatterDesc { uint32_t row, len, src, pad; } ScatterDesc;
/* tamd_host_copy: pinned host address, arena row, bytes */
typedef struct HostCopyDesc { uint64_t host; uint32_t unit, len; } HostCopyDesc;
/* tamd_digest_rows: FNV-1a 64 over `len` bytes starting `skip` bytes into the row */
typedef struct DigestDesc { uint32_t row, skip, len, pad; } DigestDesc;
/* tamd_verify_rows: mode 0 a recovery packet of `len` bytes, 1 a recovered original */
typedef struct VerifyDesc { uint32_t row, len, mode, pad; } VerifyDesc;
typedef struct VerifyOut { uint64_t hash; uint32_t len, ok; } VerifyOut;
/* tamd_frame_rows (frame.hip): the caller's device address of the packet, arena row (64-B units),
   packet bytes, row capacity (a multiple of 64), raw != 0: no length header (a recovery packet) */
typedef struct FrameDesc { uint64_t src; uint32_t row, len, cap, raw; } FrameDesc;
/* tamd_unframe_rows: the caller's slot, arena row, the bytes the row may hold (its length header is
   checked against them); raw != 0: `upper` bytes are copied as they are (a recovery packet) */
typedef struct UnframeDesc { uint64_t dst; uint32_t row, upper, raw, pad; } UnframeDesc;
typedef struct UnframeOut { uint32_t len, status; } UnframeOut;  /* payload bytes, TAMD_FRAME_* (frame.h) */
/* tamd_gather_tails: the caller's device address of a packet and its bytes; 8 bytes out each */
typedef struct TailDesc { uint64_t src; uint32_t total, pad; } TailDesc;
/* tamd_seal_packets (seal.hip): the caller's device address of a datagram, its nonce, stream (the
   row of the key table), total bytes and ciphered bytes; skip != 0: refused on the host, untouched.
   One uint32 out each: the result code (seal.h TAMD_SEAL_*), or the plain tag.
   tamd_gather_footers reads TailDesc records and writes 24 bytes each. */
typedef struct SealDesc { uint64_t data, nonce; uint32_t stream, bytes, msg, skip; } SealDesc;
/* tamd_dgram_frames (dgram.hip): one record per message -- where its frame header goes, the caller's
   device address of its body (0: zeros), the body's bytes, and head = header bytes (0 or 2) << 16 |
   the header word -- then one per datagram: where its footer goes, the footer's bytes and the
   footer itself (dgram.h tamd_dgram_footer). */
typedef struct DgramMsg { uint64_t dst, src; uint32_t len, head; } DgramMsg;
typedef struct DgramFoot { uint64_t dst; uint32_t len, pad; uint8_t b[24]; } DgramFoot;
/* tamd_dgram_sections: the caller's device address of a message section and its bytes; skip != 0:
   not walked.  DgramOut and up to `cap` table entries out each. */
typedef struct DgramSect { uint64_t data; uint32_t bytes, skip; } DgramSect;
typedef struct DgramOut { uint32_t status, count, rel_off, rel_bytes; } DgramOut;
/* tamd_lz_place_ring (lz_place.hip): a stream's history ring (lz.h: TAMD_LZ_RING + TAMD_LZ_MIRROR
   bytes), the caller's device address of a message, the ring offset it lands at and its bytes */
typedef struct LzPlaceDesc { uint64_t ring, src; uint32_t slot, len; } LzPlaceDesc;
/* the kernels of recv.hip: one RecvDesc per datagram of a call (the caller's device address, the
   row of the key table and of the anti-replay state, total bytes).  tamd_rx_parse writes a
   RecvFields each (flags 0: an invalid datagram, nothing else meaningful); tamd_rx_resolve a
   RecvResult each, include/tonk_receive.h's tamd_recv_result.  RecvCall is the argument of all
   five kernels: the records, the call's streams as a CSR list (stream listed[j] owns items
   idx[start[j] .. start[j + 1]) in list order), what the steps hand on (the predicted nonces, the
   tag verdicts under them, the bytes to decipher), the handle's state and key tables and its three
   guard blocks with where their copy goes. */
typedef struct RecvDesc { uint64_t data; uint32_t stream, bytes; } RecvDesc;
typedef struct RecvFields { uint32_t partial_nonce, partial_seq, ts24; uint8_t flags, seq_bytes, nonce_bytes, handshake_bytes; } RecvFields;
typedef struct RecvResult {
    uint64_t nonce;
    uint32_t message_bytes, timestamp24, partial_seq;
    uint8_t flags, seq_bytes, nonce_bytes, handshake_bytes;
} RecvResult;
typedef struct RecvCall {
    const RecvDesc* d;
    const uint32_t *listed, *start, *idx;
    RecvFields* f;
    uint64_t* pred;
    uint32_t *tag_ok, *rc, *clen;
    RecvResult* res;
    uint64_t* state;
    const uint32_t* keys;
    const uint8_t* guard[3];
    uint8_t* guards_out;
    uint32_t n, n_listed, max_bytes, pad;
} RecvCall;

static_assert(sizeof(GenDesc) == 24, "GenDesc");
static_assert(sizeof(GatherDesc) == 12, "GatherDesc");
static_assert(sizeof(ScatterDesc) == 16, "ScatterDesc");
static_assert(sizeof(HostCopyDesc) == 16, "HostCopyDesc");
static_assert(sizeof(DigestDesc) == 16, "DigestDesc");
static_assert(sizeof(VerifyDesc) == 16, "VerifyDesc");
static_assert(sizeof(VerifyOut) == 16, "VerifyOut");
static_assert(sizeof(FrameDesc) == 24, "FrameDesc");
static_assert(sizeof(UnframeDesc) == 24, "UnframeDesc");
static_assert(sizeof(UnframeOut) == 8, "UnframeOut");
static_assert(sizeof(TailDesc) == 16, "TailDesc");
static_assert(sizeof(SealDesc) == 32, "SealDesc");
static_assert(sizeof(DgramMsg) == 24, "DgramMsg");
static_assert(sizeof(DgramFoot) == 40, "DgramFoot");
static_assert(sizeof(DgramSect) == 16, "DgramSect");
static_assert(sizeof(DgramOut) == 16, "DgramOut");
static_assert(sizeof(LzPlaceDesc) == 24, "LzPlaceDesc");
static_assert(sizeof(RecvDesc) == 16, "RecvDesc");
static_assert(sizeof(RecvFields) == 16, "RecvFields");
static_assert(sizeof(RecvResult) == 24, "RecvResult");

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
extern "C" {
__global__ void tamd_exec16(tamd_segments, const uint8_t*, uint32_t, uint8_t*, const uint32_t*, const uint8_t*,
                            unsigned long long*);
__global__ void tamd_exec24(tamd_segments, const uint8_t*, uint32_t, uint8_t*, const uint32_t*, const uint8_t*,
                            unsigned long long*);
__global__ void tamd_serve(const tamd_serve_args);
__global__ void tamd_gf_selftest(const uint32_t*, uint8_t*);
__global__ void tamd_gen_rows(const GenDesc*, uint32_t, uint8_t*, uint32_t);
__global__ void tamd_gather_rows(const GatherDesc*, uint32_t, const uint8_t*, uint8_t*);
__global__ void tamd_scatter_rows(const ScatterDesc*, uint32_t, const uint8_t*, uint8_t*);
__global__ void tamd_host_copy(const HostCopyDesc*, uint32_t, uint8_t*, uint32_t);
__global__ void tamd_copy_in(const uint4*, uint4*, uint32_t, const uint4*, uint4*, uint32_t);
__global__ void tamd_digest_rows(const DigestDesc*, uint32_t, const uint8_t*, unsigned long long*);
__global__ void tamd_verify_rows(const VerifyDesc*, uint32_t, const uint8_t*, VerifyOut*);
__global__ void tamd_frame_rows(const FrameDesc*, uint32_t, uint8_t*, uint32_t);
__global__ void tamd_unframe_rows(const UnframeDesc*, uint32_t, const uint8_t*, uint64_t, UnframeOut*, uint32_t, uint32_t);
__global__ void tamd_gather_tails(const TailDesc*, uint32_t, uint8_t*);
__global__ void tamd_seal_packets(const SealDesc*, uint32_t, const uint32_t*, uint32_t, uint32_t*);
__global__ void tamd_gather_footers(const TailDesc*, uint32_t, uint8_t*);
__global__ void tamd_dgram_frames(const DgramMsg*, uint32_t, const DgramFoot*, uint32_t);
__global__ void tamd_dgram_sections(const DgramSect*, uint32_t, uint32_t, uint32_t, DgramOut*, uint32_t*);
__global__ void tamd_lz_place_ring(const LzPlaceDesc*, uint32_t);
__global__ void tamd_rx_parse(const RecvCall);
__global__ void tamd_rx_predict(const RecvCall);
__global__ void tamd_rx_tag(const RecvCall);
__global__ void tamd_rx_resolve(const RecvCall);
__global__ void tamd_rx_decipher(const RecvCall);
__global__ void tamd_timed_region();
__global__ void tamd_nop();
}
#endif
