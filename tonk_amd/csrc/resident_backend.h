// resident_backend.h -- the wl::Runner backend over device-resident rows: one Encoder / Decoder
// pair on one Context, its originals in input rows that are generated once in HBM and borrowed
// by the codecs (never freed).  The session's streams run it (session.cpp adds what only a
// session has: host staging and the record-mode transcript), and so do the CPU stand-ins of the
// bench session, tests/native/cp_bench.cpp and prog_digest.cpp, where rows are just handles.
// Nothing here is virtual: the Runner is a template over the backend, and a derived struct
// shadows the calls it extends.
#pragma once

#include "decoder.h"
#include "prof.h"
#include "workload.h"

#include <memory>

namespace tamd {

struct ResidentBackend {
    struct RecRef { RecoveryOut out; };
    struct DecRef {};

    Context* ctx = nullptr;
    std::unique_ptr<Encoder> enc;
    std::unique_ptr<Decoder> dec;
    uint32_t pool = 0;        // input rows per side (original i reads row i mod pool)
    bool pool_affine = false; // each side's pool rows are consecutive handles at one arena stride:
    uint32_t pool_off[2] = {0, 0}, pool_stride = 0;  // row i mod pool at pool_off[side] + (i mod pool) * stride
    RowId pool_row0[2] = {kNoRow, kNoRow};           // and its handle is pool_row0[side] + (i mod pool)
    // Only when the pool is not affine (an arena that could not place the rows back to back): the
    // handle of every original, per side.  An affine pool computes them.
    std::vector<RowId> rows_[2];
    uint32_t pool_mask = 0;   // pool - 1 when the pool is a power of two: i mod pool is one AND
    // Otherwise the adds' running position: they are sequential, so the next call's index is where
    // the last one ended, and its i mod pool is kept instead of divided out.
    struct Cursor { uint32_t index = ~0u, slot = 0; } cur_[2];
    RowId run_rows_[2];              // the first two handles of a run whose layout is given
    std::vector<RowId> run_scratch_; // all of them, for a run the codecs check themselves
    bool nobatch = false;     // tools' nobatch=1: single adds only (the runner's fallback path)
    bool contig = true;       // tools' contig=0: the codecs check every run's contiguity themselves
    uint64_t alg_bytes = 0, payload_bytes = 0;
    std::vector<RecoveredPacket*> got_;  // the packets of the last successful dec_decode

    // Input rows: `pool_n` rows of `row_bytes` per side, allocated back to back (each side an
    // array of equal slots in packet order, so runs of a window's packets sit at a fixed stride:
    // one ACCR instruction per run); original i >= pool_n reads the row of i - pool_n.  False
    // when the arena is full.
    bool alloc_inputs(uint32_t n, uint32_t pool_n, uint32_t row_bytes) {
        for (int side = 0; side < 2; ++side) {
            std::vector<RowId>& rows = rows_[side];
            rows.assign(pool_n, kNoRow);
            for (uint32_t i = 0; i < pool_n; ++i)
                if ((rows[i] = ctx->alloc(row_bytes)) == kNoRow) return false;
        }
        pool = pool_n;
        pool_mask = pool && !(pool & (pool - 1)) ? pool - 1 : 0;
        pool_affine = pool >= 2;
        for (int side = 0; side < 2 && pool_affine; ++side) {
            const std::vector<RowId>& rows = rows_[side];
            const uint32_t o0 = ctx->rows.offset(rows[0]), stride = ctx->rows.offset(rows[1]) - o0;
            pool_affine = consecutive_handles(rows.data(), pool) && stride > 0 &&
                          ctx->rows.affine(rows[0], pool, stride) && (!side || stride == pool_stride);
            pool_off[side] = o0;
            pool_row0[side] = rows[0];
            pool_stride = stride;
        }
        for (int side = 0; side < 2; ++side) {
            std::vector<RowId>& rows = rows_[side];
            if (pool_affine) {
                std::vector<RowId>().swap(rows);  // (computed: row())
            } else {
                rows.resize(n);
                for (uint32_t i = pool_n; i < n; ++i) rows[i] = rows[i - pool_n];
            }
        }
        return true;
    }
    // The input row of original `index` on a side (0: encoder, 1: decoder).
    RowId row(int side, uint32_t index) const {
        if (!pool_affine) return rows_[side][index];
        return pool_row0[side] + (pool_mask ? index & pool_mask : index % pool);
    }
    // index mod pool for an add of k originals from `index` on.
    uint32_t pool_slot(int side, uint32_t index, uint32_t k) {
        if (pool_mask) return index & pool_mask;
        Cursor& c = cur_[side];
        const uint32_t slot = c.index == index ? c.slot : index % pool;
        c.index = index + k;
        c.slot = slot + k;
        if (c.slot >= pool) c.slot = c.slot - pool < pool ? c.slot - pool : c.slot % pool;
        return slot;
    }
    // The handles of a run (rows[0..k)) and its layout.  A run that does not wrap the input pool
    // is consecutive handles at one stride: the codecs get its layout instead of checking and
    // looking it up (the row table is cold), and read rows[0] (rows[1] for what follows a window's
    // first packet) only.  Any other run gets every handle and layout 0.
    const RowId* run_rows(int side, uint32_t index, uint32_t k, uint64_t* layout) {
        *layout = 0;
        if (!pool_affine) return &rows_[side][index];
        const uint32_t slot = pool_slot(side, index, k);
        if (contig && slot + k <= pool) {
            *layout = (uint64_t)(pool_off[side] + slot * pool_stride) << 32 | pool_stride;
            run_rows_[0] = pool_row0[side] + slot;
            run_rows_[1] = run_rows_[0] + 1;
            return run_rows_;
        }
        run_scratch_.resize(k);
        for (uint32_t j = 0, m = slot; j < k; ++j) {
            run_scratch_[j] = pool_row0[side] + m;
            if (++m == pool) m = 0;
        }
        return run_scratch_.data();
    }

    int enc_add(uint32_t index, uint32_t len, uint32_t* col) {
        const uint32_t hb = length_header_bytes(len);
        TAMD_PROF_SCOPE(kEncAdd);
        const Result r = enc->add(row(0, index), hb + len, hb, len, nullptr, col, true);
        if (r == kSuccess) {
            alg_bytes += hb + len;
            payload_bytes += len;
        }
        return r;
    }
    bool enc_add_run(uint32_t index, uint32_t k, uint32_t len, uint32_t* col0) {
        if (nobatch) return false;
        const uint32_t hb = length_header_bytes(len);
        TAMD_PROF_SCOPE(kEncAdd);
        uint64_t layout;
        const RowId* rows = run_rows(0, index, k, &layout);
        if (!enc->add_run(rows, k, hb + len, hb, len, true, col0, layout)) return false;
        alg_bytes += (uint64_t)(hb + len) * k;
        payload_bytes += (uint64_t)len * k;
        return true;
    }
    bool dec_add_run(uint32_t col0, uint32_t index, uint32_t k, uint32_t len) {
        if (nobatch) return false;
        const uint32_t hb = length_header_bytes(len);
        TAMD_PROF_SCOPE(kDecAddOrig);
        uint64_t layout;
        const RowId* rows = run_rows(1, index, k, &layout);
        if (!dec->add_run_inorder(col0, rows, k, hb + len, hb, len, true, layout)) return false;
        alg_bytes += (uint64_t)(hb + len) * k;
        return true;
    }
    int enc_encode(RecRef& r) {
        TAMD_PROF_SCOPE(kEncEncode);
        const Result rc = enc->encode(r.out);
        if (rc == kSuccess) alg_bytes += r.out.total();
        return rc;
    }
    int enc_ack(const uint8_t* buf, uint32_t n, uint32_t* next) {
        TAMD_PROF_SCOPE(kEncAck);
        return enc->acknowledge(buf, n, next);
    }
    int enc_is_ready() { return enc->remaining_slots() <= 2 ? (int)kMaxPacketsReached : 0; }
    int dec_add_original(uint32_t col, uint32_t index, uint32_t len) {
        const uint32_t hb = length_header_bytes(len);
        TAMD_PROF_SCOPE(kDecAddOrig);
        bool took = false;
        const Result r = dec->add_original(col, row(1, index), hb + len, hb, len, nullptr, &took, true);
        alg_bytes += hb + len;
        return r;
    }
    void recovery_lost(const RecRef& r) { ctx->rows.free_deferred(r.out.row); }
    int dec_add_recovery(const RecRef& r) {
        uint8_t tail[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t tl = r.out.total() < 8 ? r.out.total() : 8;
        memcpy(tail + tl - r.out.footer_len, r.out.footer, r.out.footer_len);
        TAMD_PROF_SCOPE(kDecAddRec);
        bool took = false;
        const Result rc = dec->add_recovery(r.out.row, r.out.total(), tail, nullptr, &took);
        if (!took) ctx->rows.free_deferred(r.out.row);
        alg_bytes += r.out.total();
        return rc;
    }
    int dec_is_ready() {
        TAMD_PROF_SCOPE(kDecIsReady);
        return dec->is_ready();
    }
    int dec_decode(std::vector<uint32_t>& nums, DecRef&) {
        TAMD_PROF_SCOPE(kDecDecode);
        got_.clear();
        const Result rc = dec->decode(got_);
        if (rc != kSuccess) got_.clear();
        for (RecoveredPacket* rp : got_) {
            nums.push_back(rp->packet_num);
            alg_bytes += rp->framed_upper;
        }
        return rc;
    }
    int dec_ack(uint8_t* buf, uint32_t limit, uint32_t* used) {
        TAMD_PROF_SCOPE(kDecAck);
        return dec->ack(buf, limit, used);
    }
    void stats(uint64_t e[9], uint64_t d[11]) { enc->stats(e, 9); dec->stats(d, 11); }
    uint64_t vclock = 0;
    void set_time(uint64_t ms) {
        if (!vclock) enc->set_clock(&vclock);
        vclock = ms;
    }
    int enc_retransmit(uint32_t* num, uint32_t* bytes, const uint8_t** data) {
        StoredOriginal o;
        const Result rc = enc->retransmit(&o);
        if (rc == kSuccess) {
            *num = o.column;
            *bytes = o.bytes - o.header_bytes;
            *data = nullptr;  // the payload lives in HBM; the runner regenerates it for the digest
        }
        return rc;
    }
};

}  // namespace tamd
