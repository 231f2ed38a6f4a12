// handle_check.cpp -- TEST ONLY.  The session backend's input handles (ResidentBackend::row,
// run_rows), which an affine pool computes instead of storing, against the table alloc_inputs
// used to fill: `pool` rows per side allocated in order, original i >= pool reading the row of
// i - pool.  The table is rebuilt here on a twin context that makes the same allocations.
//
// Every index is compared through row(); runs are compared through run_rows() in sequential order
// (the adds' order, which the backend's running position follows) and from random indices: with a
// layout, the first handle(s) and every packet's arena offset; without one, every handle.
//
// usage: handle_check   (prints one JSON line and exits 0, or the first difference and 1)
#include "resident_streams.h"

using namespace tamd;

static int check(uint32_t n, uint32_t pool, bool contig, uint64_t* compared) {
    Context twin, ctx;
    const uint64_t arena = 2ull * pool * 1344 + (16u << 20);
    twin.rows.init(arena);
    ctx.rows.init(arena);
    std::vector<RowId> want[2];
    for (int side = 0; side < 2; ++side) {
        want[side].assign(n, kNoRow);
        for (uint32_t i = 0; i < pool; ++i) want[side][i] = twin.alloc(1302);
        for (uint32_t i = pool; i < n; ++i) want[side][i] = want[side][i - pool];
    }
    ResidentBackend be;
    be.ctx = &ctx;
    be.contig = contig;
    if (!be.alloc_inputs(n, pool, 1302)) {
        printf("n %u pool %u: alloc_inputs failed\n", n, pool);
        return 1;
    }
    for (int side = 0; side < 2; ++side)
        for (uint32_t i = 0; i < n; ++i, ++*compared)
            if (be.row(side, i) != want[side][i]) {
                printf("n %u pool %u side %d index %u: row %u, table %u\n", n, pool, side, i, be.row(side, i), want[side][i]);
                return 1;
            }
    uint64_t rng = 88172645463325252ull + n * 31 + pool;
    auto draw = [&rng](uint32_t m) {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return (uint32_t)((rng >> 16) % m);
    };
    auto run = [&](int side, uint32_t index, uint32_t k) {
        uint64_t layout = 0;
        const RowId* rows = be.run_rows(side, index, k, &layout);
        const uint32_t named = layout ? (k < 2 ? k : 2u) : k;  // (with a layout the codecs read rows[0..2) only)
        for (uint32_t j = 0; j < named; ++j, ++*compared)
            if (rows[j] != want[side][index + j]) {
                printf("n %u pool %u side %d run %u+%u: handle %u is %u, table %u\n", n, pool, side, index, k, j, rows[j],
                       want[side][index + j]);
                return 1;
            }
        if (layout && !contig) {
            printf("n %u pool %u: a layout although contig is off\n", n, pool);
            return 1;
        }
        for (uint32_t j = 0; layout && j < k; ++j, ++*compared) {
            const uint32_t off = (uint32_t)(layout >> 32) + j * (uint32_t)layout;
            if (want[side][index + j] != want[side][index] + j || off != twin.rows.offset(want[side][index + j])) {
                printf("n %u pool %u side %d run %u+%u: packet %u at offset %u, table %u\n", n, pool, side, index, k, j, off,
                       twin.rows.offset(want[side][index + j]));
                return 1;
            }
        }
        return 0;
    };
    for (int side = 0; side < 2; ++side) {
        for (uint32_t i = 0; i < n;) {  // the adds' order: runs of 1-63, some spanning the pool's end
            const uint32_t k = std::min(n - i, 1 + draw(63));
            if (run(side, i, k)) return 1;
            i += k;
        }
        for (uint32_t t = 0; t < 2000; ++t) {  // any order: the running position must not be trusted
            const uint32_t i = draw(n), k = std::min(n - i, 1 + draw(63));
            if (run(side, i, k)) return 1;
            if (draw(2) && i + k < n && run(side, i + k, std::min(n - i - k, 1 + draw(63)))) return 1;
        }
    }
    return 0;
}

int main() {
    gf_init();
    // pool a power of two, not one, n no multiple of it, one pool for everything, a pool of one
    // row (never affine: the stored table), and each with the codecs checking runs themselves
    static const uint32_t cases[][2] = {{4096, 1024}, {5000, 1024}, {3000, 1000}, {2500, 1000}, {1000, 1000},
                                        {777, 777},   {300, 7},     {100, 2},     {64, 1},      {1, 1}};
    uint64_t compared = 0;
    for (const auto& c : cases)
        for (int contig = 0; contig < 2; ++contig)
            if (check(c[0], c[1], contig != 0, &compared)) return 1;
    printf("{\"cases\": %zu, \"compared\": %llu}\n", 2 * sizeof(cases) / sizeof(cases[0]), (unsigned long long)compared);
    return 0;
}
